// ec3d_null.hip — the left null vectors of the structured A-V matrix, taken out of every solve's initial residual
// (ec3d_set_null_projection).
//
// Set-up, once per matrix (ec3d_null_prepare): the connected components of the conducting cells on the host; per
// component the adjoint solve A^T y = -A^T e_m from y = 0 -- the outer iteration of ec3d_outer.hip around
// ec3d_launch_spmv_t (ec3d_outer_begin, ec3d_adjoint_iteration), in the work vectors R, R0, P, AP, S, AS, which are free
// between two solves (X and B are the caller's and stay); M = I, or with ec3d_set_null_precond M = N, a block hierarchy
// this set-up builds and releases (ec3d_null_mg_*, section 16a) -- then w = y + e_m, its residual, and classical
// Gram-Schmidt against the vectors kept so far.  In front of a solve (ec3d_null_project): c_i = Q_i.R,
// R = R - c_1 Q_1 - ... - c_k Q_k, R0 = R, P = R, and the partials of R.R where the solve's set-up kernel looks for them.
//
// Sums and streaming launches: ec3d_stream.hpp.  One partial per workgroup and vector; k_null_collapse, one workgroup per
// vector, collapses them.
#include "ec3d_outer.hpp"

#include <chrono>
#include <cmath>

namespace {

__device__ __forceinline__ stream_d2 nload(const double *p, int64_t r, int64_t n) { return stream_mask(stream_load(p, r), r, n); }

// partials of (qbase + i * qstride) . v for i = blockIdx.y: part[i * gridDim.x + b]
__global__ __launch_bounds__(EC3D_THREADS) void k_null_dots(const double *__restrict__ qbase, int64_t qstride,
                                                           const double *__restrict__ v, int64_t n, int64_t nchunk,
                                                           double *__restrict__ part)
{
    __shared__ double lds[4];
    const double *q = qbase + (int64_t)blockIdx.y * qstride;
    double acc = 0.0;
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        const stream_d2 a = nload(q, r, n), x = nload(v, r, n);
        acc = acc + a.x * x.x;
        acc = acc + a.y * x.y;
    }
    acc = stream_block_sum(acc, lds);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// workgroup i: out[i] = the sum of its `count` partials
__global__ __launch_bounds__(EC3D_THREADS) void k_null_collapse(const double *__restrict__ part, int count,
                                                               double *__restrict__ out)
{
    __shared__ double lds[4];
    const double a = stream_block_sum(stream_strided_sum(part + (int64_t)blockIdx.x * count, count), lds);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// v = v - c_0 Q_0 - ... - c_{k-1} Q_{k-1}, every term a rounded product and a rounded difference of its own; r0, p (or
// null): copies of the new v; rr (or null): workgroup b's partial of v.v at rr[b] -- EVERY workgroup of the launch writes
// one, also those beyond the last chunk (+0.0), because the consumer adds gridDim.x of them
__global__ __launch_bounds__(EC3D_THREADS) void k_null_sub(const double *__restrict__ qbase, int64_t qstride, int k,
                                                          const double *__restrict__ coef, double *__restrict__ v,
                                                          double *__restrict__ r0, double *__restrict__ p, int64_t n,
                                                          int64_t nchunk, double *__restrict__ rr)
{
    __shared__ double lds[4];
    double acc = 0.0;
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        stream_d2 x = nload(v, r, n);
        for (int i = 0; i < k; ++i) {
            const double ci = coef[i];
            const stream_d2 a = nload(qbase + (int64_t)i * qstride, r, n);
            x.x = x.x - ci * a.x;
            x.y = x.y - ci * a.y;
        }
        stream_store(v, r, n, x);
        if (r0) stream_store(r0, r, n, x);
        if (p) stream_store(p, r, n, x);
        acc = acc + x.x * x.x;
        acc = acc + x.y * x.y;
    }
    if (!rr) return;
    acc = stream_block_sum(acc, lds);
    if (threadIdx.x == 0) rr[blockIdx.x] = acc;
}

// y = f * x on rows < n
__global__ __launch_bounds__(EC3D_THREADS) void k_null_scale(const double *__restrict__ x, double f, double *__restrict__ y,
                                                            int64_t n, int64_t nchunk)
{
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        const stream_d2 a = nload(x, r, n);
        stream_store(y, r, n, stream_d2{f * a.x, f * a.y});
    }
}

// v[row] = v[row] + 1 (w = y + e_m)
__global__ void k_null_add_one(double *v, int64_t row) { v[row] = v[row] + 1.0; }

// connected components (6-neighbourhood) of the conducting cells, in scan order of their first cell; cells: the
// conducting cells' REFERENCE cell indices in scan order.  Returns per component its cells in scan order.
std::vector<std::vector<int64_t>> components(const std::vector<int64_t> &cells, int64_t sdx, int64_t sdy, int64_t sdz)
{
    std::vector<int32_t> label((size_t)(sdx * sdy * sdz), -2); // -2: not conducting, -1: not visited
    for (int64_t q : cells) label[(size_t)q] = -1;
    std::vector<std::vector<int64_t>> out;
    std::vector<int64_t> stack;
    for (int64_t q0 : cells) {
        if (label[(size_t)q0] != -1) continue;
        const int32_t id = (int32_t)out.size();
        out.emplace_back();
        label[(size_t)q0] = id;
        stack.assign(1, q0);
        while (!stack.empty()) {
            const int64_t q = stack.back();
            stack.pop_back();
            out[(size_t)id].push_back(q);
            const int64_t i = q % sdx, j = (q / sdx) % sdy, k = q / (sdx * sdy);
            const int64_t nb[6] = {i > 0 ? q - 1 : -1, i + 1 < sdx ? q + 1 : -1, j > 0 ? q - sdx : -1,
                                   j + 1 < sdy ? q + sdx : -1, k > 0 ? q - sdx * sdy : -1, k + 1 < sdz ? q + sdx * sdy : -1};
            for (int64_t p : nb)
                if (p >= 0 && label[(size_t)p] == -1) {
                    label[(size_t)p] = id;
                    stack.push_back(p);
                }
        }
        std::sort(out[(size_t)id].begin(), out[(size_t)id].end());
    }
    return out;
}

// coef[i] = (qbase + i * qstride) . v for i < k; host (or null): where they are read back to, which synchronises
int dots_to_host(ec3d_ctx *c, const double *qbase, int64_t qstride, int k, const double *v, double *host)
{
    NullProjection &N = c->nullp;
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE;
    k_null_dots<<<dim3((unsigned)N.wgs, (unsigned)k), EC3D_THREADS, 0, c->stream>>>(qbase, qstride, v, n, nc, N.part);
    k_null_collapse<<<(unsigned)k, EC3D_THREADS, 0, c->stream>>>(N.part, N.wgs, N.coef);
    EC3D_HIP(hipGetLastError());
    if (host) {
        EC3D_HIP(hipMemcpyAsync(host, N.coef, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        EC3D_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// The six work vectors the adjoint solves ran in, zero on rows [0, n) again.  A solve that ended well left +0.0 in the
// rows no unknown lives in; one that went to NaN or inf did not (0 * NaN), and the iteration's kernels read those rows.
int scrub(ec3d_ctx *c)
{
    for (int w : {EC3D_VEC_R, EC3D_VEC_R0, EC3D_VEC_P, EC3D_VEC_AP, EC3D_VEC_S, EC3D_VEC_AS})
        EC3D_HIP(hipMemsetAsync(c->vec[w], 0, (size_t)c->A.n * sizeof(double), c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    ec3d_run_reset(c);
    c->run.forget_ap();
    return 0;
}

int build(ec3d_ctx *c)
{
    NullProjection &N = c->nullp;
    const auto t_start = std::chrono::steady_clock::now();
    const double null_tol = N.null_tol;
    ec3d_null_free(c);
    EC3D_HIP(hipSetDevice(c->device));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    const MatView A = c->A.view();
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE;
    std::vector<NullSeed> seeds;
    {
        const int rc = ec3d_null_seeds(c, seeds);
        if (rc) return rc;
    }
    const int ncomp = (int)seeds.size();
    N.last.found = ncomp;
    N.last.reported = std::min(ncomp, EC3D_NULL_MAX_REPORT);
    N.len = len;
    N.wgs = ec3d_stream_wgs(len);
    if (ncomp == 0) { // no conductor: A has no such null vector, the projection is the identity
        N.built = true;
        N.last.built = 1;
        return 0;
    }
    EC3D_HIP(N.q.alloc((size_t)ncomp * len));
    EC3D_HIP(hipMemsetAsync(N.q, 0, (size_t)ncomp * len * sizeof(double), c->stream));
    EC3D_HIP(N.part.alloc((size_t)ncomp * N.wgs));
    EC3D_HIP(N.coef.alloc((size_t)ncomp + 2));
    EC3D_HIP(N.kpart.alloc((size_t)2 * dot_blocks(n)));
    EC3D_HIP(N.kscal.alloc(1));
    EC3D_HIP(hipMemsetAsync(N.kscal, 0, sizeof(MgScalars), c->stream));
    double **v = c->vec;
    const int64_t cap = (int64_t)(20.0 * std::cbrt((double)c->n_ref)) + 2000;
    const int64_t total = cap + 1; // src/solvers.f90:25-29: itmax + 1 iterations
    const auto apply = [&](const double *x, double *y) { ec3d_launch_spmv_t(A, n, x, y, c->stream); };
    // N of ec3d_set_null_precond: a hierarchy of this set-up's own, gone when build returns
    struct OwnedMg {
        ec3d_mg *m = nullptr;
        ~OwnedMg() { ec3d_null_mg_delete(m); }
    } nmg;
    if (N.precond != EC3D_NULL_PRECOND_NONE) {
        const auto t_h = std::chrono::steady_clock::now();
        const int rc = ec3d_null_mg_build(c, N.precond, N.pre, N.post, N.coarse, &nmg.m);
        if (rc) {
            ec3d_null_free(c);
            return rc;
        }
        ec3d_null_mg_dims(nmg.m, &N.levels, N.dims);
        N.hierarchy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_h).count();
    }
    std::vector<double> h((size_t)ncomp + 2);
    int kept = 0;
    for (int ci = 0; ci < ncomp; ++ci) {
        const int64_t row = seeds[(size_t)ci].row, seed_ref = seeds[(size_t)ci].seed_ref;
        double *w = N.q.get() + (size_t)kept * len; // the next free slot: y, then w, then Q_kept
        // right-hand side -A^T e_m into R (e_m in S, A^T e_m in AS)
        EC3D_HIP(hipMemsetAsync(v[EC3D_VEC_S], 0, (size_t)n * sizeof(double), c->stream));
        k_null_add_one<<<1, 1, 0, c->stream>>>(v[EC3D_VEC_S], row);
        apply(v[EC3D_VEC_S], v[EC3D_VEC_AS]);
        k_null_scale<<<(unsigned)N.wgs, EC3D_THREADS, 0, c->stream>>>(v[EC3D_VEC_AS], -1.0, v[EC3D_VEC_R], n, nc);
        const OuterRun K{n, w, v[EC3D_VEC_R], v[EC3D_VEC_R0], v[EC3D_VEC_P], v[EC3D_VEC_AP], v[EC3D_VEC_S], v[EC3D_VEC_AS],
                         v[EC3D_VEC_P], v[EC3D_VEC_S], false, N.kpart, N.kscal, nullptr, 0}; // p^ = p, s^ = s; no history
        int rc = ec3d_outer_begin(c, K, null_tol);
        if (rc) return rc;
        SolverState st;
        int64_t launched = 0;
        bool stopped = false;
        while (launched < total && !stopped) {
            const int64_t m = std::min<int64_t>(16, total - launched);
            for (int64_t i = 0; i < m; ++i) ec3d_adjoint_iteration(c, nmg.m, K, (int)(++launched));
            EC3D_HIP(hipGetLastError());
            EC3D_HIP(hipMemcpyAsync(&st, c->state, sizeof st, hipMemcpyDeviceToHost, c->stream));
            EC3D_HIP(hipStreamSynchronize(c->stream));
            stopped = st.stop_iter != INT_MAX;
        }
        if (!stopped) {
            char msg[320];
            snprintf(msg, sizeof msg, "null projection: the adjoint solve of conducting component %d (seed row %lld) did not reach "
                     "null_tol = %.3g within %lld iterations (||r|| / ||A^T e_m|| = %.3g); its left null vector is not used",
                     ci, (long long)seed_ref, null_tol, (long long)cap, st.bnorm > 0.0 ? st.rnorm / st.bnorm : 0.0);
            ec3d_null_free(c);
            EC3D_HIP(hipStreamSynchronize(c->stream)); // (N goes with this return: nothing of it may still run)
            if ((rc = scrub(c))) return rc;
            ec3d_set_error(msg);
            return EC3D_NULL_E_SETUP;
        }
        k_null_add_one<<<1, 1, 0, c->stream>>>(w, row);
        // ||A^T w|| / ||w||, then Gram-Schmidt against the vectors kept
        apply(w, v[EC3D_VEC_AS]);
        if ((rc = dots_to_host(c, v[EC3D_VEC_AS], 0, 1, v[EC3D_VEC_AS], &h[0]))) return rc;
        if ((rc = dots_to_host(c, w, 0, 1, w, &h[1]))) return rc;
        const double n0 = std::sqrt(h[1]), res = std::sqrt(h[0]) / n0;
        if (kept > 0) {
            if ((rc = dots_to_host(c, N.q, len, kept, w, nullptr))) return rc;
            k_null_sub<<<(unsigned)N.wgs, EC3D_THREADS, 0, c->stream>>>(N.q, len, kept, N.coef, w, nullptr, nullptr, n, nc, nullptr);
            if ((rc = dots_to_host(c, w, 0, 1, w, &h[1]))) return rc;
        }
        const double n1 = std::sqrt(h[1]);
        const bool keep = std::isfinite(n0) && std::isfinite(n1) && n1 > EC3D_NULL_MIN_KEEP * n0;
        if (keep) {
            k_null_scale<<<(unsigned)N.wgs, EC3D_THREADS, 0, c->stream>>>(w, 1.0 / n1, w, n, nc);
            ++kept;
        } else {
            EC3D_HIP(hipMemsetAsync(w, 0, (size_t)len * sizeof(double), c->stream)); // the slot is free again
        }
        if (ci < EC3D_NULL_MAX_REPORT) {
            N.last.seed_row[ci] = seed_ref;
            N.last.iterations[ci] = st.stop_iter;
            N.last.residual[ci] = res;
            N.last.was_kept[ci] = keep ? 1 : 0;
        }
    }
    EC3D_HIP(hipGetLastError());
    {
        const int rc = scrub(c);
        if (rc) return rc;
    }
    N.kept = kept;
    N.built = true;
    N.last.built = 1;
    N.last.kept = kept;
    N.last.dropped = ncomp - kept;
    N.last.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return 0;
}

} // namespace

void ec3d_null_free(ec3d_ctx *c)
{
    NullProjection &N = c->nullp;
    N.q.reset();
    N.part.reset();
    N.coef.reset();
    N.kpart.reset();
    N.kscal.reset();
    N.built = false;
    N.kept = 0;
    N.len = 0;
    N.wgs = 0;
    N.last = ec3d_null_info{};
    N.levels = 0;
    N.hierarchy_ms = 0.0;
}

int ec3d_null_seeds(ec3d_ctx *c, std::vector<NullSeed> &seeds)
{
    // the conducting cells: device cell of U unknown m, scan order (ec3d_setup_rhs)
    std::vector<int32_t> dcell((size_t)c->n_cond);
    if (c->n_cond) EC3D_HIP(hipMemcpy(dcell.data(), c->cond_cell, dcell.size() * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> cells(dcell.size());
    for (size_t m = 0; m < dcell.size(); ++m) cells[m] = c->ref_cell(dcell[m]);
    const auto comps = components(cells, c->sdx, c->sdy, c->sdz);
    seeds.clear();
    for (const auto &cc : comps) {
        const int64_t mid = cc[cc.size() / 2];
        const int64_t um = std::lower_bound(cells.begin(), cells.end(), mid) - cells.begin();
        seeds.push_back(NullSeed{3 * c->A.sav_nC + c->dev_cell(mid), 3 * (int64_t)c->plane * c->planes() + um});
    }
    return 0;
}

int ec3d_null_eligible(const ec3d_ctx *c, const char *who, bool set_text)
{
    if (!ec3d_own_handle(c)) {
        if (set_text)
            ec3d_set_error(std::string(who) + ": this handle holds a z-slab (or is a slab of ec3d_multi); the left null "
                                              "vectors and their sums would need every rank's");
        return 4;
    }
    if (!c->have_matrix) return 0;
    if (!(c->A.sav && c->A.sav_box) || c->from_csr || c->poisson_full || c->sdx <= 0) {
        if (set_text)
            ec3d_set_error(std::string(who) + ": needs the structured A-V form of ec3d_assemble (not a Poisson, CSR or "
                                              "bands + tail matrix)");
        return EC3D_NULL_E_MATRIX;
    }
    return 0;
}

int ec3d_null_prepare(ec3d_ctx *c)
{
    int rc = ec3d_null_eligible(c, "ec3d_solve (null projection on)", true);
    if (rc) return rc;
    if (c->nullp.built) return 0;
    return build(c);
}

int ec3d_null_project(ec3d_ctx *c)
{
    NullProjection &N = c->nullp;
    if (N.kept == 0) return 0;
    double **v = c->vec;
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE;
    k_null_dots<<<dim3((unsigned)N.wgs, (unsigned)N.kept), EC3D_THREADS, 0, c->stream>>>(N.q, N.len, v[EC3D_VEC_R], n, nc, N.part);
    k_null_collapse<<<(unsigned)N.kept, EC3D_THREADS, 0, c->stream>>>(N.part, N.wgs, N.coef);
    // R.R of the projected residual where k_setup adds it: one partial per workgroup the residual launch counted
    const RedSrc src = ec3d_src_of(c, EC3D_BY_SPMV);
    k_null_sub<<<(unsigned)src.count, EC3D_THREADS, 0, c->stream>>>(N.q, N.len, N.kept, N.coef, v[EC3D_VEC_R], v[EC3D_VEC_R0],
                                                                   v[EC3D_VEC_P], n, nc,
                                                                   c->partials.get() + (int64_t)P_RR_INIT * src.slot_mul);
    EC3D_HIP(hipGetLastError());
    return 0;
}

int ec3d_null_note(ec3d_ctx *c, double bnorm)
{
    NullProjection &N = c->nullp;
    N.last.removed = 0.0;
    if (N.kept == 0 || bnorm == 0.0) return 0;
    std::vector<double> h((size_t)N.kept);
    EC3D_HIP(hipMemcpy(h.data(), N.coef, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    double s = 0.0;
    for (double x : h) s += x * x;
    N.last.removed = std::sqrt(s) / bnorm;
    return 0;
}

extern "C" int ec3d_set_null_projection(ec3d_handle c, int32_t on, double null_tol)
{
    if (!c) {
        ec3d_set_error("ec3d_set_null_projection: null handle");
        return 2;
    }
    if (!on) {
        c->nullp.on = 0; // Q stays with the matrix: switching on again costs nothing
        return 0;
    }
    int rc = ec3d_null_eligible(c, "ec3d_set_null_projection", true);
    if (rc) {
        c->nullp.on = 0;
        return rc;
    }
    const double tol = null_tol > 0.0 ? null_tol : 1e-10;
    if (tol != c->nullp.null_tol && c->nullp.built) {
        EC3D_HIP(hipSetDevice(c->device));
        EC3D_HIP(hipStreamSynchronize(c->stream));
        ec3d_null_free(c); // another accuracy: the vectors are made again
    }
    c->nullp.on = 1;
    c->nullp.null_tol = tol;
    return 0;
}

extern "C" int ec3d_set_null_precond(ec3d_handle c, int32_t kind, int32_t pre, int32_t post, int32_t coarse_sweeps)
{
    if (!c || kind < EC3D_NULL_PRECOND_NONE || kind > EC3D_NULL_PRECOND_BLOCK_MG_A || pre < 0 || post < 0 || coarse_sweeps < 0) {
        ec3d_set_error(!c ? "ec3d_set_null_precond: null handle"
                          : "ec3d_set_null_precond: unknown kind or negative sweep count");
        return 2;
    }
    int rc = ec3d_null_eligible(c, "ec3d_set_null_precond", true);
    if (rc) return rc;
    NullProjection &N = c->nullp;
    if (kind == N.precond && pre == N.pre && post == N.post && coarse_sweeps == N.coarse) return 0;
    EC3D_HIP(hipSetDevice(c->device));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    if (kind != EC3D_NULL_PRECOND_NONE && c->have_matrix) { // what the block hierarchy refuses is known now: build it once
        ec3d_mg *m = nullptr;
        if ((rc = ec3d_null_mg_build(c, kind, pre, post, coarse_sweeps, &m))) return rc;
        ec3d_null_mg_delete(m);
    }
    if (N.built) ec3d_null_free(c); // another set-up: the vectors are made again
    N.precond = kind;
    N.pre = pre;
    N.post = post;
    N.coarse = coarse_sweeps;
    return 0;
}

extern "C" int ec3d_get_null_precond(ec3d_handle c, int32_t *kind, int32_t *levels, int32_t *dims, double *hierarchy_ms)
{
    if (!c) {
        ec3d_set_error("ec3d_get_null_precond: null handle");
        return 2;
    }
    const NullProjection &N = c->nullp;
    if (kind) *kind = N.precond;
    if (levels) *levels = N.levels;
    for (int q = 0; dims && q < 3 * N.levels; ++q) dims[q] = N.dims[q];
    if (hierarchy_ms) *hierarchy_ms = N.hierarchy_ms;
    return 0;
}

extern "C" int ec3d_get_null_projection(ec3d_handle c, ec3d_null_info *info)
{
    if (!c || !info) {
        ec3d_set_error("ec3d_get_null_projection: null handle or info");
        return 2;
    }
    *info = c->nullp.last;
    info->on = c->nullp.on;
    info->null_tol = c->nullp.null_tol;
    info->built = c->nullp.built ? 1 : 0;
    return 0;
}

extern "C" int ec3d_left_null_vector(ec3d_handle c, int32_t index, double *w_host)
{
    int rc = ec3d_need_matrix(c, "ec3d_left_null_vector");
    if (rc) return rc;
    if ((rc = ec3d_null_eligible(c, "ec3d_left_null_vector", true))) return rc;
    if (!c->nullp.built) {
        if (!c->nullp.on) {
            ec3d_set_error("ec3d_left_null_vector: no vectors yet and the projection is off (ec3d_set_null_projection)");
            return 2;
        }
        if ((rc = build(c))) return rc;
    }
    if (index < 0 || index >= c->nullp.kept || !w_host) {
        ec3d_set_error("ec3d_left_null_vector: index " + std::to_string(index) + " is outside the " +
                       std::to_string(c->nullp.kept) + " vectors kept");
        return 2;
    }
    if ((rc = ec3d_vec_d2h(c, w_host, c->nullp.q.get() + (size_t)index * c->nullp.len))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
