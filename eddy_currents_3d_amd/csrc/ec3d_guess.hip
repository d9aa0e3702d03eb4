// ec3d_guess.hip — a solve started from the projection onto earlier solutions (ec3d_set_guess_history).
//
// The handle keeps k <= m pairs (Q_i, A Q_i), oldest first, the A Q_i orthonormal.  In front of a solve
//     R = B - A X,  c_i = (A Q_i).R,  X = X + c_1 Q_1 + ... + c_k Q_k
// takes out of the initial residual what the stored directions explain (Fischer's projection in GCR form: A need not
// be symmetric); behind it Q_new = X - X_start and A Q_new are orthogonalised against the stored pairs by two passes of
// classical Gram-Schmidt, scaled to ||A Q_new|| = 1 and stored, the oldest pair giving way when k = m.  The iteration
// in between is untouched.
//
// Kernels.  Streaming launches, sums and the rows that count (r < n: row_owned of ec3d_kernels.hip on a handle that is no
// slab; slabs are refused): ec3d_stream.hpp.  The history vectors are zero filled when they are allocated and written on
// rows < n only.  One partial per workgroup and sum; k_guess_collapse, one workgroup, collapses them
// (tests/guess_history_numpy.py restates the whole).
//
// The host reads EC3D_GS_N scalars back once per solve (ec3d_guess_update); the decisions that kernels depend on -- a zero
// right-hand side, a sum that is not finite, a new pair too small to keep -- are taken on the device from the same scalars.
#include "ec3d_stream.hpp"

#include <cmath>
#include <cstring>

// the scalars of a solve (doubles in GuessHistory::scal)
enum {
    GS_COEF = 0,      // [8] c_i of the projection
    GS_RR = 8,        // R.R in front of the projection
    GS_BB = 9,        // B.B (the residual launch's partials)
    GS_SKIP = 10,     // 1: B.B = 0 or a sum was not finite -- no kernel below stores anything
    GS_SETUP = 11,    // [3] bnorm, tol, rnorm of the solve's own set-up (SolverState)
    GS_H = 16,        // [8] Gram-Schmidt coefficients of the pass under way
    GS_N0 = 24,       // ||A Q_new||^2 before the passes
    GS_N1 = 25,       // ... and behind them
    GS_INV = 26,      // 1 / ||A Q_new||
    GS_KEEP = 27,     // 1: the pair is stored
    EC3D_GS_N = 32
};

namespace {

struct GPtrs {
    const double *p[EC3D_GUESS_MAX_DEPTH];
};
struct GIdx {
    int at[EC3D_GUESS_MAX_DEPTH + 1]; // where a collapsed sum goes in the scalars; -1: nowhere
};

// partials of a_i . v (i < K) and of v . v: slot j of workgroup b at part[j * gridDim.x + b]
template <int K>
__global__ __launch_bounds__(EC3D_THREADS) void k_guess_dots(GPtrs a, const double *__restrict__ v, int64_t n, int64_t nchunk,
                                                            double *__restrict__ part)
{
    __shared__ double lds[(K + 1) * 4];
    double acc[K + 1];
#pragma unroll
    for (int i = 0; i <= K; ++i) acc[i] = 0.0;
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        stream_d2 s[K > 0 ? K : 1];
#pragma unroll
        for (int i = 0; i < K; ++i) s[i] = stream_load(a.p[i], r);
        const stream_d2 x = stream_mask(stream_load(v, r), r, n);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const stream_d2 q = stream_mask(s[i], r, n);
            acc[i] = acc[i] + q.x * x.x;
            acc[i] = acc[i] + q.y * x.y;
        }
        acc[K] = acc[K] + x.x * x.x;
        acc[K] = acc[K] + x.y * x.y;
    }
    stream_block_sum<K + 1>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i <= K; ++i) part[(int64_t)i * gridDim.x + blockIdx.x] = acc[i];
    }
}

__device__ __forceinline__ bool gfinite(double v) { return v - v == 0.0; }

// One workgroup: the nv sums of `count` partials each go to scal[idx.at[j]].  Then, by mode:
//   1 (projection): B.B from the residual launch's partials; B.B = 0 -> every c_i = 0 and GS_SKIP
//   2 (norm behind the passes): GS_INV and GS_KEEP from GS_N0 and GS_N1
// Any mode: a sum that is not finite sets GS_SKIP.
__global__ __launch_bounds__(EC3D_THREADS) void k_guess_collapse(const double *__restrict__ part, int count, int nv, GIdx idx,
                                                                int mode, const double *__restrict__ bb_part, int bb_count,
                                                                double *__restrict__ scal)
{
    __shared__ double lds[4];
    bool skip = false;
    for (int j = 0; j < nv; ++j) {
        const double a = stream_block_sum(stream_strided_sum(part + (int64_t)j * count, count), lds);
        if (threadIdx.x == 0 && idx.at[j] >= 0) {
            scal[idx.at[j]] = a;
            skip |= !gfinite(a);
        }
    }
    double bb = 0.0;
    if (mode == 1) bb = stream_block_sum(stream_strided_sum(bb_part, bb_count), lds);
    if (threadIdx.x != 0) return;
    if (mode == 1) {
        scal[GS_BB] = bb;
        if (bb == 0.0) { // src/solvers.f90:23: the solve returns at once, X keeps its bits
            for (int j = 0; j < EC3D_GUESS_MAX_DEPTH; ++j) scal[GS_COEF + j] = 0.0;
            skip = true;
        }
    }
    if (mode == 2) {
        const double n0 = sqrt(scal[GS_N0]), n1 = sqrt(scal[GS_N1]);
        const bool keep = scal[GS_SKIP] == 0.0 && !skip && gfinite(n0) && gfinite(n1) && n1 > EC3D_GUESS_MIN_NEW * n0;
        scal[GS_INV] = keep ? 1.0 / n1 : 0.0;
        scal[GS_KEEP] = keep ? 1.0 : 0.0;
    }
    if (skip) scal[GS_SKIP] = 1.0;
}

// X = X + c_1 Q_1 + ... + c_K Q_K, every term a rounded product and a rounded sum of its own
template <int K>
__global__ __launch_bounds__(EC3D_THREADS) void k_guess_axpy_x(GPtrs q, const double *__restrict__ scal, double *__restrict__ x,
                                                              int64_t n, int64_t nchunk)
{
    if (scal[GS_SKIP] != 0.0) return;
    double c[K];
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = scal[GS_COEF + i];
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        stream_d2 s[K];
#pragma unroll
        for (int i = 0; i < K; ++i) s[i] = stream_load(q.p[i], r);
        stream_d2 v = stream_load(x, r);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            v.x = v.x + c[i] * s[i].x;
            v.y = v.y + c[i] * s[i].y;
        }
        stream_store(x, r, n, v);
    }
}

// S = X - X_start on rows < n
__global__ __launch_bounds__(EC3D_THREADS) void k_guess_diff(const double *__restrict__ x, const double *__restrict__ xs,
                                                            double *__restrict__ s, int64_t n, int64_t nchunk)
{
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        const stream_d2 a = stream_load(x, r), b = stream_load(xs, r);
        stream_store(s, r, n, stream_d2{a.x - b.x, a.y - b.y});
    }
}

// One Gram-Schmidt pass: AS = AS - h_1 AQ_1 - ... - h_K AQ_K and S = S - h_1 Q_1 - ... in the same order; leaves the
// partials of AS.AS
template <int K>
__global__ __launch_bounds__(EC3D_THREADS) void k_guess_gs(GPtrs q, GPtrs aq, const double *__restrict__ scal,
                                                          double *__restrict__ s, double *__restrict__ as, int64_t n,
                                                          int64_t nchunk, double *__restrict__ part)
{
    __shared__ double lds[4];
    if (scal[GS_SKIP] != 0.0) return; // (uniform; the collapse behind this launch has the flag too)
    double h[K];
#pragma unroll
    for (int i = 0; i < K; ++i) h[i] = scal[GS_H + i];
    double acc = 0.0;
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        stream_d2 a[K], b[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            a[i] = stream_load(aq.p[i], r);
            b[i] = stream_load(q.p[i], r);
        }
        stream_d2 va = stream_load(as, r), vs = stream_load(s, r);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            va.x = va.x - h[i] * a[i].x;
            va.y = va.y - h[i] * a[i].y;
            vs.x = vs.x - h[i] * b[i].x;
            vs.y = vs.y - h[i] * b[i].y;
        }
        stream_store(as, r, n, va);
        stream_store(s, r, n, vs);
        va = stream_mask(va, r, n);
        acc = acc + va.x * va.x;
        acc = acc + va.y * va.y;
    }
    acc = stream_block_sum(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// the new pair, scaled, into its slot -- when it is kept
__global__ __launch_bounds__(EC3D_THREADS) void k_guess_scale(const double *__restrict__ scal, const double *__restrict__ s,
                                                             const double *__restrict__ as, double *__restrict__ q,
                                                             double *__restrict__ aq, int64_t n, int64_t nchunk)
{
    if (scal[GS_KEEP] == 0.0) return;
    const double inv = scal[GS_INV];
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int64_t r = stream_chunk_row(ch);
        const stream_d2 a = stream_load(s, r), b = stream_load(as, r);
        stream_store(q, r, n, stream_d2{a.x * inv, a.y * inv});
        stream_store(aq, r, n, stream_d2{b.x * inv, b.y * inv});
    }
}

template <int K> struct Launch {
    static void dots(int k, unsigned g, hipStream_t st, const GPtrs &a, const double *v, int64_t n, int64_t nc, double *part)
    {
        if (k == K) k_guess_dots<K><<<g, EC3D_THREADS, 0, st>>>(a, v, n, nc, part);
        else Launch<K - 1>::dots(k, g, st, a, v, n, nc, part);
    }
    static void axpy_x(int k, unsigned g, hipStream_t st, const GPtrs &q, const double *scal, double *x, int64_t n, int64_t nc)
    {
        if (k == K) k_guess_axpy_x<K><<<g, EC3D_THREADS, 0, st>>>(q, scal, x, n, nc);
        else Launch<K - 1>::axpy_x(k, g, st, q, scal, x, n, nc);
    }
    static void gs(int k, unsigned g, hipStream_t st, const GPtrs &q, const GPtrs &aq, const double *scal, double *s, double *as,
                   int64_t n, int64_t nc, double *part)
    {
        if (k == K) k_guess_gs<K><<<g, EC3D_THREADS, 0, st>>>(q, aq, scal, s, as, n, nc, part);
        else Launch<K - 1>::gs(k, g, st, q, aq, scal, s, as, n, nc, part);
    }
};
template <> struct Launch<0> {
    static void dots(int, unsigned g, hipStream_t st, const GPtrs &a, const double *v, int64_t n, int64_t nc, double *part)
    {
        k_guess_dots<0><<<g, EC3D_THREADS, 0, st>>>(a, v, n, nc, part);
    }
    static void axpy_x(int, unsigned, hipStream_t, const GPtrs &, const double *, double *, int64_t, int64_t) {}
    static void gs(int, unsigned, hipStream_t, const GPtrs &, const GPtrs &, const double *, double *, double *, int64_t, int64_t,
                   double *) {}
};
typedef Launch<EC3D_GUESS_MAX_DEPTH> L;

// the stored pairs, oldest first
void stored(const GuessHistory &g, GPtrs &q, GPtrs &aq)
{
    for (int i = 0; i < EC3D_GUESS_MAX_DEPTH; ++i) {
        const int p = (g.head + std::min(i, std::max(g.k - 1, 0))) % std::max(g.depth, 1);
        q.p[i] = g.k > 0 ? g.q[(size_t)p].get() : nullptr;
        aq.p[i] = g.k > 0 ? g.aq[(size_t)p].get() : nullptr;
    }
}

void collapse(ec3d_ctx *c, int nv, const GIdx &idx, int mode)
{
    GuessHistory &g = c->guess;
    const RedSrc bb = ec3d_src_of(c, EC3D_BY_SPMV); // who left B.B: the residual launch
    k_guess_collapse<<<1, EC3D_THREADS, 0, c->stream>>>(g.part, g.wgs, nv, idx, mode, bb.base + (int64_t)P_BB * bb.slot_mul,
                                                        bb.count, g.scal);
}

} // namespace

void ec3d_guess_free(ec3d_ctx *c)
{
    GuessHistory &g = c->guess;
    g.q.clear();
    g.aq.clear();
    g.xs.reset();
    g.part.reset();
    g.scal.reset();
    g.host.reset();
    g.len = 0;
    g.k = g.head = 0;
}

// no pair stored, every vector zero as when it was allocated (the allocations stay)
int ec3d_guess_clear(ec3d_ctx *c)
{
    GuessHistory &g = c->guess;
    g.k = g.head = 0;
    if (g.len == 0) return 0;
    for (auto &v : g.q) EC3D_HIP(hipMemsetAsync(v, 0, (size_t)g.len * sizeof(double), c->stream));
    for (auto &v : g.aq) EC3D_HIP(hipMemsetAsync(v, 0, (size_t)g.len * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(g.xs, 0, (size_t)g.len * sizeof(double), c->stream));
    return 0;
}

static int guess_alloc(ec3d_ctx *c)
{
    GuessHistory &g = c->guess;
    if (g.len == c->A.n_pad && (int)g.q.size() == g.depth) return 0;
    ec3d_guess_free(c);
    const size_t len = (size_t)c->A.n_pad;
    g.q.resize((size_t)g.depth);
    g.aq.resize((size_t)g.depth);
    for (auto &v : g.q) EC3D_HIP(v.alloc(len));
    for (auto &v : g.aq) EC3D_HIP(v.alloc(len));
    EC3D_HIP(g.xs.alloc(len));
    g.wgs = ec3d_stream_wgs(c->A.n_pad);
    EC3D_HIP(g.part.alloc((size_t)(EC3D_GUESS_MAX_DEPTH + 1) * g.wgs));
    EC3D_HIP(g.scal.alloc(EC3D_GS_N));
    EC3D_HIP(g.host.alloc(EC3D_GS_N));
    g.len = c->A.n_pad;
    return ec3d_guess_clear(c);
}

// In front of ec3d_launch_begin: X_start kept, X moved along the stored directions.
int ec3d_guess_project(ec3d_ctx *c, const MatView &A)
{
    int rc = guess_alloc(c);
    if (rc) return rc;
    GuessHistory &g = c->guess;
    double **v = c->vec;
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE;
    g.last = ec3d_guess_info{};
    g.last.depth = g.depth;
    g.last.used = g.k;
    EC3D_HIP(hipMemsetAsync(g.scal, 0, EC3D_GS_N * sizeof(double), c->stream));
    EC3D_HIP(hipMemcpyAsync(g.xs, v[EC3D_VEC_X], (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (g.k == 0) return 0;
    GPtrs q, aq;
    stored(g, q, aq);
    ec3d_launch_residual(A, c->sweep_s, v[EC3D_VEC_X], v[EC3D_VEC_B], v[EC3D_VEC_R], v[EC3D_VEC_R0], v[EC3D_VEC_P], c->partials,
                         c->stream);
    L::dots(g.k, (unsigned)g.wgs, c->stream, aq, v[EC3D_VEC_R], n, nc, g.part);
    GIdx idx;
    for (int i = 0; i <= EC3D_GUESS_MAX_DEPTH; ++i) idx.at[i] = i < g.k ? GS_COEF + i : i == g.k ? GS_RR : -1;
    collapse(c, g.k + 1, idx, 1);
    L::axpy_x(g.k, (unsigned)g.wgs, c->stream, q, g.scal, v[EC3D_VEC_X], n, nc);
    EC3D_HIP(hipGetLastError());
    return 0;
}

// Behind ec3d_launch_begin: what the solve's own set-up found (||B||, ||B - A X|| of the X it starts from).
int ec3d_guess_note_setup(ec3d_ctx *c)
{
    EC3D_HIP(hipMemcpyAsync(c->guess.scal.get() + GS_SETUP, &c->state.get()->bnorm, 3 * sizeof(double), hipMemcpyDeviceToDevice,
                            c->stream));
    return 0;
}

// Behind the solve (every pending X update applied).  store: false after a zero right-hand side -- nothing is stored.
int ec3d_guess_update(ec3d_ctx *c, const MatView &A, bool store)
{
    GuessHistory &g = c->guess;
    double **v = c->vec;
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE;
    const unsigned G = (unsigned)g.wgs;
    double *S = v[EC3D_VEC_S], *AS = v[EC3D_VEC_AS]; // free between two solves: Q_new and A Q_new are made here
    const int slot = g.k < g.depth ? (g.head + g.k) % g.depth : g.head;
    if (store) {
        GPtrs q, aq;
        stored(g, q, aq);
        k_guess_diff<<<G, EC3D_THREADS, 0, c->stream>>>(v[EC3D_VEC_X], g.xs, S, n, nc);
        ec3d_launch_spmv(A, c->sweep_s, S, AS, c->stream);
        GIdx idx;
        for (int pass = 0; pass < (g.k > 0 ? 2 : 1); ++pass) {
            L::dots(g.k, G, c->stream, aq, AS, n, nc, g.part);
            for (int i = 0; i <= EC3D_GUESS_MAX_DEPTH; ++i)
                idx.at[i] = i < g.k ? GS_H + i : (i == g.k && pass == 0) ? GS_N0 : -1;
            collapse(c, g.k + 1, idx, 0);
            if (g.k > 0) L::gs(g.k, G, c->stream, q, aq, g.scal, S, AS, n, nc, g.part);
        }
        for (int i = 0; i <= EC3D_GUESS_MAX_DEPTH; ++i) idx.at[i] = i == 0 ? GS_N1 : -1;
        collapse(c, 1, idx, 2); // (k = 0: k_guess_dots<0> left AS.AS in slot 0 -- the norm behind no pass is the norm before)
        k_guess_scale<<<G, EC3D_THREADS, 0, c->stream>>>(g.scal, S, AS, g.q[(size_t)slot], g.aq[(size_t)slot], n, nc);
        EC3D_HIP(hipGetLastError());
    }
    EC3D_HIP(hipMemcpyAsync(g.host, g.scal, EC3D_GS_N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    const double *h = g.host;
    ec3d_guess_info &o = g.last;
    for (int i = 0; i < g.k; ++i) o.coef[i] = h[GS_COEF + i];
    const double bnorm = h[GS_SETUP];
    o.res_after = bnorm == 0.0 ? 0.0 : h[GS_SETUP + 2] / bnorm; // (||B|| = 0: nothing to be relative to)
    o.res_before = bnorm == 0.0 ? 0.0 : g.k > 0 ? std::sqrt(h[GS_RR]) / std::sqrt(h[GS_BB]) : o.res_after;
    bool finite = true;
    for (int i = 0; i < g.k; ++i) finite = finite && std::isfinite(h[GS_COEF + i]) && (!store || std::isfinite(h[GS_H + i]));
    if (g.k > 0) finite = finite && std::isfinite(h[GS_RR]);
    if (store) finite = finite && std::isfinite(h[GS_N0]) && std::isfinite(h[GS_N1]);
    if (!finite) {
        o.kept = -1;
        int rc = ec3d_guess_clear(c);
        if (rc) return rc;
    } else if (store && h[GS_KEEP] != 0.0) {
        o.kept = 1;
        if (g.k < g.depth) ++g.k;
        else g.head = (g.head + 1) % g.depth;
    } else {
        o.kept = 0;
    }
    o.stored = g.k;
    return 0;
}

extern "C" int ec3d_set_guess_history(ec3d_handle c, int32_t depth)
{
    if (!c || depth < 0 || depth > EC3D_GUESS_MAX_DEPTH) {
        ec3d_set_error(!c ? std::string("ec3d_set_guess_history: null handle")
                          : "ec3d_set_guess_history: depth " + std::to_string(depth) + " is outside 0 .. " +
                                std::to_string(EC3D_GUESS_MAX_DEPTH));
        return 2;
    }
    if (c->in_multi) {
        ec3d_set_error("ec3d_set_guess_history: this handle is a slab of ec3d_multi; the history's sums would need every rank's");
        return 4;
    }
    int rc = ec3d_single_rank_only(c, "ec3d_set_guess_history");
    if (rc) return rc;
    if (depth == c->guess.depth) return 0;
    EC3D_HIP(hipSetDevice(c->device));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    ec3d_guess_free(c); // any change of the depth: the pairs go, the next solve allocates for the new depth
    c->guess.depth = depth;
    c->guess.last = ec3d_guess_info{};
    c->guess.last.depth = depth;
    return 0;
}

extern "C" int ec3d_get_guess_history(ec3d_handle c, ec3d_guess_info *info)
{
    if (!c || !info) {
        ec3d_set_error("ec3d_get_guess_history: null handle or info");
        return 2;
    }
    *info = c->guess.last;
    info->depth = c->guess.depth;
    info->stored = c->guess.k;
    return 0;
}
