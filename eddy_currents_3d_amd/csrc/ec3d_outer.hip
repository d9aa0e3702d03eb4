// ec3d_outer.hip — the outer iteration: the real right-preconditioned BiCGSTAB with restart (src/solvers.f90:24-50 with
// P, S replaced by their preconditioned images in the products with A and the X update):
//   p^ = M p; v = Op p^; alpha = rho / (r0.v); s = r - alpha v; [exit on ||s|| / ||b||: x += alpha p^]
//   s^ = M s; t = Op s^; omega = (t.s)/(t.t); x += alpha p^ + omega s^; r = s - omega t; [exit on ||r|| / ||b||]
//   beta = (alpha / omega) (r.r0) / rho; p = r + beta (p - omega v); restart as the reference.
// Sums and exits stay on the device; launches past an exit are no-ops.  Stated once here for its four users
// (ec3d_outer.hpp: OuterRun, ec3d_outer_iteration):
//   the multigrid-preconditioned Poisson solve (ec3d_mg.hip): M the V-cycle in fp64 or fp32, Op = k_mg_spmv_dot, which
//     sums the dot partials in the product's own launch;
//   the block-multigrid A-V solve (ec3d_mg.hip, section 10): M the block cycle, Op = ec3d_launch_spmv;
//   the null projection's adjoint solves (ec3d_null.hip, sections 16, 16a): Op = ec3d_launch_spmv_t, M = N or M = I.
// p^ and s^ may be fp32 (the fp32 V-cycle): k_mg_xr widens them on load; every other operand and operation is fp64.
//
// The reducing kernels are grid-strided over rows (thread t of workgroup b takes the rows b * 256 + t + m * 256 * gridDim.x
// in increasing m); their workgroup sums and the scalar launch's collapse are ec3d_stream.hpp's.
#include "ec3d_outer.hpp"
#include "ec3d_recurrence.hpp"

namespace {

// partials of a.y (slot 0) and, with two, y.y (slot 1), the products summed as k_mg_spmv_dot sums them
__global__ __launch_bounds__(256) void k_avmg_dot(int64_t n, Gate g, const double *__restrict__ a,
                                                  const double *__restrict__ y, int two, double *__restrict__ part)
{
    __shared__ double lds[4];
    if (gated_off(g)) return;
    double d0 = 0.0, d1 = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const double s = y[r];
        d0 = d0 + a[r] * s;
        d1 = d1 + s * s;
    }
    d0 = stream_block_sum(d0, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = d0;
    if (two) {
        d1 = stream_block_sum(d1, lds);
        if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = d1;
    }
}

// s = r - alpha v; partial s.s.  Bytes per row: 16 read, 8 written.
__global__ __launch_bounds__(256) void k_mg_s(int64_t n, Gate g, const SolverState *st, const double *__restrict__ r,
                                              const double *__restrict__ v, double *__restrict__ s,
                                              double *__restrict__ part)
{
    __shared__ double lds[4];
    if (gated_off(g)) return;
    const double alpha = st->alpha;
    double d = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const double sv = r[q] - alpha * v[q];
        s[q] = sv;
        d = d + sv * sv;
    }
    d = stream_block_sum(d, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = d;
}

// x = x + alpha p^ + omega s^;  r = s - omega t;  partials r.r, r.r0.  After the ||S|| exit of this iteration only
// x = x + alpha p^ (src/solvers.f90:34-37).  Bytes per row: x, p^, s^, s, t, r0 read 48, x, r written 16 = 64 B.
// TX = float: p^ and s^ of the fp32 V-cycle, widened on load (56 B).
template <class TX = double>
__global__ __launch_bounds__(256) void k_mg_xr(int64_t n, int it, const SolverState *st, double *__restrict__ x,
                                               const TX *__restrict__ ph, const TX *__restrict__ sh,
                                               const double *__restrict__ s, const double *__restrict__ t,
                                               const double *__restrict__ r0, double *__restrict__ r,
                                               double *__restrict__ part)
{
    __shared__ double lds[4];
    const int stop = st->stop_iter;
    if (stop < it) return;
    const double alpha = st->alpha, omega = st->omega;
    const bool s_exit = stop == it;
    double d0 = 0.0, d1 = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        if (s_exit) {
            x[q] = x[q] + alpha * (double)ph[q];
            continue;
        }
        x[q] = x[q] + alpha * (double)ph[q] + omega * (double)sh[q];
        const double rv = s[q] - omega * t[q];
        r[q] = rv;
        d0 = d0 + rv * rv;
        d1 = d1 + rv * r0[q];
    }
    if (s_exit) return;
    d0 = stream_block_sum(d0, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = d0;
    d1 = stream_block_sum(d1, lds);
    if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = d1;
}

// p = r + beta (p - omega v), or the restart r0 = r, p = r (src/solvers.f90:46-49).  Bytes per row: 24 read, 8 (16) written.
__global__ __launch_bounds__(256) void k_mg_p(int64_t n, Gate g, const SolverState *st, const MgScalars *ms,
                                              const double *__restrict__ r, const double *__restrict__ v,
                                              double *__restrict__ p, double *__restrict__ r0)
{
    if (gated_off(g)) return;
    const double beta = ms->beta, omega = st->omega;
    const bool restart = ms->restart != 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        if (restart) {
            p[q] = r[q];
            r0[q] = r[q];
        } else {
            p[q] = r[q] + beta * (p[q] - omega * v[q]);
        }
    }
}

// The scalar steps, one workgroup; partials summed in a fixed order (thread-strided, then the workgroup tree).
enum { MG_ALPHA = 0, MG_SEXIT = 1, MG_OMEGA = 2, MG_REXIT = 3 };
__global__ __launch_bounds__(256) void k_mg_scalar(int stage, Gate g, SolverState *st, MgScalars *ms,
                                                   const double *__restrict__ part, int nparts, double *hist,
                                                   int64_t hist_cap)
{
    __shared__ double lds[4];
    if (gated_off(g)) return;
    const int nslot = (stage == MG_OMEGA || stage == MG_REXIT) ? 2 : 1;
    double v[2] = {0.0, 0.0};
    for (int sl = 0; sl < nslot; ++sl) {
        v[sl] = stream_block_sum(stream_strided_sum(part + (int64_t)sl * nparts, nparts), lds);
    }
    if (threadIdx.x != 0) return;
    const int it = g.it;
    const int64_t h = (int64_t)(it - 1) * 2;
    switch (stage) {
    // the rules themselves: ec3d_recurrence.hpp
    case MG_ALPHA: st->alpha = ec3d_alpha(st->rr0[it & 1], v[0]); break; // (:31-32)
    case MG_SEXIT: {
        const Ec3dNorm s = ec3d_snorm_step(v[0], st->bnorm, st->tol);
        if (it - 1 < hist_cap) hist[h] = s.norm;
        if (s.exit) mg_stop_publish(st, it, 1); // (:34-38)
        break;
    }
    case MG_OMEGA: st->omega = ec3d_omega(v[0], v[1]); break; // (:40)
    case MG_REXIT: {
        const Ec3dNorm rn = ec3d_rnorm_step(v[0], st->bnorm, st->tol);
        if (it - 1 < hist_cap) hist[h + 1] = rn.norm;
        st->rnorm = rn.norm;
        if (rn.exit) { // (:43)
            mg_stop_publish(st, it, 2);
            break;
        }
        const Ec3dBeta b = ec3d_beta_step(st->alpha, st->omega, v[1], st->rr0[it & 1], v[0], st->bnorm, st->tol); // (:45-49)
        ms->beta = b.beta;
        ms->restart = b.restart;
        if (b.restart) st->restarts = st->restarts + 1;
        st->rr0[(it + 1) & 1] = b.rr0_next;
        break;
    }
    }
}

} // namespace

int ec3d_outer_begin(ec3d_ctx *c, const OuterRun &k, double tol)
{
    hipStream_t s = c->stream;
    const unsigned nb = dot_blocks(k.n);
    const size_t bytes = (size_t)k.n * sizeof(double);
    EC3D_HIP(hipMemsetAsync(k.x, 0, bytes, s));
    EC3D_HIP(hipMemcpyAsync(k.r0, k.r, bytes, hipMemcpyDeviceToDevice, s));
    EC3D_HIP(hipMemcpyAsync(k.p, k.r, bytes, hipMemcpyDeviceToDevice, s));
    // b.b and r.r of the set-up (slots P_BB, P_RR_INIT) are the same sum: r = b
    k_avmg_dot<<<nb, 256, 0, s>>>(k.n, Gate{nullptr, 0, 0}, k.r, k.r, 1, k.part);
    ec3d_launch_setup(c->state, RedSrc{k.part, (int)nb, 1, (int)nb, nullptr}, tol, s);
    EC3D_HIP(hipGetLastError());
    return 0;
}

// The SpMV launches in front are not gated: past an exit nothing reads what they write.
void ec3d_outer_behind(ec3d_ctx *c, const OuterRun &k, int it, int half, bool dotted)
{
    hipStream_t s = c->stream;
    const int64_t n = k.n;
    const unsigned nb = dot_blocks(n);
    const Gate g{c->state, it, half};
    const auto scalar = [&](int stage) {
        k_mg_scalar<<<1, 256, 0, s>>>(stage, g, c->state, k.scal, k.part, (int)nb, k.hist, k.hist_cap);
    };
    if (!dotted) k_avmg_dot<<<nb, 256, 0, s>>>(n, g, half ? k.s : k.r0, half ? k.t : k.v, half, k.part);
    if (half == 0) {
        scalar(MG_ALPHA);
        k_mg_s<<<nb, 256, 0, s>>>(n, g, c->state, k.r, k.v, k.s, k.part);
        scalar(MG_SEXIT);
        return;
    }
    scalar(MG_OMEGA);
    if (k.f32)
        k_mg_xr<<<nb, 256, 0, s>>>(n, it, c->state, k.x, (const float *)k.ph, (const float *)k.sh, k.s, k.t, k.r0, k.r, k.part);
    else
        k_mg_xr<<<nb, 256, 0, s>>>(n, it, c->state, k.x, (const double *)k.ph, (const double *)k.sh, k.s, k.t, k.r0, k.r, k.part);
    scalar(MG_REXIT);
    k_mg_p<<<nb, 256, 0, s>>>(n, g, c->state, k.scal, k.r, k.v, k.p, k.r0);
}
