// ec3d_mg.hip — geometric multigrid preconditioner of the single-component operator (ec3d_assemble_poisson) and the
// right-preconditioned BiCGSTAB-with-restart that uses it (ec3d_set_preconditioner).
//
// Hierarchy: level 0 is the handle's own matrix; every coarser level is the same device assembly
// (ec3d_assemble_poisson_level) at half the cells and twice the spacing on each axis that is even and >= 8, with the
// same BND -- a rediscretisation, not a Galerkin product.  Coarsening stops when no axis can halve or a level has at
// most EC3D_MG_COARSE_ROWS rows; that level is solved by one single-workgroup launch in LDS.
//
// One V-cycle from x = 0 on level l (tests/mg_numpy.py restates it operation by operation; no reduction enters it, so
// the device result is bit-identical to the restatement):
//   w = pre sweeps of (red, black) on b, the first red half from zero being w = b / d on red, 0 on black (k_mg_smooth);
//   b_{l+1} = mean of the children's b - A w, the fine residual never stored (k_mg_restrict);
//   V-cycle on level l + 1 (the coarsest: coarse_sweeps sweeps of red, black, black, red; k_mg_coarse);
//   x = w + x_{l+1}[parent] fused with the first post half-sweep (black) (k_mg_prolong), the red half that completes
//   that sweep, then post - 1 more sweeps of (black, red) (k_mg_smooth).
// Colour of cell (i, j, k) is (i + j + k) & 1, red = 0.  A half-sweep updates one colour from the other only, so it
// runs in place; the prolongation reads w and writes x (another buffer), because its black rows read red neighbours
// the same launch corrects.
//
// A row of a level is read from the level's own device format: class byte + coefficient table in LDS (dictionary form,
// what every coarse level uses) or the seven band streams (ec3d_set_format(h, 0)).  Bands in offset order
// (-z, -y, -x, diag, +x, +y, +z); a neighbour beyond the box contributes nothing (its coefficient is 0 there anyway).
#include "../../include/ec3d_hip.h"
#include "ec3d_internal.hpp"

#include <array>
#include <climits>
#include <cmath>
#include <cstring>

#define EC3D_MG_COARSE_ROWS 4096 // x of the coarsest level in LDS (32 KiB), b and class bytes in registers
#define EC3D_MG_COARSE_THREADS 1024
#define EC3D_MG_MAXCLS 32        // dictionary classes a level may have (the single-component operator has 28)
#define EC3D_MG_DOT_BLOCKS 2048  // workgroups of the reducing kernels (grid-stride)

struct MgOp {
    int sdx, sdy, sdz;
    int64_t n, n_pad, kdz;
    const uint8_t *cls;   // dictionary form: coefficient q of row r = table[cls[r] * 7 + q]
    const double *table;
    int ncls;
    const double *bands;  // band form (cls == nullptr): bands[q * n_pad + r]
};

struct MgLevel {
    DevMatrix A;          // level 0: unused (the handle's matrix)
    MgOp op;
    int f[3] = {1, 1, 1}; // coarsening factor towards the next level per axis (1 or 2)
    double delta[3] = {0, 0, 0};
    double *x = nullptr, *w = nullptr, *b = nullptr; // coarse levels: inside ec3d_mg::vec_base
};

struct MgScalars {
    double beta;
    int restart;
    int pad_;
};

struct ec3d_mg {
    int pre = 2, post = 2, coarse = 16;
    std::vector<MgLevel> lev;
    double *vec_base = nullptr; // coarse x, w, b per level, then the fine w, p^, s^
    double *w0 = nullptr, *ph = nullptr, *sh = nullptr;
    double *part = nullptr;     // 2 * EC3D_MG_DOT_BLOCKS
    MgScalars *scal = nullptr;
};

namespace {

// ---- gating: every launch of iteration `it` is a no-op once the solve has stopped before it (strict = 0) or at it
// (strict = 1: the launches behind the ||S|| exit's check).  st == nullptr: not inside a solve (ec3d_precond_apply).
struct Gate {
    const SolverState *st;
    int it, strict;
};
__device__ __forceinline__ bool gated_off(const Gate &g)
{
    if (!g.st) return false;
    const int s = g.st->stop_iter; // written by an earlier launch on the stream: an ordinary load sees it
    return g.strict ? s <= g.it : s < g.it;
}
__device__ __forceinline__ void mg_stop_publish(SolverState *st, int it, int kind)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(&st->stop_iter),
                       (unsigned long long)(unsigned)it | ((unsigned long long)(unsigned)kind << 32), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void load_table(const MgOp &A, double *tbl)
{
    if (!A.cls) return;
    for (int q = threadIdx.x; q < A.ncls * 7; q += blockDim.x) tbl[q] = A.table[q];
    __syncthreads();
}
template <bool DICT> __device__ __forceinline__ void row_coefs(const MgOp &A, const double *tbl, int64_t r, double (&c)[7])
{
    if constexpr (DICT) {
        const double *t = tbl + 7 * (int)A.cls[r];
#pragma unroll
        for (int q = 0; q < 7; ++q) c[q] = t[q];
    } else {
#pragma unroll
        for (int q = 0; q < 7; ++q) c[q] = A.bands[(size_t)q * A.n_pad + r];
    }
}
struct Pos {
    int i, j, k;
};
__device__ __forceinline__ Pos pos_of(const MgOp &A, int64_t r)
{
    const unsigned ur = (unsigned)r, sx = (unsigned)A.sdx;
    const unsigned ij = ur % (unsigned)A.kdz;
    return Pos{(int)(ij % sx), (int)(ij / sx), (int)(ur / (unsigned)A.kdz)};
}
// x at the six neighbours in offset order (-z, -y, -x, +x, +y, +z); 0 beyond the box
template <class LD>
__device__ __forceinline__ void neighbours(const MgOp &A, const Pos &p, int64_t r, LD ld, double (&v)[6])
{
    v[0] = p.k > 0 ? ld(r - A.kdz) : 0.0;
    v[1] = p.j > 0 ? ld(r - A.sdx) : 0.0;
    v[2] = p.i > 0 ? ld(r - 1) : 0.0;
    v[3] = p.i + 1 < A.sdx ? ld(r + 1) : 0.0;
    v[4] = p.j + 1 < A.sdy ? ld(r + A.sdx) : 0.0;
    v[5] = p.k + 1 < A.sdz ? ld(r + A.kdz) : 0.0;
}
// Gauss-Seidel value of a row: (b - sum of the off-diagonal terms in offset order) / d
__device__ __forceinline__ double gs_value(const double (&c)[7], const double (&v)[6], double b)
{
    double t = b;
    t = t - c[0] * v[0];
    t = t - c[1] * v[1];
    t = t - c[2] * v[2];
    t = t - c[4] * v[3];
    t = t - c[5] * v[4];
    t = t - c[6] * v[5];
    return t / c[3];
}

// Half-sweep of one colour on level A, in place.  init: the first half from x = 0 -- x = b / d on the colour, 0 on
// the other (b - 0 terms == b).  Bytes per row (fine level, dictionary form): b 8 (the other colour's entries share
// its lines) + x 8 read (neighbours from L2 / L1) + x 8 written + 1 class byte = 25 B; init: b 8 + x 8 written + 1 = 17 B.
template <bool DICT>
__global__ __launch_bounds__(256) void k_mg_smooth(MgOp A, Gate g, int colour, int init, double *__restrict__ x,
                                                   const double *__restrict__ b)
{
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const Pos p = pos_of(A, r);
    const bool mine = ((p.i + p.j + p.k) & 1) == colour;
    if (!mine) {
        if (init) x[r] = 0.0;
        return;
    }
    double c[7];
    row_coefs<DICT>(A, tbl, r, c);
    if (init) {
        x[r] = b[r] / c[3];
        return;
    }
    double v[6];
    neighbours(A, p, r, [&](int64_t q) { return x[q]; }, v);
    x[r] = gs_value(c, v, b[r]);
}

// Residual + restriction: bc[coarse cell] = (sum of its children's b - A w, k outermost, i innermost, from 0) * 1/children.
// One thread per coarse cell; the fine residual never reaches HBM.  Bytes per FINE row: w 8 + b 8 + 1 class byte read,
// 8 / children written = 18 B at factor 2 along every axis.
template <bool DICT>
__global__ __launch_bounds__(256) void k_mg_restrict(MgOp A, MgOp C, int fx, int fy, int fz, Gate g,
                                                     const double *__restrict__ w, const double *__restrict__ b,
                                                     double *__restrict__ bc)
{
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    const int64_t rc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rc >= C.n) return;
    const Pos pc = pos_of(C, rc);
    double s = 0.0;
    for (int dk = 0; dk < fz; ++dk)
        for (int dj = 0; dj < fy; ++dj)
            for (int di = 0; di < fx; ++di) {
                const Pos p{pc.i * fx + di, pc.j * fy + dj, pc.k * fz + dk};
                const int64_t r = (int64_t)p.k * A.kdz + (int64_t)p.j * A.sdx + p.i;
                double c[7], v[6];
                row_coefs<DICT>(A, tbl, r, c);
                neighbours(A, p, r, [&](int64_t q) { return w[q]; }, v);
                double t = b[r];
                t = t - c[0] * v[0];
                t = t - c[1] * v[1];
                t = t - c[2] * v[2];
                t = t - c[3] * w[r];
                t = t - c[4] * v[3];
                t = t - c[5] * v[4];
                t = t - c[6] * v[5];
                s = s + t;
            }
    bc[rc] = s * (1.0 / (double)(fx * fy * fz));
}

// Prolongation (piecewise-constant injection) + correction fused with the first post-smoothing half-sweep (black):
// red rows x = w + xc[parent]; black rows the GS value from the corrected red neighbours.  Bytes per fine row: w 8 +
// b 8 (black rows; the lines hold both colours) + 1 class byte read, x 8 written, xc from the L2 = 25 B.
template <bool DICT>
__global__ __launch_bounds__(256) void k_mg_prolong(MgOp A, MgOp C, int fx, int fy, int fz, Gate g,
                                                    const double *__restrict__ w, const double *__restrict__ xc,
                                                    const double *__restrict__ b, double *__restrict__ x)
{
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const Pos p = pos_of(A, r);
    const auto corrected = [&](int64_t q) {
        const Pos pq = pos_of(A, q);
        const int64_t par = (int64_t)(pq.k / fz) * C.kdz + (int64_t)(pq.j / fy) * C.sdx + pq.i / fx;
        return w[q] + xc[par];
    };
    if (((p.i + p.j + p.k) & 1) == 0) {
        x[r] = corrected(r);
        return;
    }
    double c[7], v[6];
    row_coefs<DICT>(A, tbl, r, c);
    neighbours(A, p, r, corrected, v);
    x[r] = gs_value(c, v, b[r]);
}

// Coarsest level: `sweeps` sweeps of (red, black, black, red) from x = 0 by one workgroup, x in LDS, b and the class of
// a thread's (at most four) rows in registers.  A fixed linear operator of b, so BiCGSTAB stays valid.
template <bool DICT>
__global__ __launch_bounds__(EC3D_MG_COARSE_THREADS) void k_mg_coarse(MgOp A, Gate g, int sweeps,
                                                                      const double *__restrict__ b,
                                                                      double *__restrict__ x)
{
    constexpr int RPT = EC3D_MG_COARSE_ROWS / EC3D_MG_COARSE_THREADS;
    __shared__ double xs[EC3D_MG_COARSE_ROWS];
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    double br[RPT];
    Pos pr[RPT];
    int colr[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int64_t r = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
        colr[q] = -1;
        if (r < A.n) {
            pr[q] = pos_of(A, r);
            colr[q] = (pr[q].i + pr[q].j + pr[q].k) & 1;
            br[q] = b[r];
            xs[r] = 0.0;
        }
    }
    __syncthreads();
    for (int s = 0; s < sweeps; ++s)
        for (int h = 0; h < 4; ++h) {
            const int colour = (h == 0 || h == 3) ? 0 : 1;
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                if (colr[q] != colour) continue;
                const int64_t r = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
                double c[7], v[6];
                row_coefs<DICT>(A, tbl, r, c);
                neighbours(A, pr[q], r, [&](int64_t t) { return xs[t]; }, v);
                xs[r] = gs_value(c, v, br[q]);
            }
            __syncthreads();
        }
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int64_t r = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
        if (r < A.n) x[r] = xs[r];
    }
}

// ---- outer iteration ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double *lds)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wid] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < (int)(blockDim.x >> 6); ++q) s += lds[q];
    return s; // valid in thread 0
}

// y = A x (rows summed in offset order from the -z term); partials of a.y (slot 0) and, with two, y.y (slot 1).
// Bytes per row: x 8 + a 8 + 1 class byte read, y 8 written = 25 B.
template <bool DICT>
__global__ __launch_bounds__(256) void k_mg_spmv_dot(MgOp A, Gate g, const double *__restrict__ x,
                                                     const double *__restrict__ a, double *__restrict__ y, int two,
                                                     double *__restrict__ part)
{
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    __shared__ double lds[8];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    double d0 = 0.0, d1 = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.n; r += (int64_t)gridDim.x * blockDim.x) {
        const Pos p = pos_of(A, r);
        double c[7], v[6];
        row_coefs<DICT>(A, tbl, r, c);
        neighbours(A, p, r, [&](int64_t q) { return x[q]; }, v);
        double s = c[0] * v[0];
        s = s + c[1] * v[1];
        s = s + c[2] * v[2];
        s = s + c[3] * x[r];
        s = s + c[4] * v[3];
        s = s + c[5] * v[4];
        s = s + c[6] * v[5];
        y[r] = s;
        d0 = d0 + a[r] * s;
        d1 = d1 + s * s;
    }
    d0 = block_sum(d0, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = d0;
    if (two) {
        d1 = block_sum(d1, lds);
        if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = d1;
    }
}

// s = r - alpha v; partial s.s.  Bytes per row: 16 read, 8 written.
__global__ __launch_bounds__(256) void k_mg_s(int64_t n, Gate g, const SolverState *st, const double *__restrict__ r,
                                              const double *__restrict__ v, double *__restrict__ s,
                                              double *__restrict__ part)
{
    __shared__ double lds[8];
    if (gated_off(g)) return;
    const double alpha = st->alpha;
    double d = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const double sv = r[q] - alpha * v[q];
        s[q] = sv;
        d = d + sv * sv;
    }
    d = block_sum(d, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = d;
}

// x = x + alpha p^ + omega s^;  r = s - omega t;  partials r.r, r.r0.  After the ||S|| exit of this iteration only
// x = x + alpha p^ (src/solvers.f90:34-37).  Bytes per row: x, p^, s^, s, t, r0 read 48, x, r written 16 = 64 B.
__global__ __launch_bounds__(256) void k_mg_xr(int64_t n, int it, const SolverState *st, double *__restrict__ x,
                                               const double *__restrict__ ph, const double *__restrict__ sh,
                                               const double *__restrict__ s, const double *__restrict__ t,
                                               const double *__restrict__ r0, double *__restrict__ r,
                                               double *__restrict__ part)
{
    __shared__ double lds[8];
    const int stop = st->stop_iter;
    if (stop < it) return;
    const double alpha = st->alpha, omega = st->omega;
    const bool s_exit = stop == it;
    double d0 = 0.0, d1 = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        if (s_exit) {
            x[q] = x[q] + alpha * ph[q];
            continue;
        }
        x[q] = x[q] + alpha * ph[q] + omega * sh[q];
        const double rv = s[q] - omega * t[q];
        r[q] = rv;
        d0 = d0 + rv * rv;
        d1 = d1 + rv * r0[q];
    }
    if (s_exit) return;
    d0 = block_sum(d0, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = d0;
    d1 = block_sum(d1, lds);
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
    __shared__ double lds[8];
    if (gated_off(g)) return;
    const int nslot = (stage == MG_OMEGA || stage == MG_REXIT) ? 2 : 1;
    double v[2] = {0.0, 0.0};
    for (int sl = 0; sl < nslot; ++sl) {
        double a = 0.0;
        for (int q = threadIdx.x; q < nparts; q += blockDim.x) a += part[(int64_t)sl * nparts + q];
        v[sl] = block_sum(a, lds);
    }
    if (threadIdx.x != 0) return;
    const int it = g.it;
    const int64_t h = (int64_t)(it - 1) * 2;
    switch (stage) {
    case MG_ALPHA: st->alpha = st->rr0[it & 1] / v[0]; break; // (:31-32)
    case MG_SEXIT: {
        const double sn = sqrt(v[0]);
        if (it - 1 < hist_cap) hist[h] = sn;
        if (sn / st->bnorm < st->tol) mg_stop_publish(st, it, 1); // (:34-38)
        break;
    }
    case MG_OMEGA: st->omega = v[0] / v[1]; break; // (:40)
    case MG_REXIT: {
        const double rn = sqrt(v[0]), rr0_new = v[1];
        if (it - 1 < hist_cap) hist[h + 1] = rn;
        st->rnorm = rn;
        if (rn / st->bnorm < st->tol) { // (:43)
            mg_stop_publish(st, it, 2);
            break;
        }
        ms->beta = (st->alpha / st->omega) * rr0_new / st->rr0[it & 1]; // (:45)
        const bool restart = fabs(rr0_new) / st->bnorm < st->tol;   // (:47-49)
        ms->restart = restart;
        if (restart) st->restarts = st->restarts + 1;
        st->rr0[(it + 1) & 1] = restart ? v[0] : rr0_new; // R0 = R: the next rr0 is R.R
        break;
    }
    }
}

inline unsigned blocks_of(int64_t n, int t = 256) { return (unsigned)((n + t - 1) / t); }
inline unsigned dot_blocks(int64_t n) { return (unsigned)std::min<int64_t>(EC3D_MG_DOT_BLOCKS, std::max<int64_t>(1, blocks_of(n))); }

MgOp op_of(const DevMatrix &A, int sdx, int sdy, int sdz)
{
    MgOp o;
    o.sdx = sdx; o.sdy = sdy; o.sdz = sdz;
    o.n = A.n;
    o.n_pad = A.n_pad;
    o.kdz = (int64_t)sdx * sdy;
    o.cls = A.ncls > 0 ? A.cls : nullptr;
    o.table = A.table;
    o.ncls = A.ncls;
    o.bands = A.ncls > 0 ? nullptr : A.bands;
    return o;
}

#define MG_LAUNCH(kern, grid, block, ...)                                                                          \
    do {                                                                                                           \
        if (dict) kern<true><<<(grid), (block), 0, s>>>(__VA_ARGS__);                                             \
        else kern<false><<<(grid), (block), 0, s>>>(__VA_ARGS__);                                                 \
    } while (0)

// one V-cycle z = M r (enqueued)
void launch_vcycle(ec3d_mg *m, Gate g, const double *r, double *z, hipStream_t s)
{
    const int L = (int)m->lev.size();
    for (int l = 0; l + 1 < L; ++l) {
        MgLevel &F = m->lev[(size_t)l];
        const MgOp &A = F.op;
        const bool dict = A.cls != nullptr;
        const double *B = l == 0 ? r : F.b;
        double *W = l == 0 ? m->w0 : F.w;
        for (int sw = 0; sw < m->pre; ++sw) {
            MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, 0, sw == 0, W, B);
            MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, 1, 0, W, B);
        }
        const MgLevel &C = m->lev[(size_t)l + 1];
        MG_LAUNCH(k_mg_restrict, blocks_of(C.op.n), 256, A, C.op, F.f[0], F.f[1], F.f[2], g, W, B, C.b);
    }
    {
        MgLevel &K = m->lev[(size_t)L - 1];
        const bool dict = K.op.cls != nullptr;
        MG_LAUNCH(k_mg_coarse, 1, EC3D_MG_COARSE_THREADS, K.op, g, m->coarse, L == 1 ? r : K.b, L == 1 ? z : K.x);
    }
    for (int l = L - 2; l >= 0; --l) {
        MgLevel &F = m->lev[(size_t)l];
        const MgOp &A = F.op;
        const bool dict = A.cls != nullptr;
        const double *B = l == 0 ? r : F.b;
        double *W = l == 0 ? m->w0 : F.w;
        double *X = l == 0 ? z : F.x;
        const MgLevel &C = m->lev[(size_t)l + 1];
        MG_LAUNCH(k_mg_prolong, blocks_of(A.n), 256, A, C.op, F.f[0], F.f[1], F.f[2], g, W, C.x, B, X);
        MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, 0, 0, X, B);
        for (int sw = 1; sw < m->post; ++sw) {
            MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, 1, 0, X, B);
            MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, 0, 0, X, B);
        }
    }
}

void free_level_matrix(DevMatrix &A)
{
    if (A.bands) (void)hipFree(A.bands);
    if (A.tail_id) (void)hipFree(A.tail_id);
    if (A.tile_flag) (void)hipFree(A.tile_flag);
    if (A.chunk_ptr) (void)hipFree(A.chunk_ptr);
    if (A.tcol) (void)hipFree(A.tcol);
    if (A.tval) (void)hipFree(A.tval);
    if (A.cls) (void)hipFree(A.cls);
    if (A.table) (void)hipFree(A.table);
    A = DevMatrix();
}

void free_mg(ec3d_mg *m)
{
    if (!m) return;
    for (size_t l = 1; l < m->lev.size(); ++l) free_level_matrix(m->lev[l].A);
    if (m->vec_base) (void)hipFree(m->vec_base);
    if (m->part) (void)hipFree(m->part);
    if (m->scal) (void)hipFree(m->scal);
    delete m;
}

} // namespace

// ---- hierarchy rule (host) --------------------------------------------------------------------------------------------
// Level dims: an axis halves while it is even and >= 8; stop when no axis can halve or a level has <= 4096 rows.
// Returns false when the coarsest level is over the coarse solver's cap.
static bool mg_dims(int sdx, int sdy, int sdz, std::vector<std::array<int, 3>> &dims)
{
    dims.assign(1, {sdx, sdy, sdz});
    for (;;) {
        const auto d = dims.back();
        if ((int64_t)d[0] * d[1] * d[2] <= EC3D_MG_COARSE_ROWS) return true;
        std::array<int, 3> e = d;
        bool any = false;
        for (int a = 0; a < 3; ++a)
            if (d[a] % 2 == 0 && d[a] >= 8) {
                e[a] = d[a] / 2;
                any = true;
            }
        if (!any) return false;
        dims.push_back(e);
    }
}

void ec3d_mg_free(ec3d_ctx *c)
{
    free_mg(c->mg);
    c->mg = nullptr;
}

extern "C" int ec3d_set_preconditioner(ec3d_handle c, int kind, int32_t pre, int32_t post, int32_t coarse_sweeps)
{
    if (!c) {
        ec3d_set_error("ec3d_set_preconditioner: null handle");
        return 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    if (kind == EC3D_PRECOND_NONE) {
        EC3D_HIP(hipStreamSynchronize(c->stream));
        ec3d_mg_free(c);
        return 0;
    }
    if (kind != EC3D_PRECOND_MG || pre < 0 || post < 0 || coarse_sweeps < 0) {
        ec3d_set_error("ec3d_set_preconditioner: unknown kind or negative sweep count");
        return 2;
    }
    int rc = ec3d_need_matrix(c, "ec3d_set_preconditioner");
    if (rc) return rc;
    if (!c->poisson_full || c->in_multi || c->halo > 0 || c->nranks > 1 || c->dist) {
        ec3d_set_error("ec3d_set_preconditioner: the multigrid preconditioner needs a matrix from ec3d_assemble_poisson "
                       "on a handle of its own (not A-V, CSR, a slab or a handle of ec3d_multi)");
        return EC3D_PRECOND_E_MATRIX;
    }
    std::vector<std::array<int, 3>> dims;
    if (!mg_dims(c->sdx, c->sdy, c->sdz, dims)) {
        const auto d = dims.back();
        ec3d_set_error("ec3d_set_preconditioner: no axis of the " + std::to_string(d[0]) + "x" + std::to_string(d[1]) +
                       "x" + std::to_string(d[2]) + " level halves (even and >= 8) and it has more than " +
                       std::to_string(EC3D_MG_COARSE_ROWS) + " rows, the coarse solver's cap");
        return EC3D_PRECOND_E_COARSE;
    }
    if (c->A.ncls > EC3D_MG_MAXCLS) {
        ec3d_set_error("ec3d_set_preconditioner: more dictionary classes than the smoother's table holds");
        return EC3D_PRECOND_E_MATRIX;
    }
    // build the new hierarchy completely before the old one is replaced: a failure leaves the handle as it was
    ec3d_mg *m = new ec3d_mg;
    m->pre = pre ? pre : 2;
    m->post = post ? post : 2;
    m->coarse = coarse_sweeps ? coarse_sweeps : 16;
    const int L = (int)dims.size();
    m->lev.resize((size_t)L);
    const auto fail = [&](int code) {
        free_mg(m);
        return code;
    };
    m->lev[0].op = op_of(c->A, c->sdx, c->sdy, c->sdz);
    for (int a = 0; a < 3; ++a) m->lev[0].delta[a] = c->poisson_delta[a];
    int64_t coarse_len = 0;
    for (int l = 1; l < L; ++l) {
        MgLevel &P = m->lev[(size_t)l - 1], &Q = m->lev[(size_t)l];
        for (int a = 0; a < 3; ++a) {
            P.f[a] = dims[(size_t)l - 1][a] / dims[(size_t)l][a];
            Q.delta[a] = P.delta[a] * P.f[a];
        }
        rc = ec3d_assemble_poisson_level(c, Q.A, dims[(size_t)l][0], dims[(size_t)l][1], dims[(size_t)l][2],
                                         c->poisson_bnd, Q.delta);
        if (rc) return fail(rc);
        Q.op = op_of(Q.A, dims[(size_t)l][0], dims[(size_t)l][1], dims[(size_t)l][2]);
        coarse_len += 3 * ((Q.op.n + 63) / 64 * 64);
    }
    const int64_t nf = (c->A.n + 63) / 64 * 64;
    const int64_t total = coarse_len + 3 * nf;
    if (hipMalloc(&m->vec_base, (size_t)total * sizeof(double)) != hipSuccess ||
        hipMalloc(&m->part, 2 * EC3D_MG_DOT_BLOCKS * sizeof(double)) != hipSuccess ||
        hipMalloc(&m->scal, sizeof(MgScalars)) != hipSuccess) {
        (void)hipGetLastError();
        ec3d_set_error("ec3d_set_preconditioner: out of device memory for the hierarchy");
        return fail(100);
    }
    if (hipMemsetAsync(m->vec_base, 0, (size_t)total * sizeof(double), c->stream) != hipSuccess ||
        hipMemsetAsync(m->scal, 0, sizeof(MgScalars), c->stream) != hipSuccess) {
        ec3d_set_error("ec3d_set_preconditioner: hipMemsetAsync failed");
        return fail(100);
    }
    double *q = m->vec_base;
    for (int l = 1; l < L; ++l) {
        MgLevel &Q = m->lev[(size_t)l];
        const int64_t len = (Q.op.n + 63) / 64 * 64;
        Q.x = q; Q.w = q + len; Q.b = q + 2 * len;
        q += 3 * len;
    }
    m->w0 = q; m->ph = q + nf; m->sh = q + 2 * nf;
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        ec3d_set_error("ec3d_set_preconditioner: building the hierarchy failed");
        return fail(100);
    }
    ec3d_mg_free(c);
    c->mg = m;
    return 0;
}

extern "C" int ec3d_get_preconditioner(ec3d_handle c, int *kind, int32_t *levels, int32_t *dims)
{
    if (!c) {
        ec3d_set_error("ec3d_get_preconditioner: null handle");
        return 2;
    }
    const ec3d_mg *m = c->mg;
    if (kind) *kind = m ? EC3D_PRECOND_MG : EC3D_PRECOND_NONE;
    if (levels) *levels = m ? (int32_t)m->lev.size() : 0;
    if (dims && m)
        for (size_t l = 0; l < m->lev.size(); ++l) {
            dims[3 * l] = m->lev[l].op.sdx;
            dims[3 * l + 1] = m->lev[l].op.sdy;
            dims[3 * l + 2] = m->lev[l].op.sdz;
        }
    return 0;
}

extern "C" int ec3d_precond_apply(ec3d_handle c, const double *r, double *z)
{
    int rc = ec3d_need_matrix(c, "ec3d_precond_apply");
    if (rc) return rc;
    if (!c->mg) {
        ec3d_set_error("ec3d_precond_apply: no preconditioner set (ec3d_set_preconditioner)");
        return 3;
    }
    ec3d_mg *m = c->mg;
    if ((rc = ec3d_vec_h2d(c, m->ph, r))) return rc;
    launch_vcycle(m, Gate{nullptr, 0, 0}, m->ph, m->sh, c->stream);
    EC3D_HIP(hipGetLastError());
    if ((rc = ec3d_vec_d2h(c, z, m->sh))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// iterations per poll of solve_core: about 1 ms of device work (a V-cycle is ~210 B per fine row, two per iteration)
int ec3d_mg_chunk(const ec3d_ctx *c)
{
    const double est_us = (double)c->A.n_pad * 600.0 / 4.0e6 + 60.0 * (double)c->mg->lev.size();
    return (int)std::min<double>(16.0, std::max<double>(1.0, 1000.0 / est_us));
}

// One iteration of the right-preconditioned BiCGSTAB with restart (src/solvers.f90:24-50 with P, S replaced by their
// preconditioned images in the products with A and the X update):
//   p^ = M p; v = A p^; alpha = rho / (r0.v); s = r - alpha v; [exit on ||s|| / ||b||: x += alpha p^]
//   s^ = M s; t = A s^; omega = (t.s)/(t.t); x += alpha p^ + omega s^; r = s - omega t; [exit on ||r|| / ||b||]
//   beta = (alpha / omega) (r.r0) / rho; p = r + beta (p - omega v); restart as the reference.
// The work vectors: v in AP, t in AS.  Sums and exits stay on the device; launches past an exit are no-ops.
void ec3d_mg_launch_iteration(ec3d_ctx *c, int it)
{
    ec3d_mg *m = c->mg;
    double **v = c->vec;
    hipStream_t s = c->stream;
    const MgOp &A = m->lev[0].op;
    const bool dict = A.cls != nullptr;
    const int64_t n = A.n;
    const unsigned nb = dot_blocks(n);
    const Gate g0{c->state, it, 0}, g1{c->state, it, 1};
    launch_vcycle(m, g0, v[EC3D_VEC_P], m->ph, s);
    MG_LAUNCH(k_mg_spmv_dot, nb, 256, A, g0, m->ph, v[EC3D_VEC_R0], v[EC3D_VEC_AP], 0, m->part);
    k_mg_scalar<<<1, 256, 0, s>>>(MG_ALPHA, g0, c->state, m->scal, m->part, (int)nb, c->hist, c->hist_cap);
    k_mg_s<<<nb, 256, 0, s>>>(n, g0, c->state, v[EC3D_VEC_R], v[EC3D_VEC_AP], v[EC3D_VEC_S], m->part);
    k_mg_scalar<<<1, 256, 0, s>>>(MG_SEXIT, g0, c->state, m->scal, m->part, (int)nb, c->hist, c->hist_cap);
    launch_vcycle(m, g1, v[EC3D_VEC_S], m->sh, s);
    MG_LAUNCH(k_mg_spmv_dot, nb, 256, A, g1, m->sh, v[EC3D_VEC_S], v[EC3D_VEC_AS], 1, m->part);
    k_mg_scalar<<<1, 256, 0, s>>>(MG_OMEGA, g1, c->state, m->scal, m->part, (int)nb, c->hist, c->hist_cap);
    k_mg_xr<<<nb, 256, 0, s>>>(n, it, c->state, v[EC3D_VEC_X], m->ph, m->sh, v[EC3D_VEC_S], v[EC3D_VEC_AS],
                               v[EC3D_VEC_R0], v[EC3D_VEC_R], m->part);
    k_mg_scalar<<<1, 256, 0, s>>>(MG_REXIT, g1, c->state, m->scal, m->part, (int)nb, c->hist, c->hist_cap);
    k_mg_p<<<nb, 256, 0, s>>>(n, g1, c->state, m->scal, v[EC3D_VEC_R], v[EC3D_VEC_AP], v[EC3D_VEC_P], v[EC3D_VEC_R0]);
}
