// ec3d_mg.hip — geometric multigrid preconditioner of the single-component operator (ec3d_assemble_poisson), the block
// multigrid of the structured A-V form, and what each hands to the outer iteration of ec3d_outer.hip: its cycle and its
// operator (ec3d_set_preconditioner; DESIGN.md sections 9, 10).
//
// Hierarchy: level 0 is the handle's own matrix; every coarser level is the same device assembly
// (ec3d_assemble_poisson_level) at half the cells and twice the spacing on each axis that is even and >= 8, with the
// same BND -- a rediscretisation, not a Galerkin product.  Coarsening stops when no axis can halve or a level has at
// most EC3D_MG_COARSE_ROWS rows; that level is solved by one single-workgroup launch in LDS.
// With EC3D_COARSEN_AGGREGATE (ec3d_set_precond_coarsening; the rule is ec3d_mg_plan.hpp's) every axis of extent > 1 is
// ceil-halved instead, so every box gets a hierarchy: levels stay rediscretisations while every axis is even and >= 8,
// and from the first level that is not, every coarser level is the Galerkin product of piecewise-constant aggregation
// (k_mg_galerkin, fp64, once at set-up), kept as seven band streams; the restriction is then the mean over the
// aggregate's actual children (an odd axis ends in an aggregate of one cell).  tests/mg_numpy_agg.py restates it.
//
// A 7-point matrix from ec3d_set_matrix_csr whose box the caller named (ec3d_set_precond_grid) gets the same cycle: the
// matrix is checked on the device (k_mg_check_grid: no tail, the box's offsets only, zero wrap slots, a nonzero finite
// diagonal), level 0 is the handle's dictionary form itself when it has the seven offsets and at most EC3D_MG_MAXCLS
// classes, else one gathered copy of seven band streams the hierarchy owns (k_mg_gather; 56 B per row on top of the
// handle's matrix: variable coefficients with many classes, fewer than seven bands, ec3d_set_format(h, 0)), and every
// coarse level is a Galerkin product over ceil-halved dims (ec3d_mg_plan_matrix).  tests/mg_numpy_csr.py restates it.
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
// EC3D_PRECOND_FP32 (ec3d_set_precond_precision): the same cycle with every level's coefficients narrowed once at set-up,
// the right-hand side narrowed once per application and every vector and operation of the cycle in fp32 -- the kernels
// above instantiated with T = float; p^ and s^ are then fp32 vectors the outer kernels widen on load, and the outer
// iteration stays fp64 (tests/mg_numpy_f32.py restates it).
//
// EC3D_PRECOND_BLOCK_MG (the structured A-V form): its kernels (k_avmg_*) are below, behind the
// single-component ones.  N of ec3d_set_null_precond (section 16a) is the same hierarchy on the transposed blocks, a
// BlockMg of the null set-up's own; ec3d_adjoint_iteration runs the outer iteration around it, or around M = I.
//
// Host side: a handle's ec3d_mg owns one hierarchy (PoissonMg<double>, PoissonMg<float> or BlockMg), built completely
// before it replaces the old one; launch_schedule is the cycle's order of launches for all three.
//
// A row of a level is read from the level's own device format: class byte + coefficient table in LDS (dictionary form,
// what every coarse level uses) or the seven band streams (ec3d_set_format(h, 0)).  Bands in offset order
// (-z, -y, -x, diag, +x, +y, +z); a neighbour beyond the box contributes nothing (its coefficient is 0 there anyway).
#include "../../include/ec3d_hip.h"
#include "ec3d_avmg_plan.hpp"
#include "ec3d_mg_plan.hpp"
#include "ec3d_outer.hpp"

#include <array>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <variant>

#define EC3D_MG_COARSE_ROWS 4096 // x of the coarsest level in LDS (32 KiB), b and class bytes in registers
#define EC3D_MG_COARSE_THREADS 1024
#define EC3D_MG_MAXCLS 32        // dictionary classes a level may have (the single-component operator has 28)

// T: the precision of the level's coefficients and vectors (double; float for the fp32 V-cycle, EC3D_PRECOND_FP32)
template <class T> struct MgOpT {
    int sdx, sdy, sdz;
    int64_t n, n_pad, kdz;
    const uint8_t *cls;   // dictionary form: coefficient q of row r = table[cls[r] * 7 + q]
    const T *table;
    int ncls;
    const T *bands;       // band form (cls == nullptr): bands[q * n_pad + r]
};
using MgOp = MgOpT<double>;
using MgOp32 = MgOpT<float>;

// A level of the block multigrid of the structured A-V form (EC3D_PRECOND_BLOCK_MG).  One operator serves the three
// A blocks, whose vectors lie vs doubles apart.  Level 0 reads block 0's class bytes of the handle's matrix, with the
// plane pitch of the structured form (kdz) and its zero-class padding rows; coarse levels are 7 plain band streams.
struct AvOp {
    int sdx, sdy, sdz;
    int64_t kdz;          // rows between two planes
    int64_t n;            // rows of one block (level 0: planes * pitch, padding rows included)
    int64_t vs;           // doubles between the three blocks' vectors
    const uint8_t *cls;   // class form: coefficient q of row r = table[cls[r] * 16 + q], q < 7, for classes in
    const double *table;  //   [cls0, cls0 + ncls); any other class is a row without coefficients
    int cls0, ncls;
    const double *bands;  // band form (cls == nullptr): bands[q * n_pad + r]
    int64_t n_pad;
};

struct AvLevel {
    AvOp op;
    int f[3] = {1, 1, 1};     // aggregate width towards the next level per axis (1 or 2)
    DevBuf<double> bands;     // coarse levels
    double *x = nullptr, *w = nullptr, *b = nullptr; // coarse levels: inside BlockMg::vec, 3 blocks each
};

// ---- the hierarchies: a handle's ec3d_mg holds exactly one of PoissonMg<double>, PoissonMg<float>, BlockMg ---------------

// A level of the hierarchy of the single-component operator (EC3D_PRECOND_MG): what does not depend on the cycle's precision
struct MgGrid {
    int kind = EC3D_MG_LEVEL_MATRIX; // how the level's operator is made (ec3d_mg_plan.hpp)
    DevMatrix A;          // a rediscretised level's assembled matrix (level 0: unused, the handle's own)
    DevBuf<double> bands; // a Galerkin level's seven band streams (released once an fp32 hierarchy has narrowed them)
    int f[3] = {1, 1, 1}; // coarsening factor towards the next level per axis (1 or 2)
    double delta[3] = {0, 0, 0};
};
// ... and what does (the kernels' T is deduced from these)
template <class T> struct MgLevelT {
    MgOpT<T> op{};        // double: the level's own device format; float: its class bytes and the narrowed coefficients
    T *x = nullptr, *w = nullptr, *b = nullptr; // coarse levels: inside PoissonMg::vec
};
// float: every level's coefficients narrowed once at set-up -- the class table, or the seven band streams of level 0
// under ec3d_set_format(h, 0) and of a Galerkin level (rediscretised levels are always in dictionary form)
template <class T> struct MgNarrowed {};
template <> struct MgNarrowed<float> {
    std::vector<DevBuf<float>> coef;
};
// T: the precision of every vector and operation of the cycle.  float (EC3D_PRECOND_FP32): there is no fp64 vector, and
// of the fp64 operators only op0 is read.
template <class T> struct PoissonMg : MgNarrowed<T> {
    std::vector<MgGrid> grid;
    MgOp op0{};           // level 0 in fp64, from the handle's matrix: what the outer SpMV + dot launch reads
    DevBuf<double> bands0; // a CSR matrix that is no direct view: level 0's gathered band streams, which op0 points to
                           // (kept by an fp32 hierarchy too: the outer SpMV + dot reads them)
    std::vector<MgLevelT<T>> lev;
    DevBuf<T> vec;        // coarse x, w, b per level, then the fine w, [b0,] p^, s^
    T *w0 = nullptr, *ph = nullptr, *sh = nullptr;
    T *b0 = nullptr;      // float: the fine right-hand side narrowed; double: null, the cycle reads r itself
};

// The block hierarchy of the structured A-V form (EC3D_PRECOND_BLOCK_MG): one hierarchy for the three A blocks, and the
// U block's rows with the projection of their right-hand side onto the U block's range (ec3d_avmg_plan.hpp)
struct BlockMg {
    std::vector<AvLevel> lev;
    AvOp uop{};                 // the U block's rows (class form, no hierarchy)
    DevBuf<double> vec;         // coarse x, w, b per level, then the fine w (3 blocks each), p^, s^ with their halos
    double *w0 = nullptr, *ph = nullptr, *sh = nullptr;
    DevBuf<int32_t> ulist;      // AvmgPlan's ured, then ublack
    int64_t nu_red = 0, nu_black = 0;
    DevBuf<int32_t> uidx;       // AvmgPlan's ucomp, plist, chunks, cco
    const int32_t *ucomp = nullptr, *plist = nullptr, *chunks = nullptr, *cco = nullptr;
    DevBuf<double> ubuf;        // AvmgPlan's pw, inv_w, then umean (one per component) and upart (one per chunk)
    double *pw = nullptr, *inv_w = nullptr, *umean = nullptr, *upart = nullptr;
    int ncomp = 0, nchunk = 0;
    // N of the null projection's adjoint solves (ec3d_set_null_precond)
    bool adjoint = false;       // the U sweeps run on U^T between two plain-mean projections (pw = 1, inv_w = 1 / cells)
    DevBuf<double> bands0;      // EC3D_NULL_PRECOND_BLOCK_MG: the transposed A block gathered once, level 0's band streams
};

// What ec3d_ctx::mg points to: the settings and the outer iteration's scratch, which every kind has, and the hierarchy
struct ec3d_mg {
    int kind = EC3D_PRECOND_MG;
    int precision = EC3D_PRECOND_FP64; // EC3D_PRECOND_FP32: kind EC3D_PRECOND_MG only
    int coarsening = EC3D_COARSEN_REDISCRETIZE; // the rule the hierarchy was built by (EC3D_PRECOND_BLOCK_MG: aggregate)
    int pre = 2, post = 2, coarse = 16;
    DevBuf<double> part;        // 2 * EC3D_MG_DOT_BLOCKS
    DevBuf<MgScalars> scal;
    std::variant<PoissonMg<double>, PoissonMg<float>, BlockMg> h;
};

namespace {

template <class T> __device__ __forceinline__ void load_table(const MgOpT<T> &A, T *tbl)
{
    if (!A.cls) return;
    for (int q = threadIdx.x; q < A.ncls * 7; q += blockDim.x) tbl[q] = A.table[q];
    __syncthreads();
}
template <bool DICT, class T>
__device__ __forceinline__ void row_coefs(const MgOpT<T> &A, const T *tbl, int64_t r, T (&c)[7])
{
    if constexpr (DICT) {
        const T *t = tbl + 7 * (int)A.cls[r];
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
template <class OP> __device__ __forceinline__ Pos pos_of(const OP &A, int64_t r)
{
    const unsigned ur = (unsigned)r, sx = (unsigned)A.sdx;
    const unsigned ij = ur % (unsigned)A.kdz;
    return Pos{(int)(ij % sx), (int)(ij / sx), (int)(ur / (unsigned)A.kdz)};
}
// x at the six neighbours in offset order (-z, -y, -x, +x, +y, +z); 0 beyond the box
template <class OP, class LD, class T>
__device__ __forceinline__ void neighbours(const OP &A, const Pos &p, int64_t r, LD ld, T (&v)[6])
{
    v[0] = p.k > 0 ? ld(r - A.kdz) : T(0);
    v[1] = p.j > 0 ? ld(r - A.sdx) : T(0);
    v[2] = p.i > 0 ? ld(r - 1) : T(0);
    v[3] = p.i + 1 < A.sdx ? ld(r + 1) : T(0);
    v[4] = p.j + 1 < A.sdy ? ld(r + A.sdx) : T(0);
    v[5] = p.k + 1 < A.sdz ? ld(r + A.kdz) : T(0);
}
// Gauss-Seidel value of a row: (b - sum of the off-diagonal terms in offset order) / d
template <class T> __device__ __forceinline__ T gs_value(const T (&c)[7], const T (&v)[6], T b)
{
    T t = b;
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
// With T = float (13 B, init 9 B on a coarse level): the same operations in fp32.
template <bool DICT, class T = double>
__global__ __launch_bounds__(256) void k_mg_smooth(MgOpT<T> A, Gate g, int colour, int init, T *__restrict__ x,
                                                   const T *__restrict__ b)
{
    __shared__ T tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const Pos p = pos_of(A, r);
    const bool mine = ((p.i + p.j + p.k) & 1) == colour;
    if (!mine) {
        if (init) x[r] = T(0);
        return;
    }
    T c[7];
    row_coefs<DICT>(A, tbl, r, c);
    if (init) {
        x[r] = b[r] / c[3];
        return;
    }
    T v[6];
    neighbours(A, p, r, [&](int64_t q) { return x[q]; }, v);
    x[r] = gs_value(c, v, b[r]);
}

// The init half-sweep (red) of the fp32 cycle's fine level: it visits every row anyway, so it narrows the fp64
// right-hand side once (round to nearest) into bf, which every later launch of the application reads, and sets
// x = bf / d on red, 0 on black.  Bytes per row: b 8 + 1 class byte read, bf 4 + x 4 written = 17 B.
template <bool DICT>
__global__ __launch_bounds__(256) void k_mg_init_f32(MgOp32 A, Gate g, const double *__restrict__ b,
                                                     float *__restrict__ bf, float *__restrict__ x)
{
    __shared__ float tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const float bv = (float)b[r];
    bf[r] = bv;
    const Pos p = pos_of(A, r);
    if ((p.i + p.j + p.k) & 1) {
        x[r] = 0.0f;
        return;
    }
    float c[7];
    row_coefs<DICT>(A, tbl, r, c);
    x[r] = bv / c[3];
}

// Residual + restriction: bc[coarse cell] = (sum of its children's b - A w, k outermost, i innermost, from 0) * 1/children.
// One thread per coarse cell; the fine residual never reaches HBM.  Bytes per FINE row: w 8 + b 8 + 1 class byte read,
// 8 / children written = 18 B at factor 2 along every axis.
// T = float: about 9.5 B (1 / children is a power of two, exact in either precision).
// RAGGED (a level of EC3D_COARSEN_AGGREGATE whose axis is odd): a child beyond the box is skipped and the mean is over
// the children that exist, 1, 2, 4 or 8 of them; without it the aggregates are full and no bound is tested.
template <bool DICT, bool RAGGED, class T = double>
__global__ __launch_bounds__(256) void k_mg_restrict(MgOpT<T> A, MgOpT<T> C, int fx, int fy, int fz, Gate g,
                                                     const T *__restrict__ w, const T *__restrict__ b,
                                                     T *__restrict__ bc)
{
    __shared__ T tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    const int64_t rc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rc >= C.n) return;
    const Pos pc = pos_of(C, rc);
    T s = T(0);
    int children = RAGGED ? 0 : fx * fy * fz;
    for (int dk = 0; dk < fz && (!RAGGED || pc.k * fz + dk < A.sdz); ++dk)
        for (int dj = 0; dj < fy && (!RAGGED || pc.j * fy + dj < A.sdy); ++dj)
            for (int di = 0; di < fx && (!RAGGED || pc.i * fx + di < A.sdx); ++di) {
                const Pos p{pc.i * fx + di, pc.j * fy + dj, pc.k * fz + dk};
                const int64_t r = (int64_t)p.k * A.kdz + (int64_t)p.j * A.sdx + p.i;
                if constexpr (RAGGED) ++children;
                T c[7], v[6];
                row_coefs<DICT>(A, tbl, r, c);
                neighbours(A, p, r, [&](int64_t q) { return w[q]; }, v);
                T t = b[r];
                t = t - c[0] * v[0];
                t = t - c[1] * v[1];
                t = t - c[2] * v[2];
                t = t - c[3] * w[r];
                t = t - c[4] * v[3];
                t = t - c[5] * v[4];
                t = t - c[6] * v[5];
                s = s + t;
            }
    bc[rc] = s * (T(1) / (T)children);
}

// Prolongation (piecewise-constant injection) + correction fused with the first post-smoothing half-sweep (black):
// red rows x = w + xc[parent]; black rows the GS value from the corrected red neighbours.  Bytes per fine row: w 8 +
// b 8 (black rows; the lines hold both colours) + 1 class byte read, x 8 written, xc from the L2 = 25 B.
// T = float: 13 B.
template <bool DICT, class T = double>
__global__ __launch_bounds__(256) void k_mg_prolong(MgOpT<T> A, MgOpT<T> C, int fx, int fy, int fz, Gate g,
                                                    const T *__restrict__ w, const T *__restrict__ xc,
                                                    const T *__restrict__ b, T *__restrict__ x)
{
    __shared__ T tbl[EC3D_MG_MAXCLS * 7];
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
    T c[7], v[6];
    row_coefs<DICT>(A, tbl, r, c);
    neighbours(A, p, r, corrected, v);
    x[r] = gs_value(c, v, b[r]);
}

// Coarsest level: `sweeps` sweeps of (red, black, black, red) from x = 0 by one workgroup, x in LDS, b and the class of
// a thread's (at most four) rows in registers.  A fixed linear operator of b, so BiCGSTAB stays valid.
// TB: the precision b arrives in -- T, except on a single-level fp32 hierarchy, whose only launch reads the fp64
// right-hand side and narrows it on load.
template <bool DICT, class T = double, class TB = T>
__global__ __launch_bounds__(EC3D_MG_COARSE_THREADS) void k_mg_coarse(MgOpT<T> A, Gate g, int sweeps,
                                                                      const TB *__restrict__ b, T *__restrict__ x)
{
    constexpr int RPT = EC3D_MG_COARSE_ROWS / EC3D_MG_COARSE_THREADS;
    __shared__ T xs[EC3D_MG_COARSE_ROWS];
    __shared__ T tbl[EC3D_MG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    T br[RPT];
    Pos pr[RPT];
    int colr[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int64_t r = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
        colr[q] = -1;
        if (r < A.n) {
            pr[q] = pos_of(A, r);
            colr[q] = (pr[q].i + pr[q].j + pr[q].k) & 1;
            br[q] = (T)b[r];
            xs[r] = T(0);
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
                T c[7], v[6];
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

// Galerkin coarse operator of piecewise-constant aggregation (EC3D_COARSEN_AGGREGATE), in the arithmetic and order of
// k_avmg_galerkin: coarse band q = the sum of the children's couplings that cross the aggregate's face on that side (to
// a cell inside the box), the diagonal = the children's diagonals plus their couplings inside the aggregate; children k
// outermost, i innermost, within a child the diagonal first and then the couplings in offset order; times `scale` =
// 1 / (2 * nominal children).  DICT is the form of the finer level F.  One thread per coarse cell, fp64, once at set-up.
template <bool DICT>
__global__ __launch_bounds__(256) void k_mg_galerkin(MgOp F, MgOp C, int fx, int fy, int fz, double scale,
                                                     double *__restrict__ bands)
{
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    if (DICT) load_table(F, tbl);
    const int64_t rc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rc >= C.n) return;
    const Pos pc = pos_of(C, rc);
    double D = 0.0, B[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int ext[3] = {F.sdx, F.sdy, F.sdz}, f[3] = {fx, fy, fz}, agg[3] = {pc.i, pc.j, pc.k};
    // offset order: axis and direction of band q (q = 3, the diagonal, is skipped)
    const int qax[7] = {2, 1, 0, -1, 0, 1, 2}, qdir[7] = {-1, -1, -1, 0, 1, 1, 1};
    for (int dk = 0; dk < fz && pc.k * fz + dk < F.sdz; ++dk)
        for (int dj = 0; dj < fy && pc.j * fy + dj < F.sdy; ++dj)
            for (int di = 0; di < fx && pc.i * fx + di < F.sdx; ++di) {
                const int pos[3] = {pc.i * fx + di, pc.j * fy + dj, pc.k * fz + dk};
                const int64_t r = (int64_t)pos[2] * F.kdz + (int64_t)pos[1] * F.sdx + pos[0];
                double c[7];
                row_coefs<DICT>(F, tbl, r, c);
                D = D + c[3];
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    if (q == 3) continue;
                    const int a = qax[q], nb = pos[a] + qdir[q];
                    if (nb < 0 || nb >= ext[a]) continue;
                    if (nb / f[a] == agg[a]) D = D + c[q];
                    else B[q] = B[q] + c[q];
                }
            }
#pragma unroll
    for (int q = 0; q < 7; ++q) bands[(size_t)q * C.n_pad + rc] = (q == 3 ? D : B[q]) * scale;
}

// ---- a matrix from ec3d_set_matrix_csr as level 0 (ec3d_set_precond_grid) -------------------------------------------
// The handle's stored matrix as the checks and the gather read it: band b of row r from the dictionary or the band
// streams, and the slot q (offset order -z, -y, -x, diag, +x, +y, +z) of every band, -1 for an offset that is not the box's.
struct MgSrc {
    const double *bands;      // band form: bands[b * n_pad + r]
    const uint8_t *cls;       // dictionary form (cls != nullptr): table[cls[r] * nb + b]
    const double *table;
    const int32_t *tail_id;   // nullptr: the matrix has no tail
    int nb;
    int slot[EC3D_MAXB];      // band b -> q, or -1
    int band[7];              // q -> band, or -1 (a zero stream)
    int sdx, sdy;
    int64_t n, n_pad, kdz;
};
__device__ __forceinline__ double src_coef(const MgSrc &S, int b, int64_t r)
{
    return S.cls ? S.table[(size_t)S.cls[r] * S.nb + b] : S.bands[(size_t)b * S.n_pad + r];
}
// why a row is no row of a 7-point operator on the box, in the order the set-up states them
enum { MG_BAD_TAIL = 0, MG_BAD_OFFSET = 1, MG_BAD_WRAP = 2, MG_BAD_DIAG = 3 };
// One thread per row.  out[0]: the kinds found, one bit each (atomic or); out[1]: the smallest row * 4 + kind (atomic
// min), so the first offending row and the first reason it offends; both untouched by a matrix that passes.  Bytes per
// row: the stored form once (1 class byte, or 8 nb) + 4 with a tail.
__global__ __launch_bounds__(256) void k_mg_check_grid(MgSrc S, unsigned long long *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S.n) return;
    const int i = (int)(r % S.sdx), j = (int)((r % S.kdz) / S.sdx);
    int bad = -1;
    const auto note = [&](int kind) { if (bad < 0 || kind < bad) bad = kind; };
    if (S.tail_id && S.tail_id[r] >= 0) note(MG_BAD_TAIL);
    double d = 0.0;
    for (int b = 0; b < S.nb; ++b) {
        const double v = src_coef(S, b, r);
        const int q = S.slot[b];
        if (q < 0) {
            if (v != 0.0) note(MG_BAD_OFFSET);
            continue;
        }
        if (q == 3) d = v;
        // a slot whose neighbour lies beyond the box along x or y is another cell of the numbering (the z slots would be
        // columns outside the matrix)
        const bool wrap = (q == 2 && i == 0) || (q == 4 && i == S.sdx - 1) || (q == 1 && j == 0) || (q == 5 && j == S.sdy - 1);
        if (wrap && v != 0.0) note(MG_BAD_WRAP);
    }
    if (d == 0.0 || !isfinite(d)) note(MG_BAD_DIAG);
    if (bad < 0) return;
    atomicOr(&out[0], 1ull << bad);
    atomicMin(&out[1], (unsigned long long)r * 4ull + (unsigned long long)bad);
}

// Level 0's seven band streams gathered from the stored form, bits unchanged, a band the matrix does not have as zeros;
// rows [n, n_pad) as stored (zeros).  Bytes per row: the stored form once, 56 written.
__global__ __launch_bounds__(256) void k_mg_gather(MgSrc S, double *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S.n_pad) return;
#pragma unroll
    for (int q = 0; q < 7; ++q) out[(size_t)q * S.n_pad + r] = S.band[q] >= 0 ? src_coef(S, S.band[q], r) : 0.0;
}

// ---- the outer iteration's operator on level 0 (its other kernels: ec3d_outer.hip) ----------------------------------
// Grid-strided over rows like them (thread t of workgroup b takes the rows b * 256 + t + m * 256 * gridDim.x in
// increasing m); the workgroup sums are ec3d_stream.hpp's.
// y = A x (rows summed in offset order from the -z term); partials of a.y (slot 0) and, with two, y.y (slot 1).
// Bytes per row: x 8 + a 8 + 1 class byte read, y 8 written = 25 B.
// TX = float: x is p^ / s^ of the fp32 V-cycle, widened on load (exact); every product and sum stays fp64 (21 B).
template <bool DICT, class TX = double>
__global__ __launch_bounds__(256) void k_mg_spmv_dot(MgOp A, Gate g, const TX *__restrict__ x,
                                                     const double *__restrict__ a, double *__restrict__ y, int two,
                                                     double *__restrict__ part)
{
    __shared__ double tbl[EC3D_MG_MAXCLS * 7];
    __shared__ double lds[4];
    if (gated_off(g)) return;
    if (DICT) load_table(A, tbl);
    double d0 = 0.0, d1 = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.n; r += (int64_t)gridDim.x * blockDim.x) {
        const Pos p = pos_of(A, r);
        double c[7], v[6];
        row_coefs<DICT>(A, tbl, r, c);
        neighbours(A, p, r, [&](int64_t q) { return (double)x[q]; }, v);
        double s = c[0] * v[0];
        s = s + c[1] * v[1];
        s = s + c[2] * v[2];
        s = s + c[3] * (double)x[r];
        s = s + c[4] * v[3];
        s = s + c[5] * v[4];
        s = s + c[6] * v[5];
        y[r] = s;
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

// kern<DICT> on operator A (the kernel's first argument): the class form when A has class bytes, else the band form
#define MG_LAUNCH(kern, grid, block, A, ...)                                                                       \
    do {                                                                                                           \
        if ((A).cls) kern<true><<<(grid), (block), 0, s>>>(A, __VA_ARGS__);                                       \
        else kern<false><<<(grid), (block), 0, s>>>(A, __VA_ARGS__);                                              \
    } while (0)

// ... with a second template flag
#define MG_LAUNCH2(kern, flag, grid, block, A, ...)                                                                \
    do {                                                                                                           \
        if ((A).cls) kern<true, flag><<<(grid), (block), 0, s>>>(A, __VA_ARGS__);                                 \
        else kern<false, flag><<<(grid), (block), 0, s>>>(A, __VA_ARGS__);                                        \
    } while (0)

// the fine level's first half-sweep (red, from x = 0); fp32: it also narrows r into b0
inline void launch_fine_init(const PoissonMg<double> &h, Gate g, const double *r, hipStream_t s)
{
    const MgOp &A = h.lev[0].op;
    MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, 0, 1, h.w0, r);
}
inline void launch_fine_init(const PoissonMg<float> &h, Gate g, const double *r, hipStream_t s)
{
    const MgOp32 &A = h.lev[0].op;
    MG_LAUNCH(k_mg_init_f32, blocks_of(A.n), 256, A, g, r, h.b0, h.w0);
}

// The V-cycle's launch schedule from x = 0, for either kernel family (k_mg_* in the hierarchy's precision, k_avmg_*).
// The family's launches on level l: smooth(l, colour, init, post) a half-sweep, on w before the coarse correction and on
// x behind it (post); restrict_(l) the right-hand side of level l + 1; coarse() the coarsest level's solve; prolong(l)
// x = w + the correction, fused with the first post half-sweep (black).
template <class S, class R, class C, class P>
void launch_schedule(int L, int pre, int post, const S &smooth, const R &restrict_, const C &coarse, const P &prolong)
{
    for (int l = 0; l + 1 < L; ++l) {
        for (int sw = 0; sw < pre; ++sw) {
            smooth(l, 0, sw == 0, false);
            smooth(l, 1, 0, false);
        }
        restrict_(l);
    }
    coarse();
    for (int l = L - 2; l >= 0; --l) {
        prolong(l);
        smooth(l, 0, 0, true);
        for (int sw = 1; sw < post; ++sw) {
            smooth(l, 1, 0, true);
            smooth(l, 0, 0, true);
        }
    }
}

// one V-cycle z = M r (enqueued).  T = float (EC3D_PRECOND_FP32): r stays fp64; the fine level's init half-sweep narrows
// it into b0 (k_mg_init_f32), or the coarse solve does on load when the hierarchy has one level.
template <class T>
void launch_cycle(const ec3d_mg &m, const PoissonMg<T> &h, Gate g, const double *r, T *z, hipStream_t s)
{
    const int L = (int)h.lev.size();
    const auto &lev = h.lev;
    const T *b0 = h.b0; // the fine right-hand side: float the narrowed copy, double r itself
    if constexpr (std::is_same_v<T, double>) b0 = r;
    const auto B = [&](int l) { return l ? (const T *)lev[l].b : b0; };
    const auto W = [&](int l, bool post = false) { return post ? (l ? lev[l].x : z) : (l ? lev[l].w : h.w0); };
    launch_schedule(
        L, m.pre, m.post,
        [&](int l, int colour, int init, bool post) {
            const MgOpT<T> &A = lev[l].op;
            if (l == 0 && init) launch_fine_init(h, g, r, s);
            else MG_LAUNCH(k_mg_smooth, blocks_of(A.n), 256, A, g, colour, init, W(l, post), B(l));
        },
        [&](int l) {
            const MgOpT<T> &A = lev[l].op, &C = lev[l + 1].op;
            const int *f = h.grid[(size_t)l].f;
            // ragged: an axis of A is not f times C's (ceil-halving of an odd extent)
            if (C.sdx * f[0] != A.sdx || C.sdy * f[1] != A.sdy || C.sdz * f[2] != A.sdz)
                MG_LAUNCH2(k_mg_restrict, true, blocks_of(C.n), 256, A, C, f[0], f[1], f[2], g, W(l), B(l), lev[l + 1].b);
            else
                MG_LAUNCH2(k_mg_restrict, false, blocks_of(C.n), 256, A, C, f[0], f[1], f[2], g, W(l), B(l), lev[l + 1].b);
        },
        [&] {
            const MgLevelT<T> &K = lev[L - 1];
            if (L == 1) MG_LAUNCH(k_mg_coarse, 1, EC3D_MG_COARSE_THREADS, K.op, g, m.coarse, r, z);
            else MG_LAUNCH(k_mg_coarse, 1, EC3D_MG_COARSE_THREADS, K.op, g, m.coarse, K.b, K.x);
        },
        [&](int l) {
            const MgOpT<T> &A = lev[l].op, &C = lev[l + 1].op;
            const int *f = h.grid[(size_t)l].f;
            MG_LAUNCH(k_mg_prolong, blocks_of(A.n), 256, A, C, f[0], f[1], f[2], g, W(l), lev[l + 1].x, B(l), W(l, true));
        });
}

// fp64 -> fp32, round to nearest: a level's coefficients at set-up
__global__ __launch_bounds__(256) void k_mg_narrow(int64_t n, const double *__restrict__ a, float *__restrict__ o)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) o[q] = (float)a[q];
}
// fp32 -> fp64 (exact): z of ec3d_precond_apply on an fp32 hierarchy
__global__ __launch_bounds__(256) void k_mg_widen(int64_t n, const float *__restrict__ a, double *__restrict__ o)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) o[q] = (double)a[q];
}

// ---- block multigrid of the structured A-V form (EC3D_PRECOND_BLOCK_MG) ----------------------
// The kernels below restate k_mg_smooth / k_mg_restrict / k_mg_prolong / k_mg_coarse for the A blocks with three
// right-hand sides per launch (the blocks' vectors vs apart: one read of a row's coefficients serves all three), rows
// without a diagonal (level 0's padding rows) producing 0, and aggregates of ceil-halving (an odd axis ends in an
// aggregate of one cell).  tests/avmg_numpy.py restates them operation by operation.
#define EC3D_AVMG_MAXCLS 64 // classes of one block the smoothers' table holds (the native structured form: 27 + 9 D A
                            // classes with D conducting domains, so D <= 4; 27 U)

__device__ __forceinline__ void av_load_table(const AvOp &A, double *tbl)
{
    if (!A.cls) return;
    for (int q = threadIdx.x; q < A.ncls * 7; q += blockDim.x) tbl[q] = A.table[(size_t)(A.cls0 + q / 7) * 16 + q % 7];
    __syncthreads();
}
template <bool DICT> __device__ __forceinline__ void av_coefs(const AvOp &A, const double *tbl, int64_t r, double (&c)[7])
{
    if constexpr (DICT) {
        const unsigned k = (unsigned)((int)A.cls[r] - A.cls0);
        if (k >= (unsigned)A.ncls) {
#pragma unroll
            for (int q = 0; q < 7; ++q) c[q] = 0.0;
            return;
        }
        const double *t = tbl + 7 * k;
#pragma unroll
        for (int q = 0; q < 7; ++q) c[q] = t[q];
    } else {
#pragma unroll
        for (int q = 0; q < 7; ++q) c[q] = A.bands[(size_t)q * A.n_pad + r];
    }
}
template <bool DICT> __device__ __forceinline__ double av_diag(const AvOp &A, const double *tbl, int64_t r)
{
    if constexpr (DICT) {
        const unsigned k = (unsigned)((int)A.cls[r] - A.cls0);
        return k < (unsigned)A.ncls ? tbl[7 * k + 3] : 0.0;
    } else {
        return A.bands[(size_t)3 * A.n_pad + r];
    }
}

// Half-sweep of one colour on the three blocks, in place (k_mg_smooth).  Level 0, bytes per cell: class 1 + 3 x (b 8 +
// x 8 read + x 8 written) = 73 B; init: 1 + 3 x 16 = 49 B.
template <bool DICT>
__global__ __launch_bounds__(256) void k_avmg_smooth(AvOp A, Gate g, int colour, int init, double *__restrict__ x,
                                                     const double *__restrict__ b)
{
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) av_load_table(A, tbl);
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const Pos p = pos_of(A, r);
    if (((p.i + p.j + p.k) & 1) != colour) {
        if (init)
            for (int d = 0; d < 3; ++d) x[d * A.vs + r] = 0.0;
        return;
    }
    double c[7];
    av_coefs<DICT>(A, tbl, r, c);
    const bool live = c[3] != 0.0 && p.j < A.sdy;
    for (int d = 0; d < 3; ++d) {
        const int64_t o = d * A.vs;
        double val = 0.0;
        if (live && init) {
            val = b[o + r] / c[3];
        } else if (live) {
            double v[6];
            neighbours(A, p, r, [&](int64_t q) { return x[o + q]; }, v);
            val = gs_value(c, v, b[o + r]);
        }
        x[o + r] = val;
    }
}

// Residual + mean restriction over the aggregate's actual children (k_mg_restrict), three blocks.
template <bool DICT>
__global__ __launch_bounds__(256) void k_avmg_restrict(AvOp A, AvOp C, int fx, int fy, int fz, Gate g,
                                                       const double *__restrict__ w, const double *__restrict__ b,
                                                       double *__restrict__ bc)
{
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) av_load_table(A, tbl);
    const int64_t rc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rc >= C.n) return;
    const Pos pc = pos_of(C, rc);
    double s[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int dk = 0; dk < fz && pc.k * fz + dk < A.sdz; ++dk)
        for (int dj = 0; dj < fy && pc.j * fy + dj < A.sdy; ++dj)
            for (int di = 0; di < fx && pc.i * fx + di < A.sdx; ++di) {
                const Pos p{pc.i * fx + di, pc.j * fy + dj, pc.k * fz + dk};
                const int64_t r = (int64_t)p.k * A.kdz + (int64_t)p.j * A.sdx + p.i;
                double c[7];
                av_coefs<DICT>(A, tbl, r, c);
                ++cnt;
                for (int d = 0; d < 3; ++d) {
                    const int64_t o = d * A.vs;
                    double v[6];
                    neighbours(A, p, r, [&](int64_t q) { return w[o + q]; }, v);
                    double t = b[o + r];
                    t = t - c[0] * v[0];
                    t = t - c[1] * v[1];
                    t = t - c[2] * v[2];
                    t = t - c[3] * w[o + r];
                    t = t - c[4] * v[3];
                    t = t - c[5] * v[4];
                    t = t - c[6] * v[5];
                    s[d] = s[d] + t;
                }
            }
    const double mean = 1.0 / (double)cnt;
    for (int d = 0; d < 3; ++d) bc[d * C.vs + rc] = s[d] * mean;
}

// Prolongation + correction fused with the first post half-sweep (black), three blocks (k_mg_prolong).  A row without
// a diagonal is 0, as the corrected value its neighbours read.
template <bool DICT>
__global__ __launch_bounds__(256) void k_avmg_prolong(AvOp A, AvOp C, int fx, int fy, int fz, Gate g,
                                                      const double *__restrict__ w, const double *__restrict__ xc,
                                                      const double *__restrict__ b, double *__restrict__ x)
{
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) av_load_table(A, tbl);
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const Pos p = pos_of(A, r);
    double c[7];
    av_coefs<DICT>(A, tbl, r, c);
    const bool live = c[3] != 0.0 && p.j < A.sdy;
    const auto parent = [&](const Pos &q) {
        return (int64_t)(q.k / fz) * C.kdz + (int64_t)(q.j / fy) * C.sdx + q.i / fx;
    };
    const bool red = ((p.i + p.j + p.k) & 1) == 0;
    for (int d = 0; d < 3; ++d) {
        const int64_t o = d * A.vs, oc = d * C.vs;
        double val = 0.0;
        if (live && red) {
            val = w[o + r] + xc[oc + parent(p)];
        } else if (live) {
            const auto corrected = [&](int64_t q) {
                if (av_diag<DICT>(A, tbl, q) == 0.0) return 0.0;
                return w[o + q] + xc[oc + parent(pos_of(A, q))];
            };
            double v[6];
            neighbours(A, p, r, corrected, v);
            val = gs_value(c, v, b[o + r]);
        }
        x[o + r] = val;
    }
}

// Coarsest level (k_mg_coarse): workgroup d solves block d; x of the level's cells in LDS, indexed by cell (level 0's
// rows are pitched: cell (i, j, k) is row k kdz + j sdx + i).
template <bool DICT>
__global__ __launch_bounds__(EC3D_MG_COARSE_THREADS) void k_avmg_coarse(AvOp A, Gate g, int sweeps,
                                                                        const double *__restrict__ b,
                                                                        double *__restrict__ x)
{
    constexpr int RPT = EC3D_MG_COARSE_ROWS / EC3D_MG_COARSE_THREADS;
    __shared__ double xs[EC3D_MG_COARSE_ROWS];
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (gated_off(g)) return;
    if (DICT) av_load_table(A, tbl);
    AvOp Ac = A; // the same grid in cell numbering
    Ac.kdz = (int64_t)A.sdx * A.sdy;
    const int64_t ncell = Ac.kdz * A.sdz, o = (int64_t)blockIdx.x * A.vs;
    double br[RPT];
    Pos pr[RPT];
    int colr[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int64_t e = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
        colr[q] = -1;
        if (e < ncell) {
            pr[q] = pos_of(Ac, e);
            colr[q] = (pr[q].i + pr[q].j + pr[q].k) & 1;
            br[q] = b[o + (int64_t)pr[q].k * A.kdz + (int64_t)pr[q].j * A.sdx + pr[q].i];
            xs[e] = 0.0;
        }
    }
    __syncthreads();
    for (int s = 0; s < sweeps; ++s)
        for (int h = 0; h < 4; ++h) {
            const int colour = (h == 0 || h == 3) ? 0 : 1;
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                if (colr[q] != colour) continue;
                const int64_t e = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
                double c[7], v[6];
                av_coefs<DICT>(A, tbl, (int64_t)pr[q].k * A.kdz + (int64_t)pr[q].j * A.sdx + pr[q].i, c);
                if (c[3] == 0.0) continue; // stays 0
                neighbours(Ac, pr[q], e, [&](int64_t t) { return xs[t]; }, v);
                xs[e] = gs_value(c, v, br[q]);
            }
            __syncthreads();
        }
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int64_t e = threadIdx.x + (int64_t)q * EC3D_MG_COARSE_THREADS;
        if (e < ncell) x[o + (int64_t)pr[q].k * A.kdz + (int64_t)pr[q].j * A.sdx + pr[q].i] = xs[e];
    }
}

// Galerkin coarse operator of piecewise-constant aggregation: coarse band q = the sum of the children's couplings that
// cross the aggregate's face on that side (to a cell inside the box), the diagonal = the children's diagonals plus their
// couplings inside the aggregate; children k outermost, i innermost, within a child the diagonal first and then the
// couplings in offset order; times `scale` = 1 / (2 * nominal children).  One thread per coarse cell.
template <bool DICT>
__global__ __launch_bounds__(256) void k_avmg_galerkin(AvOp F, AvOp C, int fx, int fy, int fz, double scale,
                                                       double *__restrict__ bands)
{
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (DICT) av_load_table(F, tbl);
    const int64_t rc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rc >= C.n) return;
    const Pos pc = pos_of(C, rc);
    double D = 0.0, B[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int ext[3] = {F.sdx, F.sdy, F.sdz}, f[3] = {fx, fy, fz}, agg[3] = {pc.i, pc.j, pc.k};
    // offset order: axis and direction of band q (q = 3, the diagonal, is skipped)
    const int qax[7] = {2, 1, 0, -1, 0, 1, 2}, qdir[7] = {-1, -1, -1, 0, 1, 1, 1};
    for (int dk = 0; dk < fz && pc.k * fz + dk < F.sdz; ++dk)
        for (int dj = 0; dj < fy && pc.j * fy + dj < F.sdy; ++dj)
            for (int di = 0; di < fx && pc.i * fx + di < F.sdx; ++di) {
                const int pos[3] = {pc.i * fx + di, pc.j * fy + dj, pc.k * fz + dk};
                const int64_t r = (int64_t)pos[2] * F.kdz + (int64_t)pos[1] * F.sdx + pos[0];
                double c[7];
                av_coefs<DICT>(F, tbl, r, c);
                D = D + c[3];
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    if (q == 3) continue;
                    const int a = qax[q], nb = pos[a] + qdir[q];
                    if (nb < 0 || nb >= ext[a]) continue;
                    if (nb / f[a] == agg[a]) D = D + c[q];
                    else B[q] = B[q] + c[q];
                }
            }
#pragma unroll
    for (int q = 0; q < 7; ++q) bands[(size_t)q * C.n_pad + rc] = (q == 3 ? D : B[q]) * scale;
}

// Gauss-Seidel half-sweep of the U block over a list of its unknowns' rows (one colour); init: from zero, x = b / d.
// The right-hand side of a row is b - umean[its component] (the projection below).
__global__ __launch_bounds__(256) void k_avmg_usweep(AvOp U, Gate g, const int32_t *__restrict__ list,
                                                     const int32_t *__restrict__ comp, const double *__restrict__ umean,
                                                     int64_t count, int init, double *__restrict__ x,
                                                     const double *__restrict__ b)
{
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (gated_off(g)) return;
    av_load_table(U, tbl);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const int64_t r = list[e];
    double c[7];
    av_coefs<true>(U, tbl, r, c);
    const double bb = b[r] - umean[comp[e]];
    double val = 0.0;
    if (c[3] != 0.0 && init) {
        val = bb / c[3];
    } else if (c[3] != 0.0) {
        double v[6];
        neighbours(U, pos_of(U, r), r, [&](int64_t q) { return x[q]; }, v);
        val = gs_value(c, v, bb);
    }
    x[r] = val;
}

// The same half-sweep on U^T (N of the adjoint solves): the coefficient towards neighbour q is the NEIGHBOUR's row's
// coefficient 6 - q, looked up under the neighbour's U class once the neighbour is known to lie inside the box; a
// neighbour without a U unknown gives 0.  The diagonal is the row's own.
__global__ __launch_bounds__(256) void k_avmg_usweep_t(AvOp U, Gate g, const int32_t *__restrict__ list,
                                                       const int32_t *__restrict__ comp, const double *__restrict__ umean,
                                                       int64_t count, int init, double *__restrict__ x,
                                                       const double *__restrict__ b)
{
    __shared__ double tbl[EC3D_AVMG_MAXCLS * 7];
    if (gated_off(g)) return;
    av_load_table(U, tbl);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const int64_t r = list[e];
    const double d = av_diag<true>(U, tbl, r);
    const double bb = b[r] - umean[comp[e]];
    double val = 0.0;
    if (d != 0.0 && init) {
        val = bb / d;
    } else if (d != 0.0) {
        const Pos p = pos_of(U, r);
        const int64_t off[7] = {-U.kdz, -(int64_t)U.sdx, -1, 0, 1, U.sdx, U.kdz};
        const bool in[7] = {p.k > 0, p.j > 0, p.i > 0, false, p.i + 1 < U.sdx, p.j + 1 < U.sdy, p.k + 1 < U.sdz};
        double c[7], v[6];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            c[q] = 0.0;
            if (!in[q]) continue;
            const unsigned kn = (unsigned)((int)U.cls[r + off[q]] - U.cls0);
            if (kn < (unsigned)U.ncls) c[q] = tbl[7 * kn + 6 - q];
        }
        c[3] = d;
        neighbours(U, p, r, [&](int64_t q) { return x[q]; }, v);
        val = gs_value(c, v, bb);
    }
    x[r] = val;
}

// x = x - umean[its component] on the U unknowns' rows: the output projection of N
__global__ __launch_bounds__(256) void k_avmg_usub(Gate g, const int32_t *__restrict__ list,
                                                   const int32_t *__restrict__ comp, const double *__restrict__ umean,
                                                   int64_t count, double *__restrict__ x)
{
    if (gated_off(g)) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const int64_t r = list[e];
    x[r] = x[r] - umean[comp[e]];
}

// Level 0 of the TRANSPOSED A block as seven band streams (set-up of N, once): band q of row r is band 6 - q of row
// r + off[q], looked up under that row's class byte once the neighbour is known to lie inside the box and to have a
// class in [cls0, cls0 + ncls) -- else 0 --; the diagonal is the row's own.  A row without coefficients stays one.
__global__ __launch_bounds__(256) void k_avmg_gather_t(AvOp A, double *__restrict__ bands, int64_t n_pad)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const Pos p = pos_of(A, r);
    const unsigned k = (unsigned)((int)A.cls[r] - A.cls0);
    double c[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (k < (unsigned)A.ncls && p.j < A.sdy) {
        const int64_t off[7] = {-A.kdz, -(int64_t)A.sdx, -1, 0, 1, A.sdx, A.kdz};
        const bool in[7] = {p.k > 0, p.j > 0, p.i > 0, false, p.i + 1 < A.sdx, p.j + 1 < A.sdy, p.k + 1 < A.sdz};
        c[3] = A.table[(size_t)(A.cls0 + (int)k) * 16 + 3];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            if (!in[q]) continue;
            const unsigned kn = (unsigned)((int)A.cls[r + off[q]] - A.cls0);
            if (kn < (unsigned)A.ncls) c[q] = A.table[(size_t)(A.cls0 + (int)kn) * 16 + 6 - q];
        }
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) bands[(size_t)q * n_pad + r] = c[q];
}

// The U block of the A-V system is singular: a constant on one conducting component (A = 0) is a null vector of the
// whole operator, and the U rows' left null vector is w = the product over the axes of 1/2 where the cell misses a
// neighbour along that axis, 1 elsewhere (the one-sided rows carry the factor 2; exact where a missing neighbour is
// on one side only, an approximation otherwise -- M stays a fixed linear operator either way).  Gauss-Seidel on a right-hand side
// with a component along that null direction does not converge, and the outer iteration stalls; so the U sweeps see
// b - (w.b / w.1) on each component, which lies in the U block's range.  The weighted sums run in a fixed order:
// chunks of EC3D_AVMG_UCHUNK entries of one component (thread t adds entries t, t + 256, ..., then the workgroup
// tree), then per component the chunks' partials as k_mg_scalar sums them.
__global__ __launch_bounds__(256) void k_avmg_upart(Gate g, const int32_t *__restrict__ plist,
                                                    const double *__restrict__ pw, const int32_t *__restrict__ chunks,
                                                    const double *__restrict__ b, double *__restrict__ upart)
{
    __shared__ double lds[4];
    if (gated_off(g)) return;
    const int lo = chunks[2 * blockIdx.x], hi = chunks[2 * blockIdx.x + 1];
    double a = 0.0;
    for (int e = lo + (int)threadIdx.x; e < hi; e += (int)blockDim.x) a = a + pw[e] * b[plist[e]];
    a = stream_block_sum(a, lds);
    if (threadIdx.x == 0) upart[blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void k_avmg_umean(Gate g, const int32_t *__restrict__ cco,
                                                    const double *__restrict__ upart, const double *__restrict__ inv_w,
                                                    double *__restrict__ umean)
{
    __shared__ double lds[4];
    if (gated_off(g)) return;
    const int lo = cco[blockIdx.x], hi = cco[blockIdx.x + 1];
    const double a = stream_block_sum(stream_strided_sum(upart + lo, hi - lo), lds);
    if (threadIdx.x == 0) umean[blockIdx.x] = a * inv_w[blockIdx.x];
}

// z = M r of the block multigrid (enqueued): one V-cycle on each A block, the U block's sweeps.  r, z: device vectors
// of the structured form (4 blocks of nCd rows).
void launch_cycle(const ec3d_mg &m, const BlockMg &h, Gate g, const double *r, double *z, hipStream_t s)
{
    const int L = (int)h.lev.size();
    const auto &lev = h.lev;
    const auto B = [&](int l) -> const double * { return l ? lev[l].b : r; };
    const auto W = [&](int l, bool post = false) { return post ? (l ? lev[l].x : z) : (l ? lev[l].w : h.w0); };
    launch_schedule(
        L, m.pre, m.post,
        [&](int l, int colour, int init, bool post) {
            const AvOp &A = lev[l].op;
            MG_LAUNCH(k_avmg_smooth, blocks_of(A.n), 256, A, g, colour, init, W(l, post), B(l));
        },
        [&](int l) {
            const AvLevel &F = lev[l], &C = lev[l + 1];
            MG_LAUNCH(k_avmg_restrict, blocks_of(C.op.n), 256, F.op, C.op, F.f[0], F.f[1], F.f[2], g, W(l), B(l), C.b);
        },
        [&] {
            const AvLevel &K = lev[L - 1];
            MG_LAUNCH(k_avmg_coarse, 3, EC3D_MG_COARSE_THREADS, K.op, g, m.coarse, L == 1 ? r : K.b, L == 1 ? z : K.x);
        },
        [&](int l) {
            const AvLevel &F = lev[l], &C = lev[l + 1];
            MG_LAUNCH(k_avmg_prolong, blocks_of(F.op.n), 256, F.op, C.op, F.f[0], F.f[1], F.f[2], g, W(l), C.x, B(l),
                      W(l, true));
        });
    const int64_t ub = 3 * h.lev[0].op.vs; // the U block
    if (h.ncomp) {
        k_avmg_upart<<<(unsigned)h.nchunk, 256, 0, s>>>(g, h.plist, h.pw, h.chunks, r + ub, h.upart);
        k_avmg_umean<<<(unsigned)h.ncomp, 256, 0, s>>>(g, h.cco, h.upart, h.inv_w, h.umean);
    }
    const auto usweep = h.adjoint ? k_avmg_usweep_t : k_avmg_usweep;
    for (int sw = 0; sw < m.pre + m.post; ++sw) {
        if (h.nu_red)
            usweep<<<blocks_of(h.nu_red), 256, 0, s>>>(h.uop, g, h.ulist, h.ucomp, h.umean, h.nu_red, sw == 0, z + ub, r + ub);
        if (h.nu_black)
            usweep<<<blocks_of(h.nu_black), 256, 0, s>>>(h.uop, g, h.ulist + h.nu_red, h.ucomp + h.nu_red, h.umean,
                                                        h.nu_black, 0, z + ub, r + ub);
    }
    if (h.adjoint && h.ncomp) { // N: the plain mean of every component leaves the swept z too
        const int64_t nu = h.nu_red + h.nu_black;
        k_avmg_upart<<<(unsigned)h.nchunk, 256, 0, s>>>(g, h.plist, h.pw, h.chunks, z + ub, h.upart);
        k_avmg_umean<<<(unsigned)h.ncomp, 256, 0, s>>>(g, h.cco, h.upart, h.inv_w, h.umean);
        k_avmg_usub<<<blocks_of(nu), 256, 0, s>>>(g, h.ulist, h.ucomp, h.umean, nu, z + ub);
    }
}

} // namespace

// ---- hierarchy rule (host): ec3d_mg_plan.hpp for EC3D_PRECOND_MG ----------------------------------------------------

// ---- block multigrid of the structured A-V form: set-up --------------------------------------------------------------
// Level dims: every axis whose extent is > 1 is ceil-halved, until a level has <= 4096 cells (always reached).
static std::vector<std::array<int, 3>> avmg_dims(int sdx, int sdy, int sdz)
{
    std::vector<std::array<int, 3>> dims(1, {sdx, sdy, sdz});
    while ((int64_t)dims.back()[0] * dims.back()[1] * dims.back()[2] > EC3D_MG_COARSE_ROWS) {
        std::array<int, 3> e = dims.back();
        for (int a = 0; a < 3; ++a)
            if (e[a] > 1) e[a] = (e[a] + 1) / 2;
        dims.push_back(e);
    }
    return dims;
}

static inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// a matrix or setting the preconditioner is not built for; a failure of the runtime during set-up.  Either way the new
// hierarchy is dropped and the handle stays as it was
static int mg_refuse(const std::string &text, int code = EC3D_PRECOND_E_MATRIX) { ec3d_set_error(text); return code; }
static int mg_fail(const char *what)
{
    (void)hipGetLastError();
    return mg_refuse(std::string("ec3d_set_preconditioner: ") + what, 100);
}
static const char *const MG_OOM = "out of device memory for the hierarchy", *const MG_BUILD = "building the hierarchy failed";

// The coarse vectors of a hierarchy inside its vector block: x, w, b per level in level order, each `blocks` vectors of
// the level's rows rounded up to 64.  Returns where they end: the fine vectors begin there.
template <class T, class LEVEL> static T *carve_vectors(T *q, std::vector<LEVEL> &lev, int blocks)
{
    for (size_t l = 1; l < lev.size(); ++l) {
        const int64_t len = blocks * pad64(lev[l].op.n);
        lev[l].x = q; lev[l].w = q + len; lev[l].b = q + 2 * len;
        q += 3 * len;
    }
    return q;
}

// Both set-ups fill a new ec3d_mg, which ec3d_set_preconditioner puts in the old one's place when they return 0.
// null_kind: EC3D_NULL_PRECOND_NONE for M of section 10; EC3D_NULL_PRECOND_BLOCK_MG / _A for N of the adjoint solves
// (the U block transposed and projected with plain means on both sides; BLOCK_MG: level 0 of the A blocks transposed too).
static int set_block_mg(ec3d_ctx *c, ec3d_mg &m, int null_kind = EC3D_NULL_PRECOND_NONE)
{
    const DevMatrix &A = c->A;
    if (!A.sav || !ec3d_own_handle(c))
        return mg_refuse("ec3d_set_preconditioner: the block multigrid preconditioner needs the structured A-V form "
                         "(ec3d_assemble) on a handle of its own (not Poisson, bands + tail, a slab or a handle of "
                         "ec3d_multi)");
    const int sdx = (int)A.sav_step[1], pitch = (int)A.sav_step[2];
    const int sdy = (int)(c->plane / sdx), sdz = (int)(A.sav_nC / pitch);
    const int64_t nCd = A.sav_nC;
    const int a_hi = A.sav_u0, u_lo = A.sav_u0, u_hi = A.sav_zero; // A rows: classes [0, u0); U rows: [u0, zero)
    if (a_hi > EC3D_AVMG_MAXCLS || u_hi - u_lo > EC3D_AVMG_MAXCLS)
        return mg_refuse("ec3d_set_preconditioner: more classes than the block smoothers' table holds (at most 4 "
                         "conducting domains)");
    std::vector<uint8_t> cls((size_t)(4 * nCd));
    std::vector<double> tab((size_t)A.ncls * 16);
    EC3D_HIP(hipMemcpyAsync(cls.data(), A.cls, cls.size(), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipMemcpyAsync(tab.data(), A.table, tab.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    AvmgPlan p;
    const std::string refusal =
        ec3d_avmg_plan(sdx, sdy, sdz, pitch, nCd, cls.data(), tab.data(), a_hi, u_lo, u_hi, EC3D_AVMG_UCHUNK, p);
    if (!refusal.empty()) return mg_refuse(refusal);
    if (null_kind != EC3D_NULL_PRECOND_NONE) ec3d_avmg_plain_means(p);
    const std::vector<std::array<int, 3>> dims = avmg_dims(sdx, sdy, sdz);
    const int L = (int)dims.size();
    BlockMg &h = m.h.emplace<BlockMg>();
    h.adjoint = null_kind != EC3D_NULL_PRECOND_NONE;
    h.lev.resize((size_t)L);
    AvOp &A0 = h.lev[0].op;
    A0 = AvOp{};
    A0.sdx = sdx; A0.sdy = sdy; A0.sdz = sdz;
    A0.kdz = pitch;
    A0.n = A0.vs = nCd;
    A0.cls = A.cls; // block 0's classes serve all three blocks (the plan checked it)
    A0.table = A.table;
    A0.cls0 = 0; A0.ncls = a_hi;
    h.uop = A0;
    h.uop.cls = A.cls + 3 * nCd;
    h.uop.cls0 = u_lo; h.uop.ncls = u_hi - u_lo;
    if (null_kind == EC3D_NULL_PRECOND_BLOCK_MG) { // level 0 of the transposed A block: gathered once, read as band streams
        if (h.bands0.alloc((size_t)7 * nCd) != hipSuccess) return mg_fail(MG_OOM);
        k_avmg_gather_t<<<blocks_of(nCd), 256, 0, c->stream>>>(A0, h.bands0, nCd);
        A0.cls = nullptr;
        A0.bands = h.bands0;
        A0.n_pad = nCd;
    }
    int64_t coarse_len = 0;
    for (int l = 1; l < L; ++l) {
        AvLevel &P = h.lev[(size_t)l - 1], &Q = h.lev[(size_t)l];
        for (int a = 0; a < 3; ++a) P.f[a] = dims[(size_t)l - 1][a] > 1 ? 2 : 1;
        AvOp &o = Q.op;
        o = AvOp{};
        o.sdx = dims[(size_t)l][0]; o.sdy = dims[(size_t)l][1]; o.sdz = dims[(size_t)l][2];
        o.kdz = (int64_t)o.sdx * o.sdy;
        o.n = o.kdz * o.sdz;
        o.vs = o.n_pad = pad64(o.n);
        if (Q.bands.alloc((size_t)7 * o.n_pad) != hipSuccess) return mg_fail(MG_OOM);
        o.bands = Q.bands;
        coarse_len += 9 * o.n_pad;
    }
    // p^ and s^ are read by the format's SpMV, which may read the zero halo around a vector (ec3d_prepare_vectors)
    const int64_t nf = c->ghost + pad64(A.n_pad) + c->ghost;
    const int64_t total = coarse_len + 3 * nCd + 2 * nf;
    h.nu_red = (int64_t)p.ured.size(); h.nu_black = (int64_t)p.ublack.size();
    if (h.vec.alloc((size_t)total) != hipSuccess || m.part.alloc(2 * EC3D_MG_DOT_BLOCKS) != hipSuccess ||
        m.scal.alloc(1) != hipSuccess || h.ulist.alloc(std::max<size_t>(1, p.ured.size() + p.ublack.size())) != hipSuccess)
        return mg_fail(MG_OOM);
    if (hipMemsetAsync(h.vec, 0, (size_t)total * sizeof(double), c->stream) != hipSuccess ||
        hipMemsetAsync(m.scal, 0, sizeof(MgScalars), c->stream) != hipSuccess ||
        (h.nu_red && hipMemcpyAsync(h.ulist, p.ured.data(), p.ured.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
        (h.nu_black && hipMemcpyAsync(h.ulist + h.nu_red, p.ublack.data(), p.ublack.size() * 4, hipMemcpyHostToDevice,
                                      c->stream) != hipSuccess))
        return mg_fail(MG_BUILD);
    h.ncomp = (int)p.inv_w.size(); h.nchunk = (int)(p.chunks.size() / 2);
    {
        std::vector<int32_t> hi(p.ucomp);
        hi.insert(hi.end(), p.plist.begin(), p.plist.end());
        hi.insert(hi.end(), p.chunks.begin(), p.chunks.end());
        hi.insert(hi.end(), p.cco.begin(), p.cco.end());
        std::vector<double> hd(p.pw);
        hd.insert(hd.end(), p.inv_w.begin(), p.inv_w.end());
        hd.resize(hd.size() + (size_t)h.ncomp + (size_t)h.nchunk, 0.0); // umean, upart
        if (h.uidx.alloc(std::max<size_t>(1, hi.size())) != hipSuccess || h.ubuf.alloc(std::max<size_t>(1, hd.size())) != hipSuccess)
            return mg_fail(MG_OOM);
        const size_t nu = p.plist.size();
        h.ucomp = h.uidx; h.plist = h.ucomp + nu; h.chunks = h.plist + nu; h.cco = h.chunks + p.chunks.size();
        h.pw = h.ubuf; h.inv_w = h.pw + nu; h.umean = h.inv_w + h.ncomp; h.upart = h.umean + h.ncomp;
        if (hipMemcpy(h.uidx, hi.data(), hi.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h.ubuf, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return mg_fail(MG_BUILD);
    }
    h.w0 = carve_vectors(h.vec.get(), h.lev, 3);
    h.ph = h.w0 + 3 * nCd + c->ghost;
    h.sh = h.ph + nf;
    // the Galerkin levels, finest first, on the device
    for (int l = 1; l < L; ++l) {
        const AvLevel &P = h.lev[(size_t)l - 1];
        AvLevel &Q = h.lev[(size_t)l];
        const double scale = 1.0 / (2.0 * P.f[0] * P.f[1] * P.f[2]);
        hipStream_t s = c->stream;
        MG_LAUNCH(k_avmg_galerkin, blocks_of(Q.op.n), 256, P.op, Q.op, P.f[0], P.f[1], P.f[2], scale, Q.bands);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return mg_fail(MG_BUILD);
    return 0;
}

// Level 0 over a matrix from ec3d_set_matrix_csr that the caller called a 7-point operator on an sdx x sdy x sdz box
// (ec3d_set_precond_grid): the matrix is checked where it lies, on the device and in its stored form, and op0 becomes a
// view of the handle's dictionary form -- as op_of makes it for an assembled matrix -- when that has exactly the seven
// offsets and a table the smoothers' LDS holds, else seven band streams gathered once into bands0.
static int csr_level0(ec3d_ctx *c, int sdx, int sdy, int sdz, MgOp &op0, DevBuf<double> &bands0)
{
    const DevMatrix &A = c->A;
    const char *const who = "ec3d_set_preconditioner: ";
    if (A.sav)
        return mg_refuse(std::string(who) + "the matrix was recognised as the structured A-V form, which is no "
                         "single-component operator on the box of ec3d_set_precond_grid");
    const int64_t kdz = (int64_t)sdx * sdy;
    const int64_t want[7] = {-kdz, -(int64_t)sdx, -1, 0, 1, sdx, kdz};
    MgSrc S{};
    S.bands = A.ncls > 0 ? nullptr : A.bands.get();
    S.cls = A.ncls > 0 ? A.cls.get() : nullptr;
    S.table = A.table;
    S.tail_id = A.ntail > 0 ? A.tail_id.get() : nullptr;
    S.nb = A.nb;
    S.sdx = sdx; S.sdy = sdy;
    S.n = A.n; S.n_pad = A.n_pad; S.kdz = kdz;
    for (int q = 0; q < 7; ++q) S.band[q] = -1;
    int stray = -1; // a band whose offset is not the box's
    for (int b = 0; b < A.nb; ++b) {
        S.slot[b] = -1;
        for (int q = 0; q < 7; ++q)
            if (A.off[b] == want[q]) S.slot[b] = q;
        if (S.slot[b] >= 0) S.band[S.slot[b]] = b;
        else if (stray < 0) stray = b;
    }
    DevBuf<unsigned long long> found;
    unsigned long long res[2] = {0ull, ~0ull};
    if (found.alloc(2) != hipSuccess) return mg_fail(MG_OOM);
    if (hipMemcpyAsync(found, res, sizeof res, hipMemcpyHostToDevice, c->stream) != hipSuccess) return mg_fail(MG_BUILD);
    k_mg_check_grid<<<blocks_of(S.n), 256, 0, c->stream>>>(S, found);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(res, found, sizeof res, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return mg_fail(MG_BUILD);
    const std::string box = std::to_string(sdx) + "x" + std::to_string(sdy) + "x" + std::to_string(sdz);
    if (res[0]) {
        const std::string row = "row " + std::to_string(res[1] / 4 + 1) + " (1-based, the first such row) ";
        switch ((int)(res[1] & 3)) {
        case MG_BAD_TAIL:
            return mg_refuse(who + row + "has entries outside the matrix's bands (" + std::to_string(A.ntail) +
                             " rows with a tail): not a 7-point operator on the " + box + " box");
        case MG_BAD_OFFSET:
            return mg_refuse(who + row + "has an entry at a column offset that is none of 0, +-1, +-" + std::to_string(sdx) +
                             ", +-" + std::to_string(kdz) + ", the offsets of the " + box + " box");
        case MG_BAD_WRAP:
            return mg_refuse(who + row + "couples to a cell across an x or y face of the " + box +
                             " box (a nonzero coefficient where the neighbour lies beyond the box)");
        default:
            return mg_refuse(who + row + "has a zero or non-finite diagonal");
        }
    }
    if (stray >= 0) // (every coefficient of it is zero: no row names it)
        return mg_refuse(std::string(who) + "the matrix has a band at column offset " + std::to_string(A.off[stray]) +
                         ", none of the offsets of the " + box + " box (row 1 on)");
    bool seven = A.nb == 7;
    for (int b = 0; seven && b < 7; ++b) seven = S.slot[b] == b;
    if (A.ncls > 0 && A.ncls <= EC3D_MG_MAXCLS && seven) {
        op0 = op_of(A, sdx, sdy, sdz);
        return 0;
    }
    if (bands0.alloc((size_t)7 * A.n_pad) != hipSuccess) return mg_fail(MG_OOM);
    k_mg_gather<<<blocks_of(A.n_pad), 256, 0, c->stream>>>(S, bands0);
    if (hipGetLastError() != hipSuccess) return mg_fail(MG_BUILD);
    op0 = MgOp{};
    op0.sdx = sdx; op0.sdy = sdy; op0.sdz = sdz;
    op0.n = A.n; op0.n_pad = A.n_pad; op0.kdz = kdz;
    op0.bands = bands0;
    return 0;
}

// T: the precision of the cycle (float: EC3D_PRECOND_FP32)
template <class T> static int set_poisson_mg(ec3d_ctx *c, ec3d_mg &m)
{
    constexpr bool F32 = std::is_same_v<T, float>;
    // a matrix from ec3d_set_matrix_csr whose box the caller named: the hierarchy is made from the matrix alone
    const bool csr = c->from_csr && c->precond_grid[0] > 0;
    if (!(c->poisson_full || csr) || !ec3d_own_handle(c))
        return mg_refuse("ec3d_set_preconditioner: the multigrid preconditioner needs a matrix from ec3d_assemble_poisson "
                         "on a handle of its own (not A-V, CSR, a slab or a handle of ec3d_multi)");
    const int sdx0 = csr ? c->precond_grid[0] : c->sdx, sdy0 = csr ? c->precond_grid[1] : c->sdy,
              sdz0 = csr ? c->precond_grid[2] : c->sdz;
    MgPlan plan;
    const std::vector<std::array<int, 3>> &dims = plan.dims;
    if (csr) {
        ec3d_mg_plan_matrix(sdx0, sdy0, sdz0, EC3D_MG_COARSE_ROWS, plan);
        m.coarsening = EC3D_COARSEN_AGGREGATE; // whatever the handle's setting says
    } else if (!ec3d_mg_plan(sdx0, sdy0, sdz0, c->precond_coarsening == EC3D_COARSEN_AGGREGATE, EC3D_MG_COARSE_ROWS, plan)) {
        const auto d = dims.back();
        return mg_refuse("ec3d_set_preconditioner: no axis of the " + std::to_string(d[0]) + "x" + std::to_string(d[1]) +
                         "x" + std::to_string(d[2]) + " level halves (even and >= 8) and it has more than " +
                         std::to_string(EC3D_MG_COARSE_ROWS) + " rows, the coarse solver's cap", EC3D_PRECOND_E_COARSE);
    }
    if (!csr && c->A.ncls > EC3D_MG_MAXCLS)
        return mg_refuse("ec3d_set_preconditioner: more dictionary classes than the smoother's table holds");
    PoissonMg<T> &h = m.h.emplace<PoissonMg<T>>();
    const int L = (int)dims.size();
    h.grid.resize((size_t)L);
    h.lev.resize((size_t)L);
    std::vector<MgOp> op((size_t)L); // every level in fp64, as assembled
    if (csr) {
        const int rc = csr_level0(c, sdx0, sdy0, sdz0, h.op0, h.bands0);
        if (rc) return rc;
        op[0] = h.op0;
    } else {
        op[0] = h.op0 = op_of(c->A, c->sdx, c->sdy, c->sdz);
    }
    for (int a = 0; a < 3; ++a) h.grid[0].delta[a] = c->poisson_delta[a];
    int64_t coarse_len = 0;
    for (int l = 1; l < L; ++l) {
        MgGrid &P = h.grid[(size_t)l - 1], &Q = h.grid[(size_t)l];
        const auto &d = dims[(size_t)l];
        for (int a = 0; a < 3; ++a) {
            P.f[a] = d[a] == dims[(size_t)l - 1][a] ? 1 : 2; // halved, exactly or (aggregate rule) rounding up
            Q.delta[a] = P.delta[a] * P.f[a];
        }
        Q.kind = plan.kinds[(size_t)l];
        MgOp &o = op[(size_t)l];
        if (Q.kind == EC3D_MG_LEVEL_REDISCRETIZED) {
            const int rc = ec3d_assemble_poisson_level(c, Q.A, d[0], d[1], d[2], c->poisson_bnd, Q.delta);
            if (rc) return rc;
            o = op_of(Q.A, d[0], d[1], d[2]);
        } else {
            // the Galerkin product of the level above, which the stream has completed or holds ahead of this launch
            o = MgOp{};
            o.sdx = d[0]; o.sdy = d[1]; o.sdz = d[2];
            o.kdz = (int64_t)d[0] * d[1];
            o.n = o.kdz * d[2];
            o.n_pad = pad64(o.n);
            if (Q.bands.alloc((size_t)7 * o.n_pad) != hipSuccess) return mg_fail(MG_OOM);
            if (hipMemsetAsync(Q.bands, 0, (size_t)7 * o.n_pad * sizeof(double), c->stream) != hipSuccess)
                return mg_fail("hipMemsetAsync failed");
            o.bands = Q.bands;
            const MgOp &F = op[(size_t)l - 1];
            const double scale = 1.0 / (2.0 * P.f[0] * P.f[1] * P.f[2]);
            hipStream_t s = c->stream;
            MG_LAUNCH(k_mg_galerkin, blocks_of(o.n), 256, F, o, P.f[0], P.f[1], P.f[2], scale, Q.bands);
            if (hipGetLastError() != hipSuccess) return mg_fail(MG_BUILD);
        }
        coarse_len += 3 * pad64(o.n);
    }
    const int64_t nf = pad64(c->A.n);
    // double: the fine w, p^, s^; float: those and the fine right-hand side's copy
    const int64_t total = coarse_len + (F32 ? 4 : 3) * nf;
    if (h.vec.alloc((size_t)total) != hipSuccess || m.part.alloc(2 * EC3D_MG_DOT_BLOCKS) != hipSuccess ||
        m.scal.alloc(1) != hipSuccess)
        return mg_fail(MG_OOM);
    if (hipMemsetAsync(h.vec, 0, (size_t)total * sizeof(T), c->stream) != hipSuccess ||
        hipMemsetAsync(m.scal, 0, sizeof(MgScalars), c->stream) != hipSuccess)
        return mg_fail("hipMemsetAsync failed");
    if constexpr (F32) {
        // the class table, or (level 0 in band form, a Galerkin level) the seven streams; a rediscretised level's A keeps
        // owning the class bytes
        h.coef.resize((size_t)L);
        for (int l = 0; l < L; ++l) {
            const MgOp &D = op[(size_t)l];
            DevBuf<float> &coef = h.coef[(size_t)l];
            const bool dict = D.cls != nullptr;
            const int64_t len = dict ? (int64_t)D.ncls * 7 : 7 * D.n_pad;
            if (coef.alloc((size_t)len) != hipSuccess) return mg_fail(MG_OOM);
            k_mg_narrow<<<blocks_of(len), 256, 0, c->stream>>>(len, dict ? D.table : D.bands, coef);
            h.lev[(size_t)l].op = MgOp32{D.sdx, D.sdy, D.sdz, D.n, D.n_pad, D.kdz, D.cls, dict ? coef.get() : nullptr,
                                         D.ncls, dict ? nullptr : coef.get()};
        }
        if (hipGetLastError() != hipSuccess) return mg_fail(MG_BUILD);
    } else {
        for (int l = 0; l < L; ++l) h.lev[(size_t)l].op = op[(size_t)l];
    }
    T *q = h.w0 = carve_vectors(h.vec.get(), h.lev, 1);
    if constexpr (F32) h.b0 = q += nf;
    h.ph = q + nf;
    h.sh = q + 2 * nf;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return mg_fail(MG_BUILD);
    if constexpr (F32)
        for (MgGrid &G : h.grid) G.bands.reset(); // narrowed: an fp32 hierarchy keeps no fp64 coefficients of its own
    return 0;
}

// ---- N, the preconditioner of the null projection's adjoint solves (ec3d_set_null_precond) -------
// A hierarchy of its own, built inside the null set-up (or for one ec3d_null_precond_apply) and released by the caller
// before it returns: c->mg, the caller's preconditioner, is neither read nor written.
int ec3d_null_mg_build(ec3d_ctx *c, int kind, int pre, int post, int coarse, ec3d_mg **out)
{
    *out = nullptr;
    std::unique_ptr<ec3d_mg> m(new ec3d_mg);
    m->kind = EC3D_PRECOND_BLOCK_MG;
    m->coarsening = EC3D_COARSEN_AGGREGATE;
    m->pre = pre ? pre : 2;
    m->post = post ? post : 2;
    m->coarse = coarse ? coarse : 16;
    const int rc = set_block_mg(c, *m, kind);
    if (rc == EC3D_PRECOND_E_MATRIX) // the block hierarchy's refusal, under the name of the setting that asked for it
        ec3d_set_error(std::string("ec3d_set_null_precond: the block hierarchy refuses this matrix -- ") + ec3d_last_error());
    if (rc) return rc;
    *out = m.release();
    return 0;
}

void ec3d_null_mg_delete(ec3d_mg *m) { delete m; }

void ec3d_null_mg_dims(const ec3d_mg *m, int32_t *levels, int32_t *dims)
{
    const BlockMg &h = std::get<BlockMg>(m->h);
    const size_t L = std::min<size_t>(h.lev.size(), EC3D_NULL_PRECOND_MAX_LEVELS);
    *levels = (int32_t)L;
    for (size_t l = 0; l < L; ++l) {
        dims[3 * l] = h.lev[l].op.sdx;
        dims[3 * l + 1] = h.lev[l].op.sdy;
        dims[3 * l + 2] = h.lev[l].op.sdz;
    }
}

void ec3d_adjoint_iteration(ec3d_ctx *c, const ec3d_mg *m, const OuterRun &k, int it)
{
    const BlockMg *h = m ? &std::get<BlockMg>(m->h) : nullptr;
    hipStream_t s = c->stream;
    const MatView V = c->A.view();
    OuterRun o = k;
    if (h) o.ph = h->ph, o.sh = h->sh;
    ec3d_outer_iteration(
        c, o, it, false, [&](Gate g, const double *r, void *z) { if (h) launch_cycle(*m, *h, g, r, (double *)z, s); },
        [&](Gate, const void *x, const double *, double *y, int) { ec3d_launch_spmv_t(V, k.n, (const double *)x, y, s); });
}

void ec3d_mg_free(ec3d_ctx *c)
{
    delete c->mg; // (its levels' matrices and every buffer of the hierarchy with it)
    c->mg = nullptr;
}

extern "C" int ec3d_set_precond_grid(ec3d_handle c, int32_t sdx, int32_t sdy, int32_t sdz)
{
    const char *why = nullptr;
    if (c && sdx == 0 && sdy == 0 && sdz == 0) { // no grid: what a new matrix leaves, for a caller that takes its word back
        c->precond_grid[0] = c->precond_grid[1] = c->precond_grid[2] = 0;
        return 0;
    }
    if (!c) why = "null handle";
    else if (!c->have_matrix || !c->from_csr) why = "the handle holds no matrix from ec3d_set_matrix_csr";
    else if (!ec3d_own_handle(c)) why = "not on a slab or a handle of ec3d_multi";
    else if (sdx < 2 || sdy < 2 || sdz < 2) why = "every extent must be >= 2";
    else if ((int64_t)sdx * sdy * sdz != c->n_ref) why = "sdx * sdy * sdz is not the matrix's n";
    if (why) {
        ec3d_set_error(std::string("ec3d_set_precond_grid: ") + why);
        return 2;
    }
    c->precond_grid[0] = sdx; c->precond_grid[1] = sdy; c->precond_grid[2] = sdz;
    return 0;
}

extern "C" int ec3d_get_precond_grid(ec3d_handle c, int32_t *dims)
{
    if (!c) {
        ec3d_set_error("ec3d_get_precond_grid: null handle");
        return 2;
    }
    for (int a = 0; dims && a < 3; ++a) dims[a] = c->precond_grid[a];
    return 0;
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
    if ((kind != EC3D_PRECOND_MG && kind != EC3D_PRECOND_BLOCK_MG) || pre < 0 || post < 0 || coarse_sweeps < 0) {
        ec3d_set_error("ec3d_set_preconditioner: unknown kind or negative sweep count");
        return 2;
    }
    int rc = ec3d_need_matrix(c, "ec3d_set_preconditioner");
    if (rc) return rc;
    const bool f32 = c->precond_precision == EC3D_PRECOND_FP32;
    if (kind == EC3D_PRECOND_BLOCK_MG && f32)
        return mg_refuse("ec3d_set_preconditioner: the fp32 V-cycle (ec3d_set_precond_precision) is available for "
                         "EC3D_PRECOND_MG only, not for the block multigrid of the A-V form");
    // build the new hierarchy completely before the old one is replaced: a failure leaves the handle as it was
    std::unique_ptr<ec3d_mg> m(new ec3d_mg);
    m->kind = kind;
    m->precision = c->precond_precision;
    m->coarsening = kind == EC3D_PRECOND_BLOCK_MG ? EC3D_COARSEN_AGGREGATE : c->precond_coarsening;
    m->pre = pre ? pre : 2; // 0: the default
    m->post = post ? post : 2;
    m->coarse = coarse_sweeps ? coarse_sweeps : 16;
    rc = kind == EC3D_PRECOND_BLOCK_MG ? set_block_mg(c, *m) : f32 ? set_poisson_mg<float>(c, *m) : set_poisson_mg<double>(c, *m);
    if (rc) return rc;
    ec3d_mg_free(c);
    c->mg = m.release();
    return 0;
}

extern "C" int ec3d_get_preconditioner(ec3d_handle c, int *kind, int32_t *levels, int32_t *dims)
{
    if (!c) {
        ec3d_set_error("ec3d_get_preconditioner: null handle");
        return 2;
    }
    if (kind) *kind = c->mg ? c->mg->kind : EC3D_PRECOND_NONE;
    if (levels) *levels = 0;
    if (c->mg)
        std::visit([&](const auto &h) {
            if (levels) *levels = (int32_t)h.lev.size();
            for (size_t l = 0; dims && l < h.lev.size(); ++l) {
                dims[3 * l] = h.lev[l].op.sdx;
                dims[3 * l + 1] = h.lev[l].op.sdy;
                dims[3 * l + 2] = h.lev[l].op.sdz;
            }
        }, c->mg->h);
    return 0;
}

extern "C" int ec3d_set_precond_precision(ec3d_handle c, int32_t precision)
{
    if (!c || (precision != EC3D_PRECOND_FP64 && precision != EC3D_PRECOND_FP32)) {
        ec3d_set_error(!c ? std::string("ec3d_set_precond_precision: null handle")
                          : "ec3d_set_precond_precision: unknown precision " + std::to_string(precision) +
                                " (EC3D_PRECOND_FP64 = 0, EC3D_PRECOND_FP32 = 1)");
        return 2;
    }
    c->precond_precision = precision;
    return 0;
}

extern "C" int ec3d_get_precond_precision(ec3d_handle c, int32_t *setting, int32_t *in_use)
{
    if (!c) {
        ec3d_set_error("ec3d_get_precond_precision: null handle");
        return 2;
    }
    if (setting) *setting = c->precond_precision;
    if (in_use) *in_use = c->mg ? c->mg->precision : EC3D_PRECOND_FP64;
    return 0;
}

template <class T> static int level_kind(const PoissonMg<T> &h, size_t l) { return h.grid[l].kind; }
static int level_kind(const BlockMg &, size_t l) { return l ? EC3D_MG_LEVEL_GALERKIN : EC3D_MG_LEVEL_MATRIX; }

extern "C" int ec3d_set_precond_coarsening(ec3d_handle c, int32_t rule)
{
    if (!c || (rule != EC3D_COARSEN_REDISCRETIZE && rule != EC3D_COARSEN_AGGREGATE)) {
        ec3d_set_error(!c ? std::string("ec3d_set_precond_coarsening: null handle")
                          : "ec3d_set_precond_coarsening: unknown rule " + std::to_string(rule) +
                                " (EC3D_COARSEN_REDISCRETIZE = 0, EC3D_COARSEN_AGGREGATE = 1)");
        return 2;
    }
    c->precond_coarsening = rule;
    return 0;
}

extern "C" int ec3d_get_precond_coarsening(ec3d_handle c, int32_t *setting, int32_t *in_use, int32_t *level_kinds)
{
    if (!c) {
        ec3d_set_error("ec3d_get_precond_coarsening: null handle");
        return 2;
    }
    if (setting) *setting = c->precond_coarsening;
    if (in_use) *in_use = c->mg ? c->mg->coarsening : EC3D_COARSEN_REDISCRETIZE;
    if (c->mg && level_kinds)
        std::visit([&](const auto &h) {
            for (size_t l = 0; l < h.lev.size(); ++l) level_kinds[l] = level_kind(h, l);
        }, c->mg->h);
    return 0;
}

// z = M r: r up into `in`, the cycle that `launch` enqueues from `in` into `out`, z down from `out`
template <class F> static int precond_apply_through(ec3d_ctx *c, double *in, double *out, const double *r, double *z, const F &launch)
{
    int rc;
    if ((rc = ec3d_vec_h2d(c, in, r))) return rc;
    launch();
    EC3D_HIP(hipGetLastError());
    if ((rc = ec3d_vec_d2h(c, z, out))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
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
    const ec3d_mg &m = *c->mg;
    const Gate g{nullptr, 0, 0};
    hipStream_t s = c->stream;
    if (auto *h = std::get_if<PoissonMg<float>>(&m.h)) {
        // r and z in fp64 through the work vectors P and AP (as ec3d_spmv); the cycle narrows r, z is widened exactly
        double *in = c->vec[EC3D_VEC_P], *out = c->vec[EC3D_VEC_AP];
        return precond_apply_through(c, in, out, r, z, [&] {
            launch_cycle(m, *h, g, in, h->sh, s);
            k_mg_widen<<<blocks_of(c->A.n), 256, 0, s>>>(c->A.n, h->sh, out);
        });
    }
    if (auto *h = std::get_if<PoissonMg<double>>(&m.h))
        return precond_apply_through(c, h->ph, h->sh, r, z, [&] { launch_cycle(m, *h, g, h->ph, h->sh, s); });
    const BlockMg &h = std::get<BlockMg>(m.h);
    return precond_apply_through(c, h.ph, h.sh, r, z, [&] { launch_cycle(m, h, g, h.ph, h.sh, s); });
}

extern "C" int ec3d_null_precond_apply(ec3d_handle c, const double *r, double *z)
{
    int rc = ec3d_need_matrix(c, "ec3d_null_precond_apply");
    if (rc) return rc;
    if ((rc = ec3d_null_eligible(c, "ec3d_null_precond_apply", true))) return rc;
    const NullProjection &N = c->nullp;
    if (N.precond == EC3D_NULL_PRECOND_NONE || !r || !z) {
        ec3d_set_error("ec3d_null_precond_apply: no preconditioner of the adjoint solve set (ec3d_set_null_precond), or a "
                       "null vector");
        return N.precond == EC3D_NULL_PRECOND_NONE ? 3 : 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    ec3d_mg *built = nullptr;
    if ((rc = ec3d_null_mg_build(c, N.precond, N.pre, N.post, N.coarse, &built))) return rc;
    const std::unique_ptr<ec3d_mg> m(built); // N lives for this call only
    const BlockMg &h = std::get<BlockMg>(m->h);
    hipStream_t s = c->stream;
    return precond_apply_through(c, h.ph, h.sh, r, z, [&] { launch_cycle(*m, h, Gate{nullptr, 0, 0}, h.ph, h.sh, s); });
}

// iterations per poll of solve_core: about 1 ms of device work.  Poisson: a V-cycle is ~210 B per fine row, two per
// iteration.  A-V, per A cell: two applications of M (three V-cycles of ~210 B each) ~1260 B, two SpMVs of the four
// blocks and the vector kernels ~800 B; the launches of a level cost ~60 us per application on small grids
int ec3d_mg_chunk(const ec3d_ctx *c)
{
    const auto *av = std::get_if<BlockMg>(&c->mg->h);
    const double levels = std::visit([](const auto &h) { return (double)h.lev.size(); }, c->mg->h);
    const double est_us = av ? (double)av->lev[0].op.n * 2100.0 / 4.0e6 + 120.0 * levels
                             : (double)c->A.n_pad * 600.0 / 4.0e6 + 60.0 * levels;
    return (int)std::min<double>(16.0, std::max<double>(1.0, 1000.0 / est_us));
}

// The run of a solve (ec3d_outer.hpp): the handle's work vectors, v in AP and t in AS, with the hierarchy's p^ and s^
// and the history the caller asked for.
static OuterRun solve_run(ec3d_ctx *c, int64_t n, void *ph, void *sh, bool f32)
{
    double **v = c->vec;
    return OuterRun{n, v[EC3D_VEC_X], v[EC3D_VEC_R], v[EC3D_VEC_R0], v[EC3D_VEC_P], v[EC3D_VEC_AP], v[EC3D_VEC_S],
                    v[EC3D_VEC_AS], ph, sh, f32, c->mg->part, c->mg->scal, c->hist, c->hist_cap};
}

// The single-component operator.  T: the precision of M and of p^, s^, which the SpMV + dot launch and the x / r update
// widen on load.  The product's launch sums its dot partials itself.
template <class T> static void launch_iteration_of(ec3d_ctx *c, int it, const PoissonMg<T> &h)
{
    const ec3d_mg *m = c->mg;
    hipStream_t s = c->stream;
    const MgOp &A = h.op0;
    const OuterRun k = solve_run(c, A.n, h.ph, h.sh, std::is_same_v<T, float>);
    ec3d_outer_iteration(
        c, k, it, true, [&](Gate g, const double *r, void *z) { launch_cycle(*m, h, g, r, (T *)z, s); },
        [&](Gate g, const void *x, const double *a, double *y, int two) {
            MG_LAUNCH(k_mg_spmv_dot, dot_blocks(A.n), 256, A, g, (const T *)x, a, y, two, k.part);
        });
}

// The structured A-V form: M the block multigrid, v = A p^ and t = A s^ by the format's own SpMV (ec3d_launch_spmv)
static void launch_iteration_of(ec3d_ctx *c, int it, const BlockMg &h)
{
    const ec3d_mg *m = c->mg;
    hipStream_t s = c->stream;
    const MatView V = c->A.view();
    ec3d_outer_iteration(
        c, solve_run(c, c->A.n, h.ph, h.sh, false), it, false,
        [&](Gate g, const double *r, void *z) { launch_cycle(*m, h, g, r, (double *)z, s); },
        [&](Gate, const void *x, const double *, double *y, int) { ec3d_launch_spmv(V, c->sweep_s, (const double *)x, y, s); });
}

void ec3d_mg_launch_iteration(ec3d_ctx *c, int it)
{
    const ec3d_mg &m = *c->mg;
    if (auto *h = std::get_if<PoissonMg<float>>(&m.h)) launch_iteration_of(c, it, *h);
    else if (auto *h = std::get_if<PoissonMg<double>>(&m.h)) launch_iteration_of(c, it, *h);
    else launch_iteration_of(c, it, std::get<BlockMg>(m.h));
}
