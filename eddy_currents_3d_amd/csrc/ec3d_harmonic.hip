// ec3d_harmonic.hip — the time-harmonic A-V solve (K + j omega M) x^ = b^: complex BiCGSTAB with restart on the
// structured form (ec3d_harmonic_*).
//
// Operator.  The class bytes of the real matrix with two tables of their own, made at ec3d_assemble
// (k_build_table_harmonic): re, the transient table without its dt terms, and m, the unit imaginary part;
// a set-up interleaves (re, omega * m) into one table of 16 pairs per class, which k_hb_spmv holds in LDS.
//
// Vectors.  Eight complex vectors of n_pad interleaved (re, im) pairs in device numbering, no ghosts: a row's class is
// tested before a neighbour is read, as in ec3d_transpose.hip.  A row is one 16-byte access.
//
// Arithmetic (-ffp-contract=off; tests/harmonic_numpy.py restates every line).  a x = (ar xr - ai xi, ar xi + ai xr),
// every product and sum rounded on its own.  A row adds its terms from +0.0 in ascending column -- an A row its bands,
// then its U couplings; a U row its A couplings, then its bands -- and a term whose two coefficients are 0 is neither
// formed nor added.  <a, b> = sum conj(a) b, row term (ar br + ai bi, ar bi - ai br); a / b with d = br br + bi bi.
//
// Sums and launches: the streaming idiom of ec3d_stream.hpp on chunks of EC3D_TILE rows, G = ec3d_stream_wgs(n_pad)
// workgroups, workgroup w the chunks w, w + G, ...; thread t owns rows t and t + 256 of a chunk (consecutive lanes,
// consecutive 16-byte pairs) and adds row t's term, then row t + 256's.  Rows >= n enter every sum as +0.0 and are never
// stored.  Every workgroup leaves one partial per sum; the NEXT kernel's workgroups each collapse them
// (stream_strided_sum, stream_block_sum) and compute the scalars redundantly -- identical bits in every workgroup --
// and workgroup 0 records them.  No float atomics.
//
// Systems.  Everything below is written once, for S systems (omega_s, b^_s, x^_s) on the one matrix
// in lock step: the kernels of the iteration run on a grid of (G, S) and blockIdx.y names the system, whose state,
// partials, table and vectors stand s strides behind system 0's.  h_leave and h_collapse index with gridDim.x and
// blockIdx.x only, so a system's bits depend on neither S nor s.  The single solve (ec3d_harmonic_setup) is S = 1 in
// storage of its own; a batch (ec3d_harmonic_batch_*) holds up to EC3D_HARMONIC_MAX_BATCH.  The host describes the
// systems of a run in an HRun, which every launch_* takes.
//
// Iteration `it` (src/solvers.f90:29-49), five launches:
//   k_hb_spmv<1>  AP = A P, <R0, AP>
//   k_hb_s        alpha = rr0 / <R0, AP>;  S = R - alpha AP, ||S||^2
//   k_hb_spmv<2>  AS = A S, <AS, S>, <AS, AS>
//   k_hb_xr       ||S|| exit: X = X + alpha P.  Else omega = <AS, S> / <AS, AS>; X = (X + alpha P) + omega S;
//                 R = S - omega AS, ||R||^2, <R0, R>
//   k_hb_p        ||R|| exit.  Else beta = (alpha / omega) rr0_new / rr0; restart (R0 = R, P = R, rr0 = ||R||^2) when
//                 |rr0_new| / ||b^|| < tol, else P = R + beta (P - omega AP), rr0 = rr0_new
// The exit words stay on the device: stop_s is written by k_hb_xr only, stop_r by k_hb_p (and k_hb_setup) only, and a
// kernel never tests at its entry a word that its own launch may write with a value that would change the test --
// k_hb_xr of iteration it asks stop_s < it, k_hb_p stop_r < it -- so a workgroup that starts late takes the same path as
// workgroup 0.  rr0 alternates between two slots for the same reason.  The host enqueues 16 iterations and copies the S
// states back once (run_iterations), on while any system runs; a stopped system's workgroups return at their first load.
//
// Left null vectors (opt-in, ec3d_harmonic_set_null_projection and ec3d_harmonic_batch_set_null_projection; DESIGN
// sections 18a, 18c).  K + j omega M is singular as the transient matrix is: one left null vector per connected
// conducting component, and every residual keeps w^H r = w^H b^.  The set-up (null_build) finds one set of vectors per
// distinct omega by adjoint solves in lock step -- the iteration above around k_hb_spmv_h, y = A^H x, and k_hb_xr_at --
// and a solve with the setting on takes every system's own vectors out of its initial residual between k_hb_spmv<3> and
// k_hb_setup (launch_project: k_hbn_dots, k_hbn_collapse, k_hbn_sub).  tests/harmonic_null_numpy.py restates every line.
#include "ec3d_stream.hpp"

#include <chrono>
#include <cmath>
#include <cstring>

enum { HP_BB = 0, HP_RR, HP_RR0R, HP_RR0I, HP_D1R, HP_D1I, HP_SS, HP_D2R, HP_D2I, HP_D3, HP_NSLOT };

struct HarmonicState {
    double rr0[2][2]; // <R0, R> entering iteration it: rr0[it & 1]
    double alpha[2], omega[2];
    double bnorm, tol;
    double rnorm, snorm; // of the last k_hb_p / k_hb_xr that got that far
    int stop_s, stop_r;  // INT_MAX while running; the iteration of the ||S|| / ||R|| exit (stop_r = 0: ||b^|| = 0)
    int restarts, pad_;
};

namespace {

typedef stream_d2 cplx; // .x = re, .y = im
static_assert((55 + 9 * EC3D_SAV_MAXDOM) * 16 * sizeof(cplx) + 256 <= 65536, "k_hb_spmv: the table of pairs fits 64 KB of LDS");

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return cplx{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cdiv(cplx a, cplx b)
{
    const double d = b.x * b.x + b.y * b.y;
    return cplx{(a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d};
}
// the row term of <a, b> and of a norm
__device__ __forceinline__ cplx cdot(cplx a, cplx b) { return cplx{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double cabs2(cplx a) { return a.x * a.x + a.y * a.y; }

__device__ __forceinline__ int64_t h_row(int64_t ch, int half) { return ch * EC3D_TILE + half * EC3D_THREADS + threadIdx.x; }
__device__ __forceinline__ cplx h_load(const cplx *p, int64_t r, int64_t n) { return r < n ? p[r] : cplx{0.0, 0.0}; }

// NV sums, slot0 .. slot0 + NV - 1 of `part` (G partials each), in every thread
template <int NV> __device__ __forceinline__ void h_collapse(double (&v)[NV], const double *part, int slot0, int G, double *lds)
{
    stream_strided_sum<NV>(v, part + (int64_t)slot0 * G, G, G);
    stream_block_sum<NV>(v, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < NV; ++k) lds[k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; ++k) v[k] = lds[k];
    __syncthreads();
}
template <int NV> __device__ __forceinline__ void h_leave(double (&v)[NV], double *part, int slot0, double *lds)
{
    stream_block_sum<NV>(v, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < NV; ++k) part[(int64_t)(slot0 + k) * gridDim.x + blockIdx.x] = v[k];
}

struct HSav {
    const uint8_t *cls;
    const cplx *table;
    int ncls, a0, u0, zero;
    int64_t n, nC, off[7], step[3];
};

__device__ __forceinline__ void h_term(cplx &s, cplx t, const cplx *__restrict__ x, int64_t j, int64_t n)
{
    if (t.x == 0.0 && t.y == 0.0) return;
    if (j < 0 || j >= n) return; // (no table of ec3d_assemble points outside the box)
    const cplx p = cmul(t, x[j]);
    s.x = s.x + p.x;
    s.y = s.y + p.y;
}

__device__ __forceinline__ cplx h_row_product(const HSav &A, const cplx *tbl, const cplx *__restrict__ x, int64_t i)
{
    cplx s = {0.0, 0.0};
    const int cc = A.cls[i];
    if (cc >= A.zero) return s;
    const cplx *t = tbl + cc * 16;
    const int blk = (int)(i / A.nC);
    const int64_t q = i - blk * A.nC;
    if (cc < A.u0) {
        for (int b = 0; b < 7; ++b) h_term(s, t[b], x, i + A.off[b], A.n);
        if (cc >= A.a0) {
            const int64_t step = blk == 0 ? A.step[0] : (blk == 1 ? A.step[1] : A.step[2]);
            for (int m = -2; m <= 2; ++m) h_term(s, t[7 + m + 2], x, 3 * A.nC + q + m * step, A.n);
        }
    } else {
        for (int d = 0; d < 3; ++d)
            for (int j = 0; j < 3; ++j) h_term(s, t[7 + 3 * d + j], x, d * A.nC + q + (j - 1) * A.step[d], A.n);
        for (int b = 0; b < 7; ++b) h_term(s, t[b], x, i + A.off[b], A.n);
    }
    return s;
}

// Row j of A^H x: the gather of k_sav_spmv_t (ec3d_transpose.hip) in complex pairs.  Column j of A
// holds band b of row j - off[b]; for an A_d column of cell q the U rows of the cells q - (jj - 1) step_d, slot
// 7 + 3 d + jj; for a U column the A_d rows of the cells q - m step_d, slot 7 + m + 2.  The coefficient stands under the
// SOURCE row's class and is conjugated: conj(a) x = (ar xr + ai xi, ar xi - ai xr).  Terms are added from +0.0 in
// ascending source row -- bands from the largest offset down, shifts from the largest down, the A blocks before the U
// block.  A source row is tested before anything of it is read: inside its block (so inside [0, n)), of a class that
// owns the slot; x is read only where both tests passed and a coefficient is not zero.
__device__ __forceinline__ void h_term_h(cplx &s, cplx t, const cplx *__restrict__ x, int64_t i)
{
    if (t.x == 0.0 && t.y == 0.0) return;
    const cplx v = x[i];
    const cplx p = cplx{t.x * v.x + t.y * v.y, t.x * v.y - t.y * v.x};
    s.x = s.x + p.x;
    s.y = s.y + p.y;
}

__device__ __forceinline__ cplx h_row_product_h(const HSav &A, const cplx *tbl, const cplx *__restrict__ x, int64_t j)
{
    cplx s = {0.0, 0.0};
    if (A.cls[j] >= A.zero) return s; // a row of no unknown: no column of A either
    const int blk = (int)(j / A.nC);
    const int64_t q = j - blk * A.nC;
    const int64_t lo = blk * A.nC, hi = blk < 3 ? lo + A.nC : A.n;
    auto bands = [&]() {
        for (int b = 6; b >= 0; --b) {
            const int64_t i = j - A.off[b];
            if (i < lo || i >= hi) continue;
            const int cc = A.cls[i];
            if (cc >= A.zero) continue;
            h_term_h(s, tbl[cc * 16 + b], x, i);
        }
    };
    if (blk < 3) {
        bands();
        for (int jj = 2; jj >= 0; --jj) { // the U rows that reach this A_d column
            const int64_t cu = q - (jj - 1) * A.step[blk];
            if (cu < 0 || 3 * A.nC + cu >= A.n) continue;
            const int64_t i = 3 * A.nC + cu;
            const int cc = A.cls[i];
            if (cc < A.u0 || cc >= A.zero) continue;
            h_term_h(s, tbl[cc * 16 + 7 + 3 * blk + jj], x, i);
        }
    } else {
        for (int d = 0; d < 3; ++d)
            for (int m = 2; m >= -2; --m) { // the coupled A_d rows that reach this U column
                const int64_t ca = q - m * A.step[d];
                if (ca < 0 || ca >= A.nC) continue;
                const int64_t i = d * A.nC + ca;
                const int cc = A.cls[i];
                if (cc < A.a0 || cc >= A.u0) continue;
                h_term_h(s, tbl[cc * 16 + 7 + m + 2], x, i);
            }
        bands();
    }
    return s;
}

// MODE 0: y = A x.  1: and <o, y> (o = R0).  2: and <y, x>, <y, y> (x = S).  3: r = o - y (o = B^), r0 = p = r,
// ||o||^2 and ||r||^2: y, r0, p are the three outputs.  ADJ: A^H in place of A.  table: the operator's pairs (A.table of
// a single solve, the system's own in a batch)
template <int MODE, bool ADJ>
__device__ __forceinline__ void h_spmv_modes(const HSav &A, const cplx *__restrict__ table, const HarmonicState *st,
                                             const cplx *__restrict__ x, const cplx *__restrict__ o,
                                             cplx *__restrict__ y, cplx *__restrict__ r0, cplx *__restrict__ p,
                                             int64_t nchunk, double *__restrict__ part, cplx *tbl, double *lds)
{
    if ((MODE == 1 || MODE == 2) && (st->stop_s != INT_MAX || st->stop_r != INT_MAX)) return;
    for (int q = threadIdx.x; q < A.ncls * 16; q += EC3D_THREADS) tbl[q] = table[q];
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= A.n) continue;
            const cplx s = ADJ ? h_row_product_h(A, tbl, x, i) : h_row_product(A, tbl, x, i);
            if (MODE == 0) y[i] = s;
            if (MODE == 1) {
                y[i] = s;
                const cplx d = cdot(o[i], s);
                acc[0] = acc[0] + d.x;
                acc[1] = acc[1] + d.y;
            }
            if (MODE == 2) {
                y[i] = s;
                const cplx d = cdot(s, x[i]);
                acc[0] = acc[0] + d.x;
                acc[1] = acc[1] + d.y;
                acc[2] = acc[2] + cabs2(s);
            }
            if (MODE == 3) {
                const cplx b = o[i], r = cplx{b.x - s.x, b.y - s.y};
                y[i] = r;
                r0[i] = r;
                p[i] = r;
                acc[0] = acc[0] + cabs2(b);
                acc[1] = acc[1] + cabs2(r);
            }
        }
    if (MODE == 1) {
        double v[2] = {acc[0], acc[1]};
        h_leave<2>(v, part, HP_D1R, lds);
    }
    if (MODE == 2) h_leave<3>(acc, part, HP_D2R, lds);
    if (MODE == 3) {
        double v[2] = {acc[0], acc[1]};
        h_leave<2>(v, part, HP_BB, lds);
    }
}

// behind k_hb_spmv<3>, one workgroup: ||b^||, rr0 = <R0, R> = (||R||^2, 0), the exit words
__device__ __forceinline__ void h_setup_body(HarmonicState *st, const double *part, int G, double tol, double *lds)
{
    double v[2];
    h_collapse<2>(v, part, HP_BB, G, lds);
    if (threadIdx.x != 0) return;
    const double bnorm = sqrt(v[0]);
    st->rr0[0][0] = st->rr0[0][1] = 0.0;
    st->rr0[1][0] = v[1];
    st->rr0[1][1] = 0.0;
    st->alpha[0] = st->alpha[1] = st->omega[0] = st->omega[1] = 0.0;
    st->bnorm = bnorm;
    st->tol = tol;
    st->rnorm = sqrt(v[1]);
    st->snorm = 0.0;
    st->stop_s = INT_MAX;
    st->stop_r = bnorm == 0.0 ? 0 : INT_MAX; // src/solvers.f90:23
    st->restarts = 0;
    st->pad_ = 0;
}

__device__ __forceinline__ void h_s_body(HarmonicState *st, int it, const cplx *__restrict__ r,
                                         const cplx *__restrict__ ap, cplx *__restrict__ sv, int64_t n, int64_t nchunk,
                                         double *__restrict__ part, double *lds)
{
    if (st->stop_s != INT_MAX || st->stop_r != INT_MAX) return;
    double d[2];
    h_collapse<2>(d, part, HP_D1R, gridDim.x, lds);
    const cplx alpha = cdiv(cplx{st->rr0[it & 1][0], st->rr0[it & 1][1]}, cplx{d[0], d[1]});
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->alpha[0] = alpha.x;
        st->alpha[1] = alpha.y;
    }
    double acc[1] = {0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx t = cmul(alpha, ap[i]), a = r[i], s = cplx{a.x - t.x, a.y - t.y};
            sv[i] = s;
            acc[0] = acc[0] + cabs2(s);
        }
    h_leave<1>(acc, part, HP_SS, lds);
}

__device__ __forceinline__ void h_xr_body(HarmonicState *st, int it, const cplx *__restrict__ p,
                                          const cplx *__restrict__ sv, const cplx *__restrict__ as,
                                          const cplx *__restrict__ r0, cplx *__restrict__ x, cplx *__restrict__ r,
                                          int64_t n, int64_t nchunk, double *__restrict__ part, double *lds)
{
    if (st->stop_s < it || st->stop_r != INT_MAX) return;
    double v[4]; // ||S||^2, <AS, S>, <AS, AS>
    h_collapse<4>(v, part, HP_SS, gridDim.x, lds);
    const double snorm = sqrt(v[0]);
    const bool exit_s = snorm / st->bnorm < st->tol; // src/solvers.f90:34
    const cplx alpha = {st->alpha[0], st->alpha[1]};
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (exit_s) {
        if (first) {
            st->snorm = snorm;
            st->stop_s = it;
        }
        for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
            for (int half = 0; half < 2; ++half) {
                const int64_t i = h_row(ch, half);
                if (i >= n) continue;
                const cplx t = cmul(alpha, p[i]), a = x[i];
                x[i] = cplx{a.x + t.x, a.y + t.y};
            }
        return;
    }
    const cplx omega = cdiv(cplx{v[1], v[2]}, cplx{v[3], 0.0});
    if (first) {
        st->snorm = snorm;
        st->omega[0] = omega.x;
        st->omega[1] = omega.y;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx s = sv[i], t = cmul(alpha, p[i]), u = cmul(omega, s), w = cmul(omega, as[i]), a = x[i];
            x[i] = cplx{(a.x + t.x) + u.x, (a.y + t.y) + u.y};
            const cplx rn = {s.x - w.x, s.y - w.y};
            r[i] = rn;
            const cplx d = cdot(r0[i], rn);
            acc[0] = acc[0] + cabs2(rn);
            acc[1] = acc[1] + d.x;
            acc[2] = acc[2] + d.y;
        }
    h_leave<3>(acc, part, HP_RR, lds);
}

__device__ __forceinline__ void h_p_body(HarmonicState *st, int it, const cplx *__restrict__ r,
                                         const cplx *__restrict__ ap, cplx *__restrict__ p, cplx *__restrict__ r0,
                                         int64_t n, int64_t nchunk, const double *__restrict__ part, double *lds)
{
    if (st->stop_s != INT_MAX || st->stop_r < it) return;
    double v[3]; // ||R||^2, <R0, R>
    h_collapse<3>(v, part, HP_RR, gridDim.x, lds);
    const double rnorm = sqrt(v[0]), bnorm = st->bnorm, tol = st->tol;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (rnorm / bnorm < tol) { // src/solvers.f90:43
        if (first) {
            st->rnorm = rnorm;
            st->stop_r = it;
        }
        return;
    }
    const cplx alpha = {st->alpha[0], st->alpha[1]}, omega = {st->omega[0], st->omega[1]};
    const cplx rr0n = {v[1], v[2]}, rr0 = {st->rr0[it & 1][0], st->rr0[it & 1][1]};
    const cplx beta = cdiv(cmul(cdiv(alpha, omega), rr0n), rr0);              // :45
    const bool restart = sqrt(rr0n.x * rr0n.x + rr0n.y * rr0n.y) / bnorm < tol; // :47
    if (first) {
        st->rnorm = rnorm;
        st->rr0[(it + 1) & 1][0] = restart ? v[0] : rr0n.x; // after R0 = R the next <R0, R> is ||R||^2
        st->rr0[(it + 1) & 1][1] = restart ? 0.0 : rr0n.y;
        if (restart) st->restarts = st->restarts + 1;
    }
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx a = r[i];
            if (restart) {
                r0[i] = a;
                p[i] = a;
            } else {
                const cplx w = cmul(omega, ap[i]), po = p[i], t = cmul(beta, cplx{po.x - w.x, po.y - w.y});
                p[i] = cplx{a.x + t.x, a.y + t.y};
            }
        }
}

// ---- the kernels of the iteration: S systems in lock step on a grid of (G, S) (DESIGN sections 18, 18b) -------------
// blockIdx.y is the system: its state, partials, table and vectors stand `sys` strides further, and the workgroup then
// runs one of the bodies above.  The single solve is the grid (G, 1).
struct HBatch {
    cplx *vec;            // system s, vector w: vec + (s * HV_N + w) * len
    double *part;         // system s: part + s * HP_NSLOT * gridDim.x
    HarmonicState *state; // system s: state + s
    int64_t len;
};
__device__ __forceinline__ cplx *hb_vec(const HBatch &B, int w) { return B.vec + ((int64_t)blockIdx.y * HV_N + w) * B.len; }
__device__ __forceinline__ double *hb_part(const HBatch &B) { return B.part + (int64_t)blockIdx.y * HP_NSLOT * gridDim.x; }

// h_spmv_modes<MODE> on system blockIdx.y: st, part and the vectors are system 0's, the next system's stand 1 state,
// HP_NSLOT * gridDim.x partials and `vstride` pairs further; A.table is system 0's table.  The vectors come as
// __restrict__ arguments of their own: behind one base pointer the same body takes 98 VGPRs instead of 72
template <int MODE>
__global__ __launch_bounds__(EC3D_THREADS) void k_hb_spmv(HSav A, const HarmonicState *st, const cplx *__restrict__ x,
                                                         const cplx *__restrict__ o, cplx *__restrict__ y,
                                                         cplx *__restrict__ r0, cplx *__restrict__ p, int64_t nchunk,
                                                         double *__restrict__ part, int64_t vstride)
{
    extern __shared__ cplx tbl[];
    __shared__ double lds[12];
    const int64_t sys = blockIdx.y, v = sys * vstride;
    h_spmv_modes<MODE, false>(A, A.table + sys * A.ncls * 16, st + sys, x + v, MODE == 1 || MODE == 3 ? o + v : nullptr,
                              y + v, MODE == 3 ? r0 + v : nullptr, MODE == 3 ? p + v : nullptr, nchunk,
                              part + sys * HP_NSLOT * gridDim.x, tbl, lds);
}

// y = A^H x in the layout, the modes and the partial slots of k_hb_spmv: the adjoint solves of the left null vectors
// (DESIGN sections 18a, 18c) run the other four kernels around it unchanged.  There blockIdx.y is a SET of vectors, one
// per distinct omega, which borrows the work vectors, the partials and the state of system blockIdx.y; x stands
// `xstride` pairs apart -- the unknown of an adjoint solve is no work vector (MODE 3, and MODE 0 on w)
template <int MODE>
__global__ __launch_bounds__(EC3D_THREADS) void k_hb_spmv_h(HSav A, const HarmonicState *st, const cplx *__restrict__ x,
                                                           const cplx *__restrict__ o, cplx *__restrict__ y,
                                                           cplx *__restrict__ r0, cplx *__restrict__ p, int64_t nchunk,
                                                           double *__restrict__ part, int64_t vstride, int64_t xstride)
{
    extern __shared__ cplx tbl[];
    __shared__ double lds[12];
    const int64_t sys = blockIdx.y, v = sys * vstride;
    h_spmv_modes<MODE, true>(A, A.table + sys * A.ncls * 16, st + sys, x + sys * xstride,
                             MODE == 1 || MODE == 3 ? o + v : nullptr, y + v, MODE == 3 ? r0 + v : nullptr,
                             MODE == 3 ? p + v : nullptr, nchunk, part + sys * HP_NSLOT * gridDim.x, tbl, lds);
}

// one workgroup per system (grid (1, S)) behind k_hb_spmv<3> on (G, S)
__global__ __launch_bounds__(EC3D_THREADS) void k_hb_setup(HBatch B, int G, double tol)
{
    __shared__ double lds[8];
    h_setup_body(B.state + blockIdx.y, B.part + (int64_t)blockIdx.y * HP_NSLOT * G, G, tol, lds);
}

__global__ __launch_bounds__(EC3D_THREADS) void k_hb_s(HBatch B, int it, int64_t n, int64_t nchunk)
{
    __shared__ double lds[8];
    h_s_body(B.state + blockIdx.y, it, hb_vec(B, HV_R), hb_vec(B, HV_AP), hb_vec(B, HV_S), n, nchunk, hb_part(B), lds);
}

__global__ __launch_bounds__(EC3D_THREADS) void k_hb_xr(HBatch B, int it, int64_t n, int64_t nchunk)
{
    __shared__ double lds[16];
    h_xr_body(B.state + blockIdx.y, it, hb_vec(B, HV_P), hb_vec(B, HV_S), hb_vec(B, HV_AS), hb_vec(B, HV_R0), hb_vec(B, HV_X),
              hb_vec(B, HV_R), n, nchunk, hb_part(B), lds);
}

// k_hb_xr with the unknown at x + blockIdx.y * xstride in place of the system's HV_X (the adjoint solves).  A kernel of
// its own: the pointer beside the HBatch costs 10 VGPRs and a wave of occupancy (70 and 7 against 60 and 8)
__global__ __launch_bounds__(EC3D_THREADS) void k_hb_xr_at(HBatch B, int it, cplx *__restrict__ x, int64_t xstride, int64_t n,
                                                          int64_t nchunk)
{
    __shared__ double lds[16];
    h_xr_body(B.state + blockIdx.y, it, hb_vec(B, HV_P), hb_vec(B, HV_S), hb_vec(B, HV_AS), hb_vec(B, HV_R0),
              x + (int64_t)blockIdx.y * xstride, hb_vec(B, HV_R), n, nchunk, hb_part(B), lds);
}

__global__ __launch_bounds__(EC3D_THREADS) void k_hb_p(HBatch B, int it, int64_t n, int64_t nchunk)
{
    __shared__ double lds[12];
    h_p_body(B.state + blockIdx.y, it, hb_vec(B, HV_R), hb_vec(B, HV_AP), hb_vec(B, HV_P), hb_vec(B, HV_R0), n, nchunk, hb_part(B),
             lds);
}

// ---- left null vectors (DESIGN sections 18a, 18c): the streaming kernels of the set-up and of the projection --------
// The system is a grid dimension here too.  System s projects with the vectors of set set[s], of which kept[s] exist; a
// workgroup of a vector past kept[s] returns before it reads or writes anything.
struct HNSys {
    int32_t set[EC3D_HARMONIC_MAX_BATCH], kept[EC3D_HARMONIC_MAX_BATCH];
};
struct HNDiv {
    double d[EC3D_HARMONIC_MAX_BATCH]; // 0: the system is skipped
};

// partials of c_i = <Q_i, v> of system s = blockIdx.z, i = blockIdx.y: Q_i = qbase + set[s] * qset + i * qstride,
// v = vbase + s * vstride, the two parts at part[s * pstride + (2 i + {0, 1}) * G + b].  h_leave indexes with gridDim.x
// and blockIdx.x only: the sums do not depend on the other two grid dimensions
__global__ __launch_bounds__(EC3D_THREADS) void k_hbn_dots(HNSys M, const cplx *__restrict__ qbase, int64_t qset, int64_t qstride,
                                                          const cplx *__restrict__ vbase, int64_t vstride, int64_t n,
                                                          int64_t nchunk, double *__restrict__ part, int64_t pstride)
{
    __shared__ double lds[8];
    const int s = blockIdx.z;
    if ((int)blockIdx.y >= M.kept[s]) return;
    const cplx *q = qbase + (int64_t)M.set[s] * qset + (int64_t)blockIdx.y * qstride;
    const cplx *v = vbase + (int64_t)s * vstride;
    double acc[2] = {0.0, 0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx d = cdot(q[i], v[i]);
            acc[0] = acc[0] + d.x;
            acc[1] = acc[1] + d.y;
        }
    h_leave<2>(acc, part + (int64_t)s * pstride, 2 * (int)blockIdx.y, lds);
}

// workgroup (i, s): coef[s * cstride + i] = the two parts of c_i of system s, from `count` partials each
__global__ __launch_bounds__(EC3D_THREADS) void k_hbn_collapse(HNSys M, const double *__restrict__ part, int64_t pstride, int count,
                                                              cplx *__restrict__ coef, int64_t cstride)
{
    __shared__ double lds[8];
    const int s = blockIdx.y;
    if ((int)blockIdx.x >= M.kept[s]) return;
    double v[2];
    stream_strided_sum<2>(v, part + (int64_t)s * pstride + (int64_t)2 * blockIdx.x * count, count, count);
    stream_block_sum<2>(v, lds);
    if (threadIdx.x == 0) coef[(int64_t)s * cstride + blockIdx.x] = cplx{v[0], v[1]};
}

// v = v - c_0 Q_0 - ... - c_{k-1} Q_{k-1} on system s = blockIdx.y with its own k = kept[s] vectors, every term a rounded
// cmul and a rounded difference per part; r0, p (or null): copies of the new v; rr (or null): workgroup b's partial of
// ||v||^2 at rr[b], written by EVERY workgroup of the system.  r0, p, rr are system 0's, vstride pairs and rrstride
// doubles apart.  A system that kept nothing is left as it is, partials included
__global__ __launch_bounds__(EC3D_THREADS) void k_hbn_sub(HNSys M, const cplx *__restrict__ qbase, int64_t qset, int64_t qstride,
                                                         const cplx *__restrict__ coef, int64_t cstride, cplx *__restrict__ vbase,
                                                         cplx *__restrict__ r0base, cplx *__restrict__ pbase, int64_t vstride,
                                                         int64_t n, int64_t nchunk, double *__restrict__ rrbase, int64_t rrstride)
{
    __shared__ double lds[4];
    const int s = blockIdx.y, k = M.kept[s];
    if (k == 0) return;
    const cplx *q = qbase + (int64_t)M.set[s] * qset;
    const cplx *c = coef + (int64_t)s * cstride;
    cplx *v = vbase + (int64_t)s * vstride;
    cplx *r0 = r0base ? r0base + (int64_t)s * vstride : nullptr, *p = pbase ? pbase + (int64_t)s * vstride : nullptr;
    double acc[1] = {0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            cplx x = v[i];
            for (int m = 0; m < k; ++m) {
                const cplx t = cmul(c[m], q[(int64_t)m * qstride + i]);
                x = cplx{x.x - t.x, x.y - t.y};
            }
            v[i] = x;
            if (r0) r0[i] = x;
            if (p) p[i] = x;
            acc[0] = acc[0] + cabs2(x);
        }
    if (!rrbase) return;
    stream_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) rrbase[(int64_t)s * rrstride + blockIdx.x] = acc[0];
}

// v = v / D.d[s] on rows < n of system s = blockIdx.y, each part divided on its own
__global__ __launch_bounds__(EC3D_THREADS) void k_hbn_div(HNDiv D, cplx *__restrict__ vbase, int64_t vstride, int64_t n, int64_t nchunk)
{
    const double d = D.d[blockIdx.y];
    if (d == 0.0) return;
    cplx *v = vbase + (int64_t)blockIdx.y * vstride;
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx a = v[i];
            v[i] = cplx{a.x / d, a.y / d};
        }
}

// Re v[row] = Re v[row] + a (e_m and -e_m) on system blockIdx.x
__global__ void k_hbn_add_re(cplx *vbase, int64_t vstride, int64_t row, double a)
{
    cplx *v = vbase + (int64_t)blockIdx.x * vstride;
    v[row].x = v[row].x + a;
}

// host copies: (re plane, im plane) in device numbering <-> interleaved pairs; rows >= n of an uploaded vector are zero
__global__ void k_h_pack(const double *__restrict__ re, const double *__restrict__ im, cplx *__restrict__ v, int64_t n, int64_t n_pad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pad) v[i] = i < n ? cplx{re[i], im[i]} : cplx{0.0, 0.0};
}
__global__ void k_h_unpack(const cplx *__restrict__ v, double *__restrict__ re, double *__restrict__ im, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const cplx a = v[i];
        re[i] = a.x;
        im[i] = a.y;
    }
}

// ec3d_harmonic_load: the part of x^ and b^ into the real X and B ...
__global__ void k_h_load(const cplx *__restrict__ xh, const cplx *__restrict__ bh, int part, double *__restrict__ x,
                         double *__restrict__ b, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cplx a = xh[i], c = bh[i];
    x[i] = part ? a.y : a.x;
    b[i] = part ? c.y : c.x;
}
// ... B on the A rows of a conductor cell = the part of j (omega C) A^, omega C being the diagonal entry of the row's
// class in the im table ...
__global__ void k_h_load_eddy(const cplx *__restrict__ xh, const uint8_t *__restrict__ cls, const cplx *__restrict__ table,
                              const int32_t *__restrict__ cond_cell, int64_t nc, int64_t nCd, int part, double *__restrict__ b)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nc) return;
    const int64_t L = cond_cell[m];
    for (int d = 0; d < 3; ++d) {
        const int64_t q = d * nCd + L;
        const double w = table[(int64_t)cls[q] * 16 + 3].y;
        const cplx a = xh[q];
        b[q] = part ? w * a.x : -(w * a.y);
    }
}
// ... and both zeroed on the cel_bndX/Y/Z lists (src/EC3D.f90:426-432)
__global__ void k_h_zero_list(const int32_t *list, int64_t cnt, double *x, double *b)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnt) return;
    x[list[q]] = 0.0;
    b[list[q]] = 0.0;
}

inline unsigned blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

// the matrix with the table of system (or set) 0
HSav view_of(const ec3d_ctx *c, const cplx *table)
{
    const DevMatrix &A = c->A;
    HSav T;
    T.cls = A.cls;
    T.table = table;
    T.ncls = A.ncls;
    T.a0 = A.sav_a0;
    T.u0 = A.sav_u0;
    T.zero = A.sav_zero;
    T.n = A.n;
    T.nC = A.sav_nC;
    for (int b = 0; b < 7; ++b) T.off[b] = A.off[b];
    for (int d = 0; d < 3; ++d) T.step[d] = A.sav_step[d];
    return T;
}

// vector w of system sys
cplx *sysv(const ec3d_ctx *c, const HarmonicSystems &T, int sys, int w)
{
    return reinterpret_cast<cplx *>(T.vec.get()) + ((size_t)sys * HV_N + (size_t)w) * (size_t)c->A.n_pad;
}
cplx *hv(const ec3d_ctx *c, int w) { return sysv(c, c->harm.one, 0, w); }
bool is_batch(const ec3d_ctx *c, const HarmonicSystems &T) { return &T == &c->harm.batch; }

// the operator of a solve: K + j omega M or its conjugate transpose (the adjoint solves of the left null vectors)
enum HOp { H_A = 0, H_AH };

// S systems in lock step, as every launch of the iteration takes them: system s works in the state, partials and
// vectors `s` strides behind B's, under the table tab + s * ncls * 16, on the unknown x + s * xstride
struct HRun {
    int S, G;
    HBatch B;
    const cplx *tab;
    HOp op;
    cplx *x;
    int64_t xstride;
};
cplx *runv(const HRun &R, int w) { return R.B.vec + (int64_t)w * R.B.len; } // vector w of system 0

// the systems of T, each solving A x = b for its own HV_X
HRun run_of(const ec3d_ctx *c, const HarmonicSystems &T)
{
    const HBatch B = {sysv(c, T, 0, 0), T.part.get(), T.state.get(), c->A.n_pad};
    return HRun{T.n, T.wgs, B, reinterpret_cast<const cplx *>(T.tab.get()), H_A, sysv(c, T, 0, HV_X), (int64_t)HV_N * B.len};
}

// x: system 0's, xstride pairs apart (the adjoint only: under H_A x is a work vector); o, y, r0, p: work vectors of system 0
template <int MODE>
void launch_spmv(ec3d_ctx *c, const HRun &R, const cplx *x, int64_t xstride, const cplx *o, cplx *y, cplx *r0, cplx *p)
{
    const dim3 grid((unsigned)R.G, (unsigned)R.S);
    const size_t lds = (size_t)c->A.ncls * 16 * sizeof(cplx);
    const int64_t nc = c->A.n_pad / EC3D_TILE, vs = (int64_t)HV_N * R.B.len;
    if (R.op == H_A)
        k_hb_spmv<MODE><<<grid, EC3D_THREADS, lds, c->stream>>>(view_of(c, R.tab), R.B.state, x, o, y, r0, p, nc, R.B.part, vs);
    else
        k_hb_spmv_h<MODE><<<grid, EC3D_THREADS, lds, c->stream>>>(view_of(c, R.tab), R.B.state, x, o, y, r0, p, nc, R.B.part, vs,
                                                                  xstride);
}

// For every system s of T: c_{s,i} = <Q_{s,i}, R_s>; R_s = R_s - sum_i c_{s,i} Q_{s,i}, R0 = P = R; the partials of
// ||R_s||^2 in system s's HP_RR slots (one per workgroup), where k_hb_spmv<3> left them and k_hb_setup reads them
void launch_project(ec3d_ctx *c, const HarmonicSystems &T)
{
    const HarmonicNull &N = T.null;
    HNSys M{};
    int kmax = 0;
    for (int s = 0; s < T.n; ++s) {
        M.set[s] = N.set_of[s];
        M.kept[s] = N.kept[N.set_of[s]];
        kmax = std::max(kmax, M.kept[s]);
    }
    if (kmax == 0) return;
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE, vs = (int64_t)HV_N * len;
    const unsigned G = (unsigned)T.wgs, S = (unsigned)T.n;
    const int64_t pstride = (int64_t)2 * N.ncomp * T.wgs, cstride = N.ncomp, qset = (int64_t)N.ncomp * len;
    const cplx *q = reinterpret_cast<const cplx *>(N.q.get());
    cplx *coef = reinterpret_cast<cplx *>(N.coef.get());
    k_hbn_dots<<<dim3(G, (unsigned)kmax, S), EC3D_THREADS, 0, c->stream>>>(M, q, qset, len, sysv(c, T, 0, HV_R), vs, n, nc, N.part,
                                                                          pstride);
    k_hbn_collapse<<<dim3((unsigned)kmax, S), EC3D_THREADS, 0, c->stream>>>(M, N.part, pstride, T.wgs, coef, cstride);
    k_hbn_sub<<<dim3(G, S), EC3D_THREADS, 0, c->stream>>>(M, q, qset, len, coef, cstride, sysv(c, T, 0, HV_R), sysv(c, T, 0, HV_R0),
                                                         sysv(c, T, 0, HV_P), vs, n, nc, T.part.get() + (int64_t)HP_RR * T.wgs,
                                                         (int64_t)HP_NSLOT * T.wgs);
}

// R = b - op x, R0 = R, P = R and the state of a solve that has just begun; b: a work vector of system 0; project (or
// null): the systems whose left null vectors leave R first
void launch_begin(ec3d_ctx *c, const HRun &R, const cplx *b, double tol, const HarmonicSystems *project)
{
    launch_spmv<3>(c, R, R.x, R.xstride, b, runv(R, HV_R), runv(R, HV_R0), runv(R, HV_P));
    if (project) launch_project(c, *project);
    k_hb_setup<<<dim3(1, (unsigned)R.S), EC3D_THREADS, 0, c->stream>>>(R.B, R.G, tol);
}

// one lock-step iteration: five launches, every system in each
void launch_iteration(ec3d_ctx *c, const HRun &R, int it)
{
    const dim3 grid((unsigned)R.G, (unsigned)R.S);
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE, vs = (int64_t)HV_N * R.B.len;
    hipStream_t s = c->stream;
    launch_spmv<1>(c, R, runv(R, HV_P), vs, runv(R, HV_R0), runv(R, HV_AP), nullptr, nullptr);
    k_hb_s<<<grid, EC3D_THREADS, 0, s>>>(R.B, it, n, nc);
    launch_spmv<2>(c, R, runv(R, HV_S), vs, nullptr, runv(R, HV_AS), nullptr, nullptr);
    if (R.x == runv(R, HV_X))
        k_hb_xr<<<grid, EC3D_THREADS, 0, s>>>(R.B, it, n, nc);
    else
        k_hb_xr_at<<<grid, EC3D_THREADS, 0, s>>>(R.B, it, R.x, R.xstride, n, nc);
    k_hb_p<<<grid, EC3D_THREADS, 0, s>>>(R.B, it, n, nc);
}

inline bool h_stopped(const HarmonicState &q) { return q.stop_s != INT_MAX || q.stop_r != INT_MAX; }

// the S states in one copy
int states_to_host(ec3d_ctx *c, const HRun &R, std::vector<HarmonicState> &st)
{
    st.resize((size_t)R.S);
    EC3D_HIP(hipMemcpyAsync(st.data(), R.B.state, st.size() * sizeof(HarmonicState), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// itmax + 1 iterations at most (src/solvers.f90:25-29) behind a launch_begin, 16 enqueued per poll, on while any system
// runs; st: the states at the last poll
int run_iterations(ec3d_ctx *c, const HRun &R, int64_t itmax, std::vector<HarmonicState> &st)
{
    const int64_t total = itmax + 1;
    int64_t launched = 0;
    bool running;
    do {
        const int64_t m = std::min<int64_t>(16, total - launched);
        for (int64_t i = 0; i < m; ++i) launch_iteration(c, R, (int)(++launched));
        EC3D_HIP(hipGetLastError());
        int rc = states_to_host(c, R, st);
        if (rc) return rc;
        running = false;
        for (const HarmonicState &q : st) running = running || !h_stopped(q);
    } while (launched < total && running);
    return 0;
}

// iter, restarts, stop_kind and relres of a solve from its last state; total = itmax + 1 iterations were allowed
void h_report(ec3d_harmonic_info &o, const HarmonicState &st, int64_t total)
{
    o.iter = h_stopped(st) ? std::min(st.stop_s, st.stop_r) : (int32_t)std::max<int64_t>(total, 0);
    o.restarts = st.restarts;
    o.stop_kind = st.stop_s != INT_MAX ? 1 : (st.stop_r != INT_MAX && st.stop_r > 0 ? 2 : 0);
    const double last_norm = o.stop_kind == 1 ? st.snorm : st.rnorm;
    o.relres = st.bnorm > 0.0 ? last_norm / st.bnorm : 0.0;
}

// what every entry point refuses first; ready: ec3d_harmonic_setup must have run
int h_need(ec3d_ctx *c, const char *who, bool ready)
{
    if (!c) {
        ec3d_set_error(std::string(who) + ": null handle");
        return 2;
    }
    int rc = ec3d_need_undivided(c, who);
    if (rc) return rc;
    if ((rc = ec3d_null_eligible(c, who, true))) return rc;
    if (!c->harm.re || !c->harm.m) {
        ec3d_set_error(std::string(who) + ": needs the A-V system [Ax|Ay|Az|U] from ec3d_assemble");
        return 3;
    }
    if (ready && c->harm.one.n == 0) {
        ec3d_set_error(std::string(who) + ": call ec3d_harmonic_setup first");
        return 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    return 0;
}

// h_need and: a batch exists, sys is one of its systems (any_sys: not asked)
int hb_need(ec3d_ctx *c, const char *who, int32_t sys, bool any_sys)
{
    int rc = h_need(c, who, false);
    if (rc) return rc;
    const int bn = c->harm.batch.n;
    if (bn == 0) {
        ec3d_set_error(std::string(who) + ": call ec3d_harmonic_batch_setup first");
        return 2;
    }
    if (!any_sys && (sys < 0 || sys >= bn)) {
        ec3d_set_error(std::string(who) + ": system " + std::to_string(sys) + " is outside the batch of " + std::to_string(bn));
        return 2;
    }
    return 0;
}

// the entry points that exist for the single system and for system sys of the batch: what they refuse first, and *T
int h_enter(ec3d_ctx *c, const char *who, bool batch, int32_t sys, HarmonicSystems **T)
{
    const int rc = batch ? hb_need(c, who, sys, false) : h_need(c, who, true);
    if (rc) return rc;
    *T = batch ? &c->harm.batch : &c->harm.one;
    return 0;
}

// the (re, omega m) pairs of the operators omega[0 .. S - 1], one after another, from the two tables of ec3d_assemble
int h_tables(ec3d_ctx *c, int S, const double *omega, std::vector<double> &tabs)
{
    const size_t nt = (size_t)c->A.ncls * 16;
    std::vector<double> re(nt), m(nt);
    EC3D_HIP(hipMemcpy(re.data(), c->harm.re, nt * sizeof(double), hipMemcpyDeviceToHost));
    EC3D_HIP(hipMemcpy(m.data(), c->harm.m, nt * sizeof(double), hipMemcpyDeviceToHost));
    tabs.resize((size_t)S * 2 * nt);
    for (int s = 0; s < S; ++s)
        for (size_t q = 0; q < nt; ++q) {
            tabs[((size_t)s * nt + q) * 2] = re[q];
            tabs[((size_t)s * nt + q) * 2 + 1] = omega[s] * m[q]; // one rounding per entry
        }
    return 0;
}

int h_which(int which, const char *who)
{
    if (which == EC3D_VEC_X || which == EC3D_VEC_B) return 0;
    ec3d_set_error(std::string(who) + ": which must be EC3D_VEC_X or EC3D_VEC_B");
    return 2;
}

// stage: the 2 * n_pad doubles of staging of the systems that own dst
int h_to_device(ec3d_ctx *c, double *stage, cplx *dst, const double *re, const double *im)
{
    const int64_t len = c->A.n_pad;
    double *sre = stage, *sim = stage + len;
    int rc;
    if ((rc = ec3d_vec_h2d(c, sre, re))) return rc;
    if (im) {
        if ((rc = ec3d_vec_h2d(c, sim, im))) return rc;
    } else {
        EC3D_HIP(hipMemsetAsync(sim, 0, (size_t)c->A.n * sizeof(double), c->stream));
    }
    k_h_pack<<<blocks(len), 256, 0, c->stream>>>(sre, sim, dst, c->A.n, len);
    EC3D_HIP(hipGetLastError());
    return 0;
}

int h_to_host(ec3d_ctx *c, double *stage, const cplx *src, double *re, double *im)
{
    double *sre = stage, *sim = stage + c->A.n_pad;
    k_h_unpack<<<blocks(c->A.n), 256, 0, c->stream>>>(src, sre, sim, c->A.n);
    EC3D_HIP(hipGetLastError());
    int rc;
    if (re && (rc = ec3d_vec_d2h(c, re, sre))) return rc;
    if (im && (rc = ec3d_vec_d2h(c, im, sim))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- storage ---------------------------------------------------------------------------------------------------------
// the vectors of a null projection and what was reported of them; the setting stays
void null_free(HarmonicNull &N)
{
    HarmonicNull fresh;
    fresh.on = N.on;
    fresh.tol = N.tol;
    N = std::move(fresh); // (a buffer that is moved onto is freed)
}

// the systems and their null projection; its setting stays with the handle
void systems_free(HarmonicSystems &T)
{
    null_free(T.null);
    HarmonicSystems fresh;
    fresh.null = std::move(T.null);
    T = std::move(fresh);
}

// everything of S systems but the tables' contents: vectors, partials, staging and states, all zero
int systems_alloc(ec3d_ctx *c, HarmonicSystems &T, int S)
{
    const size_t nt = (size_t)c->A.ncls * 16, len = (size_t)c->A.n_pad;
    const int G = ec3d_stream_wgs((int64_t)len);
    EC3D_HIP(T.vec.alloc((size_t)S * HV_N * 2 * len));
    EC3D_HIP(T.tab.alloc((size_t)S * 2 * nt));
    EC3D_HIP(T.part.alloc((size_t)S * HP_NSLOT * G));
    EC3D_HIP(T.stage.alloc(2 * len));
    EC3D_HIP(T.state.alloc((size_t)S));
    EC3D_HIP(hipMemsetAsync(T.vec, 0, (size_t)S * HV_N * 2 * len * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(T.part, 0, (size_t)S * HP_NSLOT * G * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(T.stage, 0, 2 * len * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(T.state, 0, (size_t)S * sizeof(HarmonicState), c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    T.wgs = G;
    T.bytes = (int64_t)(((size_t)S * HV_N * 2 * len + (size_t)S * 2 * nt + (size_t)S * HP_NSLOT * G + 2 * len) * sizeof(double) +
                        (size_t)S * sizeof(HarmonicState));
    return 0;
}

// ---- left null vectors (DESIGN sections 18a, 18c) --------------------------------------------------------------------
// the lowest system whose omega has the bits of system s's
int shares_with(const HarmonicSystems &T, int s)
{
    for (int t = 0; t < s; ++t)
        if (std::memcmp(&T.omega[t], &T.omega[s], sizeof(double)) == 0) return t;
    return s;
}

// out[d] = the real part of sum <a_d, v_d> over the rows (a == v: ||v_d||^2), d < D: a_d = a + d * astride,
// v_d = v + d * vstride; one k_hbn_dots, one collapse and one copy, in the partials and coefficients of the projection
int dots_to_host(ec3d_ctx *c, const HarmonicSystems &T, int D, const cplx *a, int64_t astride, const cplx *v, int64_t vstride,
                 double *out)
{
    const HarmonicNull &N = T.null;
    HNSys M{};
    for (int d = 0; d < D; ++d) {
        M.set[d] = d;
        M.kept[d] = 1;
    }
    const int64_t pstride = (int64_t)2 * N.ncomp * T.wgs, cstride = N.ncomp;
    cplx *coef = reinterpret_cast<cplx *>(N.coef.get());
    k_hbn_dots<<<dim3((unsigned)T.wgs, 1, (unsigned)D), EC3D_THREADS, 0, c->stream>>>(M, a, astride, 0, v, vstride, c->A.n,
                                                                                    c->A.n_pad / EC3D_TILE, N.part, pstride);
    k_hbn_collapse<<<dim3(1, (unsigned)D), EC3D_THREADS, 0, c->stream>>>(M, N.part, pstride, T.wgs, coef, cstride);
    EC3D_HIP(hipGetLastError());
    std::vector<double> h((size_t)2 * cstride * D);
    EC3D_HIP(hipMemcpyAsync(h.data(), coef, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    for (int d = 0; d < D; ++d) out[d] = h[(size_t)2 * cstride * d];
    return 0;
}

// A w that missed null_tol is never used.  Missed: no exit within the cap, or an exit of the recurrence that the true
// residual ||A^H w|| / ||c|| does not bear out.  The exits bound the recurrence's residual by null_tol ||c||; the true
// one differs from it by the rounding gathered along the solve, some 1e-14 ||c|| and far below any null_tol the
// arithmetic can deliver, so twice the bound tells a solve that delivered from a recurrence that ran away.
bool null_solve_missed(const HarmonicState &q, double true_rel, double null_tol)
{
    return !h_stopped(q) || !(true_rel <= 2.0 * null_tol);
}

// the error of a set-up whose adjoint solve of set d, component ci missed; the batch's names the system and its omega
std::string null_missed_text(const HarmonicSystems &T, bool batch, int d, int ci, const NullSeed &seed, const HarmonicState &q,
                             int64_t cap, double true_rel)
{
    char who[120] = "harmonic null projection: the adjoint solve of";
    if (batch)
        snprintf(who, sizeof who, "harmonic batch null projection: the adjoint solve of system %d (omega = %.17g),",
                 T.null.first[d], T.omega[T.null.first[d]]);
    const bool stopped = h_stopped(q);
    char msg[480];
    snprintf(msg, sizeof msg, "%s conducting component %d (seed row %lld) did not reach null_tol = %.3g: %s after %lld iterations "
             "(cap %lld), true residual ||A^H w|| / ||A^H e_m|| = %.3g; %s", who, ci, (long long)seed.seed_ref, T.null.tol,
             stopped ? "the recurrence took an exit" : "no exit", (long long)(stopped ? std::min(q.stop_s, q.stop_r) : cap + 1),
             (long long)cap, true_rel, batch ? "no left null vector of the batch is used" : "its left null vector is not used");
    return msg;
}

// w of norm n0 left Gram-Schmidt against the vectors kept with norm n1: kept unless (nearly) nothing of it is new
bool null_keeps(double n0, double n1) { return std::isfinite(n0) && std::isfinite(n1) && n1 > EC3D_NULL_MIN_KEEP * n0; }

// The set-up of a null projection, once per matrix and set of omegas.  Per connected conducting component
// (ec3d_null_seeds), for the D distinct omegas of T in lock step: c = A^H (-e_m) into AS by one launch (-e_m in S); the
// adjoint solve A^H y = c from y = 0 -- this file's iteration around k_hb_spmv_h, set d in the work vectors R, R0, P, AP,
// S, AS, the partials and the state of system d, which nothing reads between two solves; X^ and B^ of no system are
// touched -- then w = y + e_m, ||A^H w|| / ||w||, and classical Gram-Schmidt against the vectors kept, the decisions on
// the host from one copy of D figures.  The unknown: the single system solves in the next free slot of its Q, where a
// kept vector stays; the sets of a batch keep different numbers of vectors, so set d solves in the staging vector
// y + d * n_pad under the table of its omega, and a kept vector is copied into its slot: a copy keeps the bits.
int null_build(ec3d_ctx *c, HarmonicSystems &T)
{
    HarmonicNull &N = T.null;
    const bool staged = is_batch(c, T);
    const auto t_start = std::chrono::steady_clock::now();
    null_free(N);
    EC3D_HIP(hipStreamSynchronize(c->stream));
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE, vs = (int64_t)HV_N * len;
    int D = 0;
    for (int s = 0; s < T.n; ++s) {
        const int f = shares_with(T, s);
        if (f == s) {
            N.first[D] = s;
            N.set_of[s] = D++;
        } else {
            N.set_of[s] = N.set_of[f];
        }
    }
    N.sets = D;
    std::vector<NullSeed> seeds;
    int rc = ec3d_null_seeds(c, seeds);
    if (rc) return rc;
    const int ncomp = (int)seeds.size();
    for (int d = 0; d < D; ++d) {
        N.last[d].found = ncomp;
        N.last[d].reported = std::min(ncomp, EC3D_NULL_MAX_REPORT);
    }
    if (ncomp == 0) { // no conductor: the operator has no such null vector, the projection is the identity
        N.built = true;
        return 0;
    }
    const size_t nt = (size_t)c->A.ncls * 16, nq = (size_t)D * ncomp * 2 * len;
    const size_t npart = (size_t)T.n * 2 * ncomp * T.wgs, ncoef = (size_t)T.n * 2 * ncomp;
    EC3D_HIP(N.q.alloc(nq));
    EC3D_HIP(hipMemsetAsync(N.q, 0, nq * sizeof(double), c->stream));
    EC3D_HIP(N.part.alloc(npart));
    EC3D_HIP(N.coef.alloc(ncoef));
    N.bytes = (int64_t)((nq + npart + ncoef) * sizeof(double));
    if (staged) {
        EC3D_HIP(N.y.alloc((size_t)D * 2 * len));
        EC3D_HIP(N.tab.alloc((size_t)D * 2 * nt));
        N.bytes += (int64_t)(((size_t)D * 2 * len + (size_t)D * 2 * nt) * sizeof(double));
        EC3D_HIP(hipMemsetAsync(N.part, 0, npart * sizeof(double), c->stream));
        EC3D_HIP(hipMemsetAsync(N.coef, 0, ncoef * sizeof(double), c->stream));
        std::vector<double> omega((size_t)D), tabs;
        for (int d = 0; d < D; ++d) omega[(size_t)d] = T.omega[N.first[d]];
        if ((rc = h_tables(c, D, omega.data(), tabs))) return rc;
        EC3D_HIP(hipMemcpy(N.tab, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    N.ncomp = ncomp;
    cplx *Q = reinterpret_cast<cplx *>(N.q.get()), *coef = reinterpret_cast<cplx *>(N.coef.get());
    const int64_t cap = (int64_t)(20.0 * std::cbrt((double)c->n_ref)) + 2000;
    const int64_t pstride = (int64_t)2 * ncomp * T.wgs, cstride = ncomp, qset = (int64_t)ncomp * len;
    const dim3 grid((unsigned)T.wgs, (unsigned)D);
    HRun R = run_of(c, T);
    R.S = D;
    R.op = H_AH;
    if (staged) R.tab = reinterpret_cast<const cplx *>(N.tab.get());
    hipStream_t s = c->stream;
    std::vector<HarmonicState> st;
    std::vector<double> aw2((size_t)D), w2((size_t)D), w2b((size_t)D);
    for (int ci = 0; ci < ncomp; ++ci) {
        const int64_t row = seeds[(size_t)ci].row;
        R.x = staged ? reinterpret_cast<cplx *>(N.y.get()) : Q + (size_t)N.kept[0] * len; // y, then w, then (divided) Q_kept
        R.xstride = staged ? len : qset;
        for (int d = 0; d < D; ++d) EC3D_HIP(hipMemsetAsync(sysv(c, T, d, HV_S), 0, (size_t)n * sizeof(cplx), s));
        k_hbn_add_re<<<(unsigned)D, 1, 0, s>>>(runv(R, HV_S), vs, row, -1.0);
        launch_spmv<0>(c, R, runv(R, HV_S), vs, nullptr, runv(R, HV_AS), nullptr, nullptr);
        if (staged) EC3D_HIP(hipMemsetAsync(R.x, 0, (size_t)D * len * sizeof(cplx), s)); // (a free slot of Q is zero)
        launch_begin(c, R, runv(R, HV_AS), N.tol, nullptr);
        EC3D_HIP(hipGetLastError());
        if ((rc = run_iterations(c, R, cap, st))) return rc;
        k_hbn_add_re<<<(unsigned)D, 1, 0, s>>>(R.x, R.xstride, row, 1.0);
        // c - A^H y = -A^H w: ||A^H w|| is the adjoint system's TRUE residual, and the figure of the report
        launch_spmv<0>(c, R, R.x, R.xstride, nullptr, runv(R, HV_AS), nullptr, nullptr);
        if ((rc = dots_to_host(c, T, D, runv(R, HV_AS), vs, runv(R, HV_AS), vs, aw2.data()))) return rc;
        if ((rc = dots_to_host(c, T, D, R.x, R.xstride, R.x, R.xstride, w2.data()))) return rc;
        for (int d = 0; d < D; ++d) {
            const double true_rel = std::sqrt(aw2[(size_t)d]) / st[(size_t)d].bnorm;
            if (!null_solve_missed(st[(size_t)d], true_rel, N.tol)) continue;
            const std::string msg = null_missed_text(T, staged, d, ci, seeds[(size_t)ci], st[(size_t)d], cap, true_rel);
            null_free(N);
            ec3d_set_error(msg);
            return EC3D_NULL_E_SETUP;
        }
        HNSys K{};
        int kmax = 0;
        for (int d = 0; d < D; ++d) {
            K.set[d] = d;
            K.kept[d] = N.kept[d];
            kmax = std::max(kmax, K.kept[d]);
        }
        w2b = w2;
        if (kmax > 0) {
            k_hbn_dots<<<dim3(grid.x, (unsigned)kmax, grid.y), EC3D_THREADS, 0, s>>>(K, Q, qset, len, R.x, R.xstride, n, nc, N.part,
                                                                                   pstride);
            k_hbn_collapse<<<dim3((unsigned)kmax, grid.y), EC3D_THREADS, 0, s>>>(K, N.part, pstride, T.wgs, coef, cstride);
            k_hbn_sub<<<grid, EC3D_THREADS, 0, s>>>(K, Q, qset, len, coef, cstride, R.x, nullptr, nullptr, R.xstride, n, nc, nullptr, 0);
            std::vector<double> after((size_t)D);
            if ((rc = dots_to_host(c, T, D, R.x, R.xstride, R.x, R.xstride, after.data()))) return rc;
            for (int d = 0; d < D; ++d)
                if (K.kept[d] > 0) w2b[(size_t)d] = after[(size_t)d];
        }
        HNDiv dv{};
        bool keep[EC3D_HARMONIC_MAX_BATCH] = {false}, any = false;
        for (int d = 0; d < D; ++d) {
            const double n1 = std::sqrt(w2b[(size_t)d]);
            keep[d] = null_keeps(std::sqrt(w2[(size_t)d]), n1);
            dv.d[d] = keep[d] ? n1 : 0.0;
            any = any || keep[d];
        }
        if (any) k_hbn_div<<<grid, EC3D_THREADS, 0, s>>>(dv, R.x, R.xstride, n, nc);
        for (int d = 0; d < D; ++d) {
            cplx *w = R.x + (size_t)d * R.xstride;
            if (keep[d] && staged)
                EC3D_HIP(hipMemcpyAsync(Q + (size_t)d * qset + (size_t)N.kept[d] * len, w, (size_t)len * sizeof(cplx),
                                        hipMemcpyDeviceToDevice, s));
            if (!keep[d] && !staged) EC3D_HIP(hipMemsetAsync(w, 0, (size_t)len * sizeof(cplx), s)); // the slot is free again
            if (keep[d]) ++N.kept[d];
            if (ci < EC3D_NULL_MAX_REPORT) {
                ec3d_null_info &L = N.last[d];
                const HarmonicState &q = st[(size_t)d];
                L.seed_row[ci] = seeds[(size_t)ci].seed_ref;
                L.iterations[ci] = std::min(q.stop_s, q.stop_r);
                L.was_kept[ci] = keep[d] ? 1 : 0;
                L.residual[ci] = std::sqrt(aw2[(size_t)d]) / std::sqrt(w2[(size_t)d]);
                N.restarts[d][ci] = q.restarts;
            }
        }
    }
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipStreamSynchronize(s));
    N.built = true;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    for (int d = 0; d < D; ++d) {
        N.last[d].kept = N.kept[d];
        N.last[d].dropped = ncomp - N.kept[d];
        N.last[d].setup_ms = ms;
    }
    return 0;
}

// removed_s = sqrt(sum_i |c_{s,i}|^2) / ||b^_s|| of the projection that has just run, per system: one copy of the
// coefficients
int null_note(ec3d_ctx *c, HarmonicSystems &T, const std::vector<HarmonicState> &st)
{
    HarmonicNull &N = T.null;
    bool any = false;
    for (int s = 0; s < T.n; ++s) {
        N.removed[s] = 0.0;
        any = any || (N.kept[N.set_of[s]] > 0 && st[(size_t)s].bnorm != 0.0);
    }
    if (!any) return 0;
    std::vector<double> h((size_t)T.n * 2 * N.ncomp);
    EC3D_HIP(hipMemcpy(h.data(), N.coef, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < T.n; ++s) {
        const int kept = N.kept[N.set_of[s]];
        const double bnorm = st[(size_t)s].bnorm;
        if (kept == 0 || bnorm == 0.0) continue;
        const double *q = h.data() + (size_t)s * 2 * N.ncomp;
        double sum = 0.0;
        for (int i = 0; i < 2 * kept; i += 2) sum += q[i] * q[i] + q[i + 1] * q[i + 1];
        N.removed[s] = std::sqrt(sum) / bnorm;
    }
    return 0;
}

// ---- what the entry points of the single system and of the batch share ----------------------------------------------
// the solve of every system of T; the report in T.last
int h_solve(ec3d_ctx *c, HarmonicSystems &T, double tol, int32_t itmax)
{
    HarmonicNull &N = T.null;
    int rc;
    if (N.on && !N.built && (rc = null_build(c, T))) return rc;
    const auto t_start = std::chrono::steady_clock::now();
    const HRun R = run_of(c, T);
    launch_begin(c, R, runv(R, HV_B), tol, N.on ? &T : nullptr);
    EC3D_HIP(hipGetLastError());
    std::vector<HarmonicState> st;
    if ((rc = run_iterations(c, R, itmax, st))) return rc;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    for (int s = 0; s < T.n; ++s) {
        h_report(T.last[s], st[(size_t)s], (int64_t)itmax + 1); // src/solvers.f90:25-29: itmax + 1 iterations
        T.last[s].ms = ms;
    }
    if (N.on) return null_note(c, T, st);
    return 0;
}

// b^ - A x^ of every system as a solve would begin with it, the left null vectors taken out if `project`: the states
int h_residual(ec3d_ctx *c, HarmonicSystems &T, bool project, std::vector<HarmonicState> &st)
{
    int rc;
    if (project && !T.null.built && (rc = null_build(c, T))) return rc;
    const HRun R = run_of(c, T);
    launch_begin(c, R, runv(R, HV_B), 0.0, project ? &T : nullptr);
    EC3D_HIP(hipGetLastError());
    if ((rc = states_to_host(c, R, st))) return rc;
    return project ? null_note(c, T, st) : 0;
}

int h_upload(ec3d_ctx *c, const char *who, bool batch, int32_t sys, int which, const double *re, const double *im)
{
    HarmonicSystems *T;
    int rc = h_enter(c, who, batch, sys, &T);
    if (rc) return rc;
    if ((rc = h_which(which, who))) return rc;
    if (!re) {
        ec3d_set_error(std::string(who) + ": re is NULL");
        return 2;
    }
    if ((rc = h_to_device(c, T->stage, sysv(c, *T, sys, which == EC3D_VEC_X ? HV_X : HV_B), re, im))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int h_download(ec3d_ctx *c, const char *who, bool batch, int32_t sys, int which, double *re, double *im)
{
    HarmonicSystems *T;
    int rc = h_enter(c, who, batch, sys, &T);
    if (rc) return rc;
    if ((rc = h_which(which, who))) return rc;
    if (!re || !im) {
        ec3d_set_error(std::string(who) + ": re or im is NULL");
        return 2;
    }
    return h_to_host(c, T->stage, sysv(c, *T, sys, which == EC3D_VEC_X ? HV_X : HV_B), re, im);
}

int h_device_vector(ec3d_ctx *c, const char *who, bool batch, int32_t sys, int which, double **device_ptr, int64_t *pairs)
{
    HarmonicSystems *T;
    const int rc = h_enter(c, who, batch, sys, &T);
    if (rc) return rc;
    if (which < 0 || which >= HV_N || !device_ptr || !pairs) {
        ec3d_set_error(std::string(who) + ": unknown vector or NULL argument");
        return 2;
    }
    *device_ptr = reinterpret_cast<double *>(sysv(c, *T, sys, which));
    *pairs = c->A.n_pad;
    return 0;
}

// on: a tolerance other than the vectors' own has them made again
int h_null_switch_on(ec3d_ctx *c, HarmonicNull &N, double null_tol)
{
    const double tol = null_tol > 0.0 ? null_tol : 1e-10;
    if (tol != N.tol && N.built) {
        EC3D_HIP(hipStreamSynchronize(c->stream));
        null_free(N); // another accuracy: the vectors are made again
    }
    N.on = 1;
    N.tol = tol;
    return 0;
}

void h_null_info(const HarmonicNull &N, int sys, ec3d_null_info *info)
{
    *info = N.built ? N.last[N.set_of[sys]] : ec3d_null_info{};
    info->on = N.on;
    info->null_tol = N.tol;
    info->built = N.built ? 1 : 0;
    info->removed = N.removed[sys];
}

int h_left_null_vector(ec3d_ctx *c, const char *who, bool batch, int32_t sys, int32_t index, double *re, double *im)
{
    HarmonicSystems *T;
    int rc = h_enter(c, who, batch, sys, &T);
    if (rc) return rc;
    HarmonicNull &N = T->null;
    if (!N.built) {
        if (!N.on) {
            ec3d_set_error(std::string(who) + ": no vectors yet and the projection is off (" +
                           (batch ? "ec3d_harmonic_batch_set_null_projection" : "ec3d_harmonic_set_null_projection") + ")");
            return 2;
        }
        if ((rc = null_build(c, *T))) return rc;
    }
    const int d = N.set_of[sys], kept = N.kept[d];
    if (index < 0 || index >= kept || !re || !im) {
        ec3d_set_error(std::string(who) + ": index " + std::to_string(index) + " is outside the " + std::to_string(kept) +
                       " vectors kept" + (batch ? " for system " + std::to_string(sys) : std::string()) + ", or a NULL argument");
        return 2;
    }
    return h_to_host(c, T->stage, reinterpret_cast<const cplx *>(N.q.get()) + ((size_t)d * N.ncomp + (size_t)index) * c->A.n_pad, re,
                     im);
}

void h_null_restarts(const HarmonicNull &N, int sys, int32_t *restarts)
{
    for (int i = 0; i < EC3D_NULL_MAX_REPORT; ++i) restarts[i] = N.built ? N.restarts[N.set_of[sys]][i] : 0;
}

// y = op x: x^ of the handle, or the caller's (through P); y through AP
int h_spmv_entry(ec3d_ctx *c, const char *who, HOp op, const double *xre, const double *xim, double *yre, double *yim)
{
    int rc = h_need(c, who, true);
    if (rc) return rc;
    if (!yre || !yim || (xre && !xim)) {
        ec3d_set_error(std::string(who) + ": NULL argument");
        return 2;
    }
    HRun R = run_of(c, c->harm.one);
    R.op = op;
    const cplx *x = hv(c, HV_X);
    if (xre) {
        if ((rc = h_to_device(c, c->harm.one.stage, hv(c, HV_P), xre, xim))) return rc;
        x = hv(c, HV_P);
    }
    launch_spmv<0>(c, R, x, R.xstride, nullptr, hv(c, HV_AP), nullptr, nullptr);
    EC3D_HIP(hipGetLastError());
    return h_to_host(c, c->harm.one.stage, hv(c, HV_AP), yre, yim);
}

} // namespace

void ec3d_harmonic_free(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    systems_free(H.one);
    systems_free(H.batch);
    H.re.reset();
    H.m.reset();
}

extern "C" int ec3d_harmonic_setup(ec3d_handle c, double omega)
{
    int rc = h_need(c, "ec3d_harmonic_setup", false);
    if (rc) return rc;
    if (!(omega >= 0.0) || !std::isfinite(omega)) {
        ec3d_set_error("ec3d_harmonic_setup: omega must be finite and not negative");
        return 2;
    }
    HarmonicSystems &T = c->harm.one;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    if (!(T.n && omega == T.omega[0])) null_free(T.null); // Q belongs to the matrix and to omega
    std::vector<double> tab;
    if ((rc = h_tables(c, 1, &omega, tab))) return rc;
    if (!T.vec && (rc = systems_alloc(c, T, 1))) return rc; // the first set-up on this matrix; the vectors stay across omegas
    EC3D_HIP(hipMemcpy(T.tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    T.n = 1;
    T.omega[0] = omega;
    T.last[0] = ec3d_harmonic_info{};
    T.last[0].ready = 1;
    T.last[0].omega = omega;
    T.last[0].device_bytes = T.bytes;
    return 0;
}

extern "C" int ec3d_harmonic_upload(ec3d_handle c, int which, const double *re, const double *im)
{
    return h_upload(c, "ec3d_harmonic_upload", false, 0, which, re, im);
}

extern "C" int ec3d_harmonic_download(ec3d_handle c, int which, double *re, double *im)
{
    return h_download(c, "ec3d_harmonic_download", false, 0, which, re, im);
}

extern "C" int ec3d_harmonic_spmv(ec3d_handle c, const double *xre, const double *xim, double *yre, double *yim)
{
    return h_spmv_entry(c, "ec3d_harmonic_spmv", H_A, xre, xim, yre, yim);
}

extern "C" int ec3d_harmonic_solve(ec3d_handle c, double tol, int32_t itmax, int32_t *iter, double *relres)
{
    int rc = h_need(c, "ec3d_harmonic_solve", true);
    if (rc) return rc;
    HarmonicSystems &T = c->harm.one;
    if ((rc = h_solve(c, T, tol, itmax))) return rc;
    if (iter) *iter = T.last[0].iter;
    if (relres) *relres = T.last[0].relres;
    return 0;
}

extern "C" int ec3d_harmonic_true_residual(ec3d_handle c, double *rel, double *bnorm)
{
    int rc = h_need(c, "ec3d_harmonic_true_residual", true);
    if (rc) return rc;
    if (!rel) {
        ec3d_set_error("ec3d_harmonic_true_residual: rel is NULL");
        return 2;
    }
    std::vector<HarmonicState> st;
    if ((rc = h_residual(c, c->harm.one, false, st))) return rc;
    if (bnorm) *bnorm = st[0].bnorm;
    *rel = st[0].bnorm > 0.0 ? st[0].rnorm / st[0].bnorm : st[0].rnorm;
    return 0;
}

extern "C" int ec3d_harmonic_load(ec3d_handle c, int32_t part)
{
    int rc = h_need(c, "ec3d_harmonic_load", true);
    if (rc) return rc;
    if (part != 0 && part != 1) {
        ec3d_set_error("ec3d_harmonic_load: part must be 0 (Re) or 1 (Im)");
        return 2;
    }
    double *x = c->vec[EC3D_VEC_X], *b = c->vec[EC3D_VEC_B];
    hipStream_t s = c->stream;
    k_h_load<<<blocks(c->A.n), 256, 0, s>>>(hv(c, HV_X), hv(c, HV_B), part, x, b, c->A.n);
    if (c->n_cond) {
        k_h_load_eddy<<<blocks(c->n_cond), 256, 0, s>>>(hv(c, HV_X), c->A.cls, reinterpret_cast<const cplx *>(c->harm.one.tab.get()),
                                                       c->cond_cell, c->n_cond, c->nCd, part, b);
        const int64_t cnt = c->bnd_off[3];
        if (cnt) k_h_zero_list<<<blocks(cnt), 256, 0, s>>>(c->bnd_list, cnt, x, b);
    }
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipStreamSynchronize(s));
    return 0;
}

extern "C" int ec3d_get_harmonic(ec3d_handle c, ec3d_harmonic_info *out)
{
    if (!c || !out) {
        ec3d_set_error("ec3d_get_harmonic: null handle or info");
        return 2;
    }
    const HarmonicSystems &T = c->harm.one;
    *out = T.last[0];
    out->ready = T.n ? 1 : 0;
    out->omega = T.omega[0];
    out->device_bytes += T.null.bytes; // Q, its partials and coefficients, while they exist
    return 0;
}

extern "C" int ec3d_harmonic_device_vector(ec3d_handle c, int which, double **device_ptr, int64_t *pairs)
{
    return h_device_vector(c, "ec3d_harmonic_device_vector", false, 0, which, device_ptr, pairs);
}

// ---- left null vectors of K + j omega M -------------------------------------------------------
extern "C" int ec3d_harmonic_set_null_projection(ec3d_handle c, int32_t on, double null_tol)
{
    if (!c) {
        ec3d_set_error("ec3d_harmonic_set_null_projection: null handle");
        return 2;
    }
    if (!on) {
        c->harm.one.null.on = 0; // Q stays with the matrix and omega: switching on again costs nothing
        return 0;
    }
    const int rc = h_need(c, "ec3d_harmonic_set_null_projection", true);
    if (rc) return rc; // (the setting as it was)
    return h_null_switch_on(c, c->harm.one.null, null_tol);
}

extern "C" int ec3d_get_harmonic_null(ec3d_handle c, ec3d_null_info *info)
{
    if (!c || !info) {
        ec3d_set_error("ec3d_get_harmonic_null: null handle or info");
        return 2;
    }
    h_null_info(c->harm.one.null, 0, info);
    return 0;
}

extern "C" int ec3d_harmonic_left_null_vector(ec3d_handle c, int32_t index, double *re, double *im)
{
    return h_left_null_vector(c, "ec3d_harmonic_left_null_vector", false, 0, index, re, im);
}

extern "C" int ec3d_harmonic_spmv_h(ec3d_handle c, const double *xre, const double *xim, double *yre, double *yim)
{
    return h_spmv_entry(c, "ec3d_harmonic_spmv_h", H_AH, xre, xim, yre, yim);
}

extern "C" int ec3d_harmonic_projected_residual(ec3d_handle c, double *rel, double *removed)
{
    int rc = h_need(c, "ec3d_harmonic_projected_residual", true);
    if (rc) return rc;
    HarmonicSystems &T = c->harm.one;
    if (!T.null.on || !rel) {
        ec3d_set_error(!rel ? "ec3d_harmonic_projected_residual: rel is NULL"
                            : "ec3d_harmonic_projected_residual: the projection is off (ec3d_harmonic_set_null_projection)");
        return 2;
    }
    std::vector<HarmonicState> st;
    if ((rc = h_residual(c, T, true, st))) return rc;
    *rel = st[0].bnorm > 0.0 ? st[0].rnorm / st[0].bnorm : st[0].rnorm;
    if (removed) *removed = T.null.removed[0];
    return 0;
}

extern "C" int ec3d_harmonic_null_restarts(ec3d_handle c, int32_t *restarts)
{
    if (!c || !restarts) {
        ec3d_set_error("ec3d_harmonic_null_restarts: null handle or array");
        return 2;
    }
    h_null_restarts(c->harm.one.null, 0, restarts);
    return 0;
}

// ---- a batch of systems in lock step ----------------------------------------------------------
extern "C" int ec3d_harmonic_batch_setup(ec3d_handle c, int32_t nsys, const double *omega)
{
    int rc = h_need(c, "ec3d_harmonic_batch_setup", false);
    if (rc) return rc;
    if (nsys < 0 || nsys > EC3D_HARMONIC_MAX_BATCH) {
        ec3d_set_error("ec3d_harmonic_batch_setup: nsys must be in [0, " + std::to_string(EC3D_HARMONIC_MAX_BATCH) + "]");
        return 2;
    }
    HarmonicSystems &T = c->harm.batch;
    if (nsys == 0) {
        EC3D_HIP(hipStreamSynchronize(c->stream));
        systems_free(T);
        return 0;
    }
    if (!omega) {
        ec3d_set_error("ec3d_harmonic_batch_setup: omega is NULL");
        return 2;
    }
    for (int32_t s = 0; s < nsys; ++s)
        if (!(omega[s] >= 0.0) || !std::isfinite(omega[s])) {
            ec3d_set_error("ec3d_harmonic_batch_setup: omega[" + std::to_string(s) + "] must be finite and not negative");
            return 2;
        }
    EC3D_HIP(hipStreamSynchronize(c->stream));
    std::vector<double> tabs;
    if ((rc = h_tables(c, nsys, omega, tabs))) return rc;
    systems_free(T); // nothing is refused from here on: the batch before goes, whatever its size
    if ((rc = systems_alloc(c, T, nsys))) {
        systems_free(T);
        return rc;
    }
    EC3D_HIP(hipMemcpy(T.tab, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice));
    T.n = nsys;
    for (int32_t s = 0; s < nsys; ++s) {
        T.omega[s] = omega[s];
        T.last[s].ready = 1;
        T.last[s].omega = omega[s];
        T.last[s].device_bytes = T.bytes;
    }
    return 0;
}

extern "C" int ec3d_harmonic_batch_upload(ec3d_handle c, int32_t sys, int which, const double *re, const double *im)
{
    return h_upload(c, "ec3d_harmonic_batch_upload", true, sys, which, re, im);
}

extern "C" int ec3d_harmonic_batch_download(ec3d_handle c, int32_t sys, int which, double *re, double *im)
{
    return h_download(c, "ec3d_harmonic_batch_download", true, sys, which, re, im);
}

extern "C" int ec3d_harmonic_batch_solve(ec3d_handle c, double tol, int32_t itmax, int32_t *iter)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_solve", 0, true);
    if (rc) return rc;
    if (c->harm.one.null.on) {
        ec3d_set_error("ec3d_harmonic_batch_solve: ec3d_harmonic_set_null_projection is on, and its vectors belong to one omega; "
                       "switch it off, or solve the systems one by one (ec3d_harmonic_batch_select)");
        return 2;
    }
    HarmonicSystems &T = c->harm.batch;
    if ((rc = h_solve(c, T, tol, itmax))) return rc;
    for (int s = 0; iter && s < T.n; ++s) iter[s] = T.last[s].iter;
    return 0;
}

extern "C" int ec3d_get_harmonic_batch(ec3d_handle c, int32_t sys, ec3d_harmonic_info *out)
{
    int rc = hb_need(c, "ec3d_get_harmonic_batch", sys, false);
    if (rc) return rc;
    if (!out) {
        ec3d_set_error("ec3d_get_harmonic_batch: info is NULL");
        return 2;
    }
    *out = c->harm.batch.last[sys];
    out->device_bytes += c->harm.batch.null.bytes; // the left null vectors of the batch, while they exist
    return 0;
}

extern "C" int ec3d_harmonic_batch_select(ec3d_handle c, int32_t sys)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_select", sys, false);
    if (rc) return rc;
    const HarmonicSystems &T = c->harm.batch;
    if ((rc = ec3d_harmonic_setup(c, T.omega[sys]))) return rc;
    const size_t bytes = (size_t)c->A.n_pad * sizeof(cplx);
    EC3D_HIP(hipMemcpyAsync(hv(c, HV_X), sysv(c, T, sys, HV_X), bytes, hipMemcpyDeviceToDevice, c->stream));
    EC3D_HIP(hipMemcpyAsync(hv(c, HV_B), sysv(c, T, sys, HV_B), bytes, hipMemcpyDeviceToDevice, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ec3d_harmonic_batch_device_vector(ec3d_handle c, int32_t sys, int which, double **device_ptr, int64_t *pairs)
{
    return h_device_vector(c, "ec3d_harmonic_batch_device_vector", true, sys, which, device_ptr, pairs);
}

// ---- left null vectors inside a batch ----------------------------------------------------------
extern "C" int ec3d_harmonic_batch_set_null_projection(ec3d_handle c, int32_t on, double null_tol)
{
    if (!c) {
        ec3d_set_error("ec3d_harmonic_batch_set_null_projection: null handle");
        return 2;
    }
    if (!on) { // the handle is checked as everywhere; only the batch is not asked for.  The vectors stay with the batch
        const int rc = h_need(c, "ec3d_harmonic_batch_set_null_projection", false);
        if (rc) return rc;
        c->harm.batch.null.on = 0;
        return 0;
    }
    const int rc = hb_need(c, "ec3d_harmonic_batch_set_null_projection", 0, true);
    if (rc) return rc; // (the setting as it was)
    return h_null_switch_on(c, c->harm.batch.null, null_tol);
}

extern "C" int ec3d_get_harmonic_batch_null(ec3d_handle c, int32_t sys, ec3d_null_info *info, int32_t *shares)
{
    int rc = hb_need(c, "ec3d_get_harmonic_batch_null", sys, false);
    if (rc) return rc;
    if (!info) {
        ec3d_set_error("ec3d_get_harmonic_batch_null: info is NULL");
        return 2;
    }
    h_null_info(c->harm.batch.null, sys, info);
    if (shares) *shares = shares_with(c->harm.batch, sys);
    return 0;
}

extern "C" int ec3d_harmonic_batch_left_null_vector(ec3d_handle c, int32_t sys, int32_t index, double *re, double *im)
{
    return h_left_null_vector(c, "ec3d_harmonic_batch_left_null_vector", true, sys, index, re, im);
}

extern "C" int ec3d_harmonic_batch_null_restarts(ec3d_handle c, int32_t sys, int32_t *restarts)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_null_restarts", sys, false);
    if (rc) return rc;
    if (!restarts) {
        ec3d_set_error("ec3d_harmonic_batch_null_restarts: restarts is NULL");
        return 2;
    }
    h_null_restarts(c->harm.batch.null, sys, restarts);
    return 0;
}

extern "C" int ec3d_harmonic_batch_projected_residual(ec3d_handle c, double *rel, double *removed)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_projected_residual", 0, true);
    if (rc) return rc;
    HarmonicSystems &T = c->harm.batch;
    if (!T.null.on || !rel) {
        ec3d_set_error(!rel ? "ec3d_harmonic_batch_projected_residual: rel is NULL"
                            : "ec3d_harmonic_batch_projected_residual: the projection is off "
                              "(ec3d_harmonic_batch_set_null_projection)");
        return 2;
    }
    std::vector<HarmonicState> st;
    if ((rc = h_residual(c, T, true, st))) return rc;
    for (int s = 0; s < T.n; ++s) {
        const HarmonicState &q = st[(size_t)s];
        rel[s] = q.bnorm > 0.0 ? q.rnorm / q.bnorm : q.rnorm;
        if (removed) removed[s] = T.null.removed[s];
    }
    return 0;
}

