// ec3d_harmonic.hip — the time-harmonic A-V solve (K + j omega M) x^ = b^: complex BiCGSTAB with restart on the
// structured form (ec3d_harmonic_*).
//
// Operator.  The class bytes of the real matrix with two tables of their own, made at ec3d_assemble
// (k_build_table_harmonic): re, the transient table without its dt terms, and m, the unit imaginary part;
// ec3d_harmonic_setup interleaves (re, omega * m) into one table of 16 pairs per class, which k_h_spmv holds in LDS.
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
// Iteration `it` (src/solvers.f90:29-49), five launches:
//   k_h_spmv<1>   AP = A P, <R0, AP>
//   k_h_s         alpha = rr0 / <R0, AP>;  S = R - alpha AP, ||S||^2
//   k_h_spmv<2>   AS = A S, <AS, S>, <AS, AS>
//   k_h_xr        ||S|| exit: X = X + alpha P.  Else omega = <AS, S> / <AS, AS>; X = (X + alpha P) + omega S;
//                 R = S - omega AS, ||R||^2, <R0, R>
//   k_h_p         ||R|| exit.  Else beta = (alpha / omega) rr0_new / rr0; restart (R0 = R, P = R, rr0 = ||R||^2) when
//                 |rr0_new| / ||b^|| < tol, else P = R + beta (P - omega AP), rr0 = rr0_new
// The exit words stay on the device: stop_s is written by k_h_xr only, stop_r by k_h_p (and the set-up) only, and a
// kernel never tests at its entry a word that its own launch may write with a value that would change the test --
// k_h_xr of iteration it asks stop_s < it, k_h_p stop_r < it -- so a workgroup that starts late takes the same path as
// workgroup 0.  rr0 alternates between two slots for the same reason.  The host enqueues 16 iterations and polls once.
//
// Left null vectors (opt-in, ec3d_harmonic_set_null_projection).  K + j omega M is singular as the
// transient matrix is: one left null vector per connected conducting component, and every residual keeps w^H r = w^H b^.
// The set-up (null_build) finds them by adjoint solves -- the iteration above around k_h_spmv_h, y = A^H x -- and a solve
// with the setting on takes them out of its initial residual between k_h_spmv<3> and k_h_setup (k_hn_dots,
// k_hn_collapse, k_hn_sub).  tests/harmonic_null_numpy.py restates every line.
//
// Batch (opt-in, ec3d_harmonic_batch_*).  Up to EC3D_HARMONIC_MAX_BATCH systems (omega_s, b^_s, x^_s)
// on the one matrix ride in the five launches of an iteration on a grid of (G, S): the bodies of k_h_s, k_h_xr, k_h_p
// and k_h_setup are __device__ functions, as h_spmv_modes is, and k_hb_* run them on the system blockIdx.y names.  Every
// system keeps the bits of its own single solve; the host copies the S states back once per 16 lock-step iterations.
//
// Left null vectors inside a batch (opt-in, ec3d_harmonic_batch_set_null_projection).  One set of
// vectors per distinct omega of the batch: batch_null_build runs the adjoint solves of all the sets in lock step --
// k_hb_spmv_h and k_hb_xr_at around the batch's own k_hb_s, k_hb_p, k_hb_setup, in the work vectors of the first systems,
// the unknown in a staging vector per set -- and null_build's every step per set; k_hbn_* are k_hn_* with the system as
// one more grid dimension, and batch_launch_project takes every system's own vectors out of its R between k_hb_spmv<3>
// and k_hb_setup.  Every system keeps the bits of its own single projected solve.
#include "ec3d_stream.hpp"

#include <chrono>
#include <cmath>
#include <cstring>

enum { HP_BB = 0, HP_RR, HP_RR0R, HP_RR0I, HP_D1R, HP_D1I, HP_SS, HP_D2R, HP_D2I, HP_D3, HP_NSLOT };

struct HarmonicState {
    double rr0[2][2]; // <R0, R> entering iteration it: rr0[it & 1]
    double alpha[2], omega[2];
    double bnorm, tol;
    double rnorm, snorm; // of the last k_h_p / k_h_xr that got that far
    int stop_s, stop_r;  // INT_MAX while running; the iteration of the ||S|| / ||R|| exit (stop_r = 0: ||b^|| = 0)
    int restarts, pad_;
};

namespace {

typedef stream_d2 cplx; // .x = re, .y = im
static_assert((55 + 9 * EC3D_SAV_MAXDOM) * 16 * sizeof(cplx) + 256 <= 65536, "k_h_spmv: the table of pairs fits 64 KB of LDS");

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

template <int MODE>
__global__ __launch_bounds__(EC3D_THREADS) void k_h_spmv(HSav A, const HarmonicState *st, const cplx *__restrict__ x,
                                                        const cplx *__restrict__ o, cplx *__restrict__ y,
                                                        cplx *__restrict__ r0, cplx *__restrict__ p, int64_t nchunk,
                                                        double *__restrict__ part)
{
    extern __shared__ cplx tbl[];
    __shared__ double lds[12];
    h_spmv_modes<MODE, false>(A, A.table, st, x, o, y, r0, p, nchunk, part, tbl, lds);
}

// y = A^H x in the layout, the modes and the partial slots of k_h_spmv: the adjoint solves of the left null vectors run
// k_h_s, k_h_xr, k_h_p and k_h_setup around it unchanged
template <int MODE>
__global__ __launch_bounds__(EC3D_THREADS) void k_h_spmv_h(HSav A, const HarmonicState *st, const cplx *__restrict__ x,
                                                          const cplx *__restrict__ o, cplx *__restrict__ y,
                                                          cplx *__restrict__ r0, cplx *__restrict__ p, int64_t nchunk,
                                                          double *__restrict__ part)
{
    extern __shared__ cplx tbl[];
    __shared__ double lds[12];
    h_spmv_modes<MODE, true>(A, A.table, st, x, o, y, r0, p, nchunk, part, tbl, lds);
}

// behind k_h_spmv<3>, one workgroup: ||b^||, rr0 = <R0, R> = (||R||^2, 0), the exit words
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

__global__ __launch_bounds__(EC3D_THREADS) void k_h_setup(HarmonicState *st, const double *part, int G, double tol)
{
    __shared__ double lds[8];
    h_setup_body(st, part, G, tol, lds);
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

__global__ __launch_bounds__(EC3D_THREADS) void k_h_s(HarmonicState *st, int it, const cplx *__restrict__ r,
                                                     const cplx *__restrict__ ap, cplx *__restrict__ sv, int64_t n,
                                                     int64_t nchunk, double *__restrict__ part)
{
    __shared__ double lds[8];
    h_s_body(st, it, r, ap, sv, n, nchunk, part, lds);
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

__global__ __launch_bounds__(EC3D_THREADS) void k_h_xr(HarmonicState *st, int it, const cplx *__restrict__ p,
                                                      const cplx *__restrict__ sv, const cplx *__restrict__ as,
                                                      const cplx *__restrict__ r0, cplx *__restrict__ x,
                                                      cplx *__restrict__ r, int64_t n, int64_t nchunk,
                                                      double *__restrict__ part)
{
    __shared__ double lds[16];
    h_xr_body(st, it, p, sv, as, r0, x, r, n, nchunk, part, lds);
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

__global__ __launch_bounds__(EC3D_THREADS) void k_h_p(HarmonicState *st, int it, const cplx *__restrict__ r,
                                                     const cplx *__restrict__ ap, cplx *__restrict__ p,
                                                     cplx *__restrict__ r0, int64_t n, int64_t nchunk,
                                                     const double *__restrict__ part)
{
    __shared__ double lds[12];
    h_p_body(st, it, r, ap, p, r0, n, nchunk, part, lds);
}

// ---- a batch of systems in lock step (ec3d_harmonic_batch_*) -----------------------------------
// blockIdx.y is the system: its state, partials, table and vectors stand `sys` strides further, and the workgroup then
// runs the body of the single kernel.  h_leave and h_collapse index with gridDim.x and blockIdx.x only, so the sums of
// system s are the sums of its own single solve; a stopped system's workgroups return at their first load.
struct HBatch {
    cplx *vec;            // system s, vector w: vec + (s * HV_N + w) * len
    double *part;         // system s: part + s * HP_NSLOT * gridDim.x
    HarmonicState *state; // system s: state + s
    int64_t len;
};
__device__ __forceinline__ cplx *hb_vec(const HBatch &B, int w) { return B.vec + ((int64_t)blockIdx.y * HV_N + w) * B.len; }
__device__ __forceinline__ double *hb_part(const HBatch &B) { return B.part + (int64_t)blockIdx.y * HP_NSLOT * gridDim.x; }

// k_h_spmv<MODE> on system blockIdx.y: st, part and the vectors are system 0's, the next system's stand 1 state,
// HP_NSLOT * gridDim.x partials and `vstride` pairs further; A.table is system 0's table.  The vectors come as arguments
// of their own, __restrict__ as k_h_spmv's: behind one base pointer the same body takes 98 VGPRs instead of 72
template <int MODE>
__global__ __launch_bounds__(EC3D_THREADS) void k_hb_spmv(HSav A, const HarmonicState *st, const cplx *__restrict__ x,
                                                         const cplx *__restrict__ o, cplx *__restrict__ y,
                                                         cplx *__restrict__ r0, cplx *__restrict__ p, int64_t nchunk,
                                                         double *__restrict__ part, int64_t vstride)
{
    static_assert(MODE >= 1 && MODE <= 3, "the batch has the begin launch and the two products of an iteration");
    extern __shared__ cplx tbl[];
    __shared__ double lds[12];
    const int64_t sys = blockIdx.y, v = sys * vstride;
    h_spmv_modes<MODE, false>(A, A.table + sys * A.ncls * 16, st + sys, x + v, MODE == 2 ? nullptr : o + v, y + v,
                              MODE == 3 ? r0 + v : nullptr, MODE == 3 ? p + v : nullptr, nchunk,
                              part + sys * HP_NSLOT * gridDim.x, tbl, lds);
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

__global__ __launch_bounds__(EC3D_THREADS) void k_hb_p(HBatch B, int it, int64_t n, int64_t nchunk)
{
    __shared__ double lds[12];
    h_p_body(B.state + blockIdx.y, it, hb_vec(B, HV_R), hb_vec(B, HV_AP), hb_vec(B, HV_P), hb_vec(B, HV_R0), n, nchunk, hb_part(B),
             lds);
}

// ---- left null vectors: the streaming kernels of the set-up and of the projection -------------
// partials of c_i = <Q_i, v>, Q_i = qbase + i * qstride, i = blockIdx.y: the two parts at part[(2 i + {0, 1}) * G + b]
__global__ __launch_bounds__(EC3D_THREADS) void k_hn_dots(const cplx *__restrict__ qbase, int64_t qstride,
                                                         const cplx *__restrict__ v, int64_t n, int64_t nchunk,
                                                         double *__restrict__ part)
{
    __shared__ double lds[8];
    const cplx *q = qbase + (int64_t)blockIdx.y * qstride;
    double acc[2] = {0.0, 0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx d = cdot(q[i], v[i]);
            acc[0] = acc[0] + d.x;
            acc[1] = acc[1] + d.y;
        }
    h_leave<2>(acc, part, 2 * (int)blockIdx.y, lds);
}

// workgroup i: coef[i] = the two parts of c_i, from `count` partials each
__global__ __launch_bounds__(EC3D_THREADS) void k_hn_collapse(const double *__restrict__ part, int count, cplx *__restrict__ coef)
{
    __shared__ double lds[8];
    double v[2];
    stream_strided_sum<2>(v, part + (int64_t)2 * blockIdx.x * count, count, count);
    stream_block_sum<2>(v, lds);
    if (threadIdx.x == 0) coef[blockIdx.x] = cplx{v[0], v[1]};
}

// v = v - c_0 Q_0 - ... - c_{k-1} Q_{k-1}, every term a rounded cmul and a rounded difference per part; r0, p (or null):
// copies of the new v; rr (or null): workgroup b's partial of ||v||^2 at rr[b], written by EVERY workgroup of the launch
__global__ __launch_bounds__(EC3D_THREADS) void k_hn_sub(const cplx *__restrict__ qbase, int64_t qstride, int k,
                                                        const cplx *__restrict__ coef, cplx *__restrict__ v,
                                                        cplx *__restrict__ r0, cplx *__restrict__ p, int64_t n,
                                                        int64_t nchunk, double *__restrict__ rr)
{
    __shared__ double lds[4];
    double acc[1] = {0.0};
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            cplx x = v[i];
            for (int m = 0; m < k; ++m) {
                const cplx t = cmul(coef[m], qbase[(int64_t)m * qstride + i]);
                x = cplx{x.x - t.x, x.y - t.y};
            }
            v[i] = x;
            if (r0) r0[i] = x;
            if (p) p[i] = x;
            acc[0] = acc[0] + cabs2(x);
        }
    if (!rr) return;
    stream_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) rr[blockIdx.x] = acc[0];
}

// v = v / d on rows < n, each part divided on its own
__global__ __launch_bounds__(EC3D_THREADS) void k_hn_div(cplx *__restrict__ v, double d, int64_t n, int64_t nchunk)
{
    for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x)
        for (int half = 0; half < 2; ++half) {
            const int64_t i = h_row(ch, half);
            if (i >= n) continue;
            const cplx a = v[i];
            v[i] = cplx{a.x / d, a.y / d};
        }
}

// Re v[row] = Re v[row] + a (e_m and -e_m)
__global__ void k_hn_add_re(cplx *v, int64_t row, double a) { v[row].x = v[row].x + a; }

// ---- left null vectors inside a batch ----------------------------------------------------------
// The adjoint solves of the batch's distinct omegas in lock step: `sys` below is a SET of vectors (one per distinct
// omega), which borrows the work vectors, the partials and the state of system `sys` of the batch.
// k_h_spmv_h<MODE> on set blockIdx.y: A.table is set 0's table; st, part, o, y, r0, p are system 0's, `vstride` pairs
// apart; x stands `xstride` pairs apart -- the unknown of the adjoint solves has a vector of its own per set (MODE 3,
// and MODE 0 on w), the work vectors have the batch's stride.  __restrict__ arguments of system 0 plus strides, as
// k_hb_spmv has them.
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

// k_hb_xr with the unknown at x + blockIdx.y * xstride in place of the system's HV_X
__global__ __launch_bounds__(EC3D_THREADS) void k_hb_xr_at(HBatch B, int it, cplx *__restrict__ x, int64_t xstride, int64_t n,
                                                          int64_t nchunk)
{
    __shared__ double lds[16];
    h_xr_body(B.state + blockIdx.y, it, hb_vec(B, HV_P), hb_vec(B, HV_S), hb_vec(B, HV_AS), hb_vec(B, HV_R0),
              x + (int64_t)blockIdx.y * xstride, hb_vec(B, HV_R), n, nchunk, hb_part(B), lds);
}

// The streaming kernels above with the system as one more grid dimension.  System s projects with the vectors of set
// set[s], of which kept[s] exist; a workgroup of a vector past kept[s] returns before it reads or writes anything.
struct HNSys {
    int32_t set[EC3D_HARMONIC_MAX_BATCH], kept[EC3D_HARMONIC_MAX_BATCH];
};
struct HNDiv {
    double d[EC3D_HARMONIC_MAX_BATCH]; // 0: the system is skipped
};

// k_hn_dots on system blockIdx.z: Q_i = qbase + set[s] * qset + i * qstride, v = vbase + s * vstride, the partials at
// part + s * pstride.  h_leave indexes with gridDim.x and blockIdx.x only: the sums are k_hn_dots' own
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

// k_hn_collapse on system blockIdx.y: coef[s * cstride + i]
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

// k_hn_sub on system blockIdx.y with its own kept[s] vectors; r0, p, rr (or null) are system 0's, vstride pairs and
// rrstride doubles apart.  A system that kept nothing is left as it is, partials included
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

// k_hn_div on system blockIdx.y by D.d[s]
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

// k_hn_add_re on system blockIdx.x
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

HSav view_of(const ec3d_ctx *c)
{
    const DevMatrix &A = c->A;
    HSav T;
    T.cls = A.cls;
    T.table = reinterpret_cast<const cplx *>(c->harm.tab.get());
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

cplx *hv(const ec3d_ctx *c, int w) { return reinterpret_cast<cplx *>(c->harm.vec[w]); }

// the operator of a solve: K + j omega M or its conjugate transpose (the adjoint solves of the left null vectors)
enum HOp { H_A = 0, H_AH };

template <int MODE> void launch_spmv(ec3d_ctx *c, HOp op, const cplx *x, const cplx *o, cplx *y, cplx *r0, cplx *p)
{
    const Harmonic &H = c->harm;
    const size_t lds = (size_t)c->A.ncls * 16 * sizeof(cplx);
    if (op == H_A)
        k_h_spmv<MODE><<<(unsigned)H.wgs, EC3D_THREADS, lds, c->stream>>>(view_of(c), H.state, x, o, y, r0, p,
                                                                         c->A.n_pad / EC3D_TILE, H.part);
    else
        k_h_spmv_h<MODE><<<(unsigned)H.wgs, EC3D_THREADS, lds, c->stream>>>(view_of(c), H.state, x, o, y, r0, p,
                                                                           c->A.n_pad / EC3D_TILE, H.part);
}

// c_i = <Q_i, R>; R = R - c_1 Q_1 - ... - c_k Q_k, R0 = R, P = R; the partials of ||R||^2 where k_h_spmv<3> left them
// (HP_RR, one per workgroup of that launch), so k_h_setup reads them unchanged
void launch_project(ec3d_ctx *c)
{
    const Harmonic &H = c->harm;
    if (H.null_kept == 0) return;
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE;
    const cplx *q = reinterpret_cast<const cplx *>(H.nq.get());
    cplx *coef = reinterpret_cast<cplx *>(H.ncoef.get());
    k_hn_dots<<<dim3((unsigned)H.wgs, (unsigned)H.null_kept), EC3D_THREADS, 0, c->stream>>>(q, len, hv(c, HV_R), n, nc, H.npart);
    k_hn_collapse<<<(unsigned)H.null_kept, EC3D_THREADS, 0, c->stream>>>(H.npart, H.wgs, coef);
    k_hn_sub<<<(unsigned)H.wgs, EC3D_THREADS, 0, c->stream>>>(q, len, H.null_kept, coef, hv(c, HV_R), hv(c, HV_R0), hv(c, HV_P), n,
                                                             nc, H.part.get() + (int64_t)HP_RR * H.wgs);
}

// R = b - op x, R0 = R, P = R and the state of a solve that has just begun; project: the left null vectors leave R first
void launch_begin(ec3d_ctx *c, HOp op, const cplx *x, const cplx *b, double tol, bool project)
{
    const Harmonic &H = c->harm;
    launch_spmv<3>(c, op, x, b, hv(c, HV_R), hv(c, HV_R0), hv(c, HV_P));
    if (project) launch_project(c);
    k_h_setup<<<1, EC3D_THREADS, 0, c->stream>>>(H.state, H.part, H.wgs, tol);
}

void launch_iteration(ec3d_ctx *c, HOp op, cplx *x, int it)
{
    const Harmonic &H = c->harm;
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE;
    const unsigned G = (unsigned)H.wgs;
    hipStream_t s = c->stream;
    launch_spmv<1>(c, op, hv(c, HV_P), hv(c, HV_R0), hv(c, HV_AP), nullptr, nullptr);
    k_h_s<<<G, EC3D_THREADS, 0, s>>>(H.state, it, hv(c, HV_R), hv(c, HV_AP), hv(c, HV_S), n, nc, H.part);
    launch_spmv<2>(c, op, hv(c, HV_S), nullptr, hv(c, HV_AS), nullptr, nullptr);
    k_h_xr<<<G, EC3D_THREADS, 0, s>>>(H.state, it, hv(c, HV_P), hv(c, HV_S), hv(c, HV_AS), hv(c, HV_R0), x, hv(c, HV_R), n, nc,
                                     H.part);
    k_h_p<<<G, EC3D_THREADS, 0, s>>>(H.state, it, hv(c, HV_R), hv(c, HV_AP), hv(c, HV_P), hv(c, HV_R0), n, nc, H.part);
}

// itmax + 1 iterations at most (src/solvers.f90:25-29) behind a launch_begin, 16 enqueued per poll; st: the state at the
// last poll.  *stopped: an exit was taken
int run_iterations(ec3d_ctx *c, HOp op, cplx *x, int64_t itmax, HarmonicState &st, bool *stopped)
{
    const int64_t total = itmax + 1;
    int64_t launched = 0;
    *stopped = false;
    do {
        const int64_t m = std::min<int64_t>(16, total - launched);
        for (int64_t i = 0; i < m; ++i) launch_iteration(c, op, x, (int)(++launched));
        EC3D_HIP(hipGetLastError());
        EC3D_HIP(hipMemcpyAsync(&st, c->harm.state, sizeof st, hipMemcpyDeviceToHost, c->stream));
        EC3D_HIP(hipStreamSynchronize(c->stream));
        *stopped = st.stop_s != INT_MAX || st.stop_r != INT_MAX;
    } while (launched < total && !*stopped);
    return 0;
}

// iter, restarts, stop_kind and relres of a solve from its last state; total = itmax + 1 iterations were allowed
void h_report(ec3d_harmonic_info &o, const HarmonicState &st, bool stopped, int64_t total)
{
    o.iter = stopped ? std::min(st.stop_s, st.stop_r) : (int32_t)std::max<int64_t>(total, 0);
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
    if (ready && !c->harm.ready) {
        ec3d_set_error(std::string(who) + ": call ec3d_harmonic_setup first");
        return 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    return 0;
}

// the (re, omega m) pairs of one operator from the two tables of ec3d_assemble
std::vector<double> h_table(const std::vector<double> &re, const std::vector<double> &m, double omega)
{
    std::vector<double> tab(2 * re.size());
    for (size_t q = 0; q < re.size(); ++q) {
        tab[2 * q] = re[q];
        tab[2 * q + 1] = omega * m[q]; // one rounding per entry
    }
    return tab;
}

int h_which(int which, const char *who)
{
    if (which == EC3D_VEC_X || which == EC3D_VEC_B) return 0;
    ec3d_set_error(std::string(who) + ": which must be EC3D_VEC_X or EC3D_VEC_B");
    return 2;
}

// stage: 2 * n_pad doubles of staging, the single solve's (H.stage) or the batch's (H.bstage)
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

// sum over the rows of <a, v>'s terms (a == v: ||v||^2 in the real part), read back: one k_hn_dots and one collapse
int dot_to_host(ec3d_ctx *c, const cplx *a, const cplx *v, double *re)
{
    Harmonic &H = c->harm;
    cplx *coef = reinterpret_cast<cplx *>(H.ncoef.get());
    k_hn_dots<<<dim3((unsigned)H.wgs, 1), EC3D_THREADS, 0, c->stream>>>(a, 0, v, c->A.n, c->A.n_pad / EC3D_TILE, H.npart);
    k_hn_collapse<<<1, EC3D_THREADS, 0, c->stream>>>(H.npart, H.wgs, coef);
    EC3D_HIP(hipGetLastError());
    double h[2];
    EC3D_HIP(hipMemcpyAsync(h, coef, sizeof h, hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    *re = h[0];
    return 0;
}

// The set-up of ec3d_harmonic_set_null_projection, once per matrix and omega.  Per connected conducting component
// (ec3d_null_seeds): c = A^H (-e_m) into AS by one launch (-e_m in S); the adjoint solve A^H y = c from y = 0 -- this
// file's iteration around k_h_spmv_h, y in the next free slot of Q, in the work vectors R, R0, P, AP, S, AS and the
// state, which nothing reads between two solves; X^ and B^ are not touched -- then w = y + e_m, ||A^H w|| / ||w||, and
// classical Gram-Schmidt against the vectors kept.
int null_build(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    const auto t_start = std::chrono::steady_clock::now();
    ec3d_harmonic_null_free(c);
    EC3D_HIP(hipStreamSynchronize(c->stream));
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE;
    std::vector<NullSeed> seeds;
    int rc = ec3d_null_seeds(c, seeds);
    if (rc) return rc;
    const int ncomp = (int)seeds.size();
    ec3d_null_info &L = H.null_last;
    L.found = ncomp;
    L.reported = std::min(ncomp, EC3D_NULL_MAX_REPORT);
    if (ncomp == 0) { // no conductor: the operator has no such null vector, the projection is the identity
        H.null_built = true;
        return 0;
    }
    EC3D_HIP(H.nq.alloc((size_t)ncomp * 2 * len));
    EC3D_HIP(hipMemsetAsync(H.nq, 0, (size_t)ncomp * 2 * len * sizeof(double), c->stream));
    EC3D_HIP(H.npart.alloc((size_t)2 * ncomp * H.wgs));
    EC3D_HIP(H.ncoef.alloc((size_t)2 * ncomp));
    H.null_bytes = (int64_t)(((size_t)ncomp * 2 * len + (size_t)2 * ncomp * H.wgs + (size_t)2 * ncomp) * sizeof(double));
    cplx *Q = reinterpret_cast<cplx *>(H.nq.get()), *coef = reinterpret_cast<cplx *>(H.ncoef.get());
    const int64_t cap = (int64_t)(20.0 * std::cbrt((double)c->n_ref)) + 2000;
    const unsigned G = (unsigned)H.wgs;
    int kept = 0;
    for (int ci = 0; ci < ncomp; ++ci) {
        const int64_t row = seeds[(size_t)ci].row;
        cplx *w = Q + (size_t)kept * len; // the next free slot: y, then w, then Q_kept
        EC3D_HIP(hipMemsetAsync(hv(c, HV_S), 0, (size_t)n * sizeof(cplx), c->stream));
        k_hn_add_re<<<1, 1, 0, c->stream>>>(hv(c, HV_S), row, -1.0);
        launch_spmv<0>(c, H_AH, hv(c, HV_S), nullptr, hv(c, HV_AS), nullptr, nullptr);
        launch_begin(c, H_AH, w, hv(c, HV_AS), H.null_tol, false);
        EC3D_HIP(hipGetLastError());
        HarmonicState st;
        bool stopped = false;
        if ((rc = run_iterations(c, H_AH, w, cap, st, &stopped))) return rc;
        k_hn_add_re<<<1, 1, 0, c->stream>>>(w, row, 1.0);
        // c - A^H y = -A^H w: ||A^H w|| is the adjoint system's TRUE residual, and the figure of the report
        double aw2 = 0.0, w2 = 0.0;
        launch_spmv<0>(c, H_AH, w, nullptr, hv(c, HV_AS), nullptr, nullptr);
        if ((rc = dot_to_host(c, hv(c, HV_AS), hv(c, HV_AS), &aw2))) return rc;
        if ((rc = dot_to_host(c, w, w, &w2))) return rc;
        // A w that missed null_tol is never used.  Missed: no exit within the cap, or an exit of the recurrence that the
        // true residual does not bear out.  The exits bound the recurrence's residual by null_tol ||c||; the true one
        // differs from it by the rounding gathered along the solve, some 1e-14 ||c|| and far below any null_tol the
        // arithmetic can deliver, so twice the bound tells a solve that delivered from a recurrence that ran away.
        const double true_rel = std::sqrt(aw2) / st.bnorm;
        if (!stopped || !(true_rel <= 2.0 * H.null_tol)) {
            char msg[400];
            snprintf(msg, sizeof msg, "harmonic null projection: the adjoint solve of conducting component %d (seed row %lld) did "
                     "not reach null_tol = %.3g: %s after %lld iterations (cap %lld), true residual ||A^H w|| / ||A^H e_m|| = %.3g; "
                     "its left null vector is not used", ci, (long long)seeds[(size_t)ci].seed_ref, H.null_tol,
                     stopped ? "the recurrence took an exit" : "no exit",
                     (long long)(stopped ? std::min(st.stop_s, st.stop_r) : cap + 1), (long long)cap, true_rel);
            ec3d_harmonic_null_free(c);
            ec3d_set_error(msg);
            return EC3D_NULL_E_SETUP;
        }
        const double n0 = std::sqrt(w2), res = std::sqrt(aw2) / n0;
        if (kept > 0) {
            k_hn_dots<<<dim3(G, (unsigned)kept), EC3D_THREADS, 0, c->stream>>>(Q, len, w, n, nc, H.npart);
            k_hn_collapse<<<(unsigned)kept, EC3D_THREADS, 0, c->stream>>>(H.npart, H.wgs, coef);
            k_hn_sub<<<G, EC3D_THREADS, 0, c->stream>>>(Q, len, kept, coef, w, nullptr, nullptr, n, nc, nullptr);
            if ((rc = dot_to_host(c, w, w, &w2))) return rc;
        }
        const double n1 = std::sqrt(w2);
        const bool keep = std::isfinite(n0) && std::isfinite(n1) && n1 > EC3D_NULL_MIN_KEEP * n0;
        if (keep) {
            k_hn_div<<<G, EC3D_THREADS, 0, c->stream>>>(w, n1, n, nc);
            ++kept;
        } else {
            EC3D_HIP(hipMemsetAsync(w, 0, (size_t)len * sizeof(cplx), c->stream)); // the slot is free again
        }
        if (ci < EC3D_NULL_MAX_REPORT) {
            L.seed_row[ci] = seeds[(size_t)ci].seed_ref;
            L.iterations[ci] = std::min(st.stop_s, st.stop_r);
            L.was_kept[ci] = keep ? 1 : 0;
            L.residual[ci] = res;
            H.null_restarts[ci] = st.restarts;
        }
    }
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipStreamSynchronize(c->stream));
    H.null_kept = kept;
    H.null_built = true;
    L.kept = kept;
    L.dropped = ncomp - kept;
    L.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return 0;
}

// removed = sqrt(sum |c_i|^2) / ||b^|| of the projection that has just run: one copy of the coefficients
int null_note(ec3d_ctx *c, double bnorm)
{
    Harmonic &H = c->harm;
    H.null_last.removed = 0.0;
    if (H.null_kept == 0 || bnorm == 0.0) return 0;
    std::vector<double> h((size_t)2 * H.null_kept);
    EC3D_HIP(hipMemcpy(h.data(), H.ncoef, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    double s = 0.0;
    for (size_t i = 0; i < h.size(); i += 2) s += h[i] * h[i] + h[i + 1] * h[i + 1];
    H.null_last.removed = std::sqrt(s) / bnorm;
    return 0;
}

// ---- the batch ---------------------------------------------------------------------------------
HBatch batch_of(const ec3d_ctx *c)
{
    const Harmonic &H = c->harm;
    HBatch B;
    B.vec = reinterpret_cast<cplx *>(H.bvec.get());
    B.part = H.bpart.get();
    B.state = H.bstate.get();
    B.len = c->A.n_pad;
    return B;
}

// the matrix with system 0's table of the batch
HSav batch_view_of(const ec3d_ctx *c)
{
    HSav T = view_of(c);
    T.table = reinterpret_cast<const cplx *>(c->harm.btab.get());
    return T;
}

cplx *hbv(const ec3d_ctx *c, int sys, int w)
{
    return reinterpret_cast<cplx *>(c->harm.bvec.get()) + ((size_t)sys * HV_N + (size_t)w) * (size_t)c->A.n_pad;
}

// the vectors of ec3d_harmonic_batch_set_null_projection and what was reported of them; the setting stays
void batch_null_free(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    H.bnq.reset();
    H.bny.reset();
    H.bntab.reset();
    H.bnpart.reset();
    H.bncoef.reset();
    H.bnull_built = false;
    H.bnsets = 0;
    H.bncomp = 0;
    H.bnull_bytes = 0;
    H.bnull_setup_ms = 0.0;
    for (int s = 0; s < EC3D_HARMONIC_MAX_BATCH; ++s) {
        H.bnset_of[s] = H.bnfirst[s] = H.bnkept[s] = 0;
        H.bnremoved[s] = 0.0;
        H.bnull_last[s] = ec3d_null_info{};
        for (auto &r : H.bnull_restarts[s]) r = 0;
    }
}

void batch_free(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    batch_null_free(c);
    H.bvec.reset();
    H.btab.reset();
    H.bpart.reset();
    H.bstage.reset();
    H.bstate.reset();
    H.bn = 0;
    H.bwgs = 0;
    H.bbytes = 0;
    for (auto &o : H.bomega) o = 0.0;
    for (auto &l : H.blast) l = ec3d_harmonic_info{};
}

// everything of a batch of S systems; the caller frees the batch when this fails
int batch_alloc(ec3d_ctx *c, int S, const std::vector<double> &tabs)
{
    Harmonic &H = c->harm;
    const size_t nt = (size_t)c->A.ncls * 16, len = (size_t)c->A.n_pad;
    const int G = ec3d_stream_wgs((int64_t)len);
    EC3D_HIP(H.bvec.alloc((size_t)S * HV_N * 2 * len));
    EC3D_HIP(H.btab.alloc((size_t)S * 2 * nt));
    EC3D_HIP(H.bpart.alloc((size_t)S * HP_NSLOT * G));
    EC3D_HIP(H.bstage.alloc(2 * len));
    EC3D_HIP(H.bstate.alloc((size_t)S));
    EC3D_HIP(hipMemsetAsync(H.bvec, 0, (size_t)S * HV_N * 2 * len * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(H.bpart, 0, (size_t)S * HP_NSLOT * G * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(H.bstage, 0, 2 * len * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(H.bstate, 0, (size_t)S * sizeof(HarmonicState), c->stream));
    EC3D_HIP(hipMemcpy(H.btab, tabs.data(), (size_t)S * 2 * nt * sizeof(double), hipMemcpyHostToDevice));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    H.bwgs = G;
    H.bbytes = (int64_t)(((size_t)S * HV_N * 2 * len + (size_t)S * 2 * nt + (size_t)S * HP_NSLOT * G + 2 * len) * sizeof(double) +
                         (size_t)S * sizeof(HarmonicState));
    return 0;
}

// h_need and: a batch exists, sys is one of its systems (sys < 0: not asked)
int hb_need(ec3d_ctx *c, const char *who, int32_t sys, bool any_sys)
{
    int rc = h_need(c, who, false);
    if (rc) return rc;
    const Harmonic &H = c->harm;
    if (H.bn == 0) {
        ec3d_set_error(std::string(who) + ": call ec3d_harmonic_batch_setup first");
        return 2;
    }
    if (!any_sys && (sys < 0 || sys >= H.bn)) {
        ec3d_set_error(std::string(who) + ": system " + std::to_string(sys) + " is outside the batch of " + std::to_string(H.bn));
        return 2;
    }
    return 0;
}

// launch_project for every system of the batch: c_{s,i} = <Q_{s,i}, R_s>; R_s = R_s - sum_i c_{s,i} Q_{s,i}, R0 = P = R; the
// partials of ||R_s||^2 in system s's HP_RR slots, where k_hb_spmv<3> left them and k_hb_setup reads them
void batch_launch_project(ec3d_ctx *c)
{
    const Harmonic &H = c->harm;
    HNSys M{};
    int kmax = 0;
    for (int s = 0; s < H.bn; ++s) {
        M.set[s] = H.bnset_of[s];
        M.kept[s] = H.bnkept[H.bnset_of[s]];
        kmax = std::max(kmax, M.kept[s]);
    }
    if (kmax == 0) return;
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE, vs = (int64_t)HV_N * len;
    const unsigned G = (unsigned)H.bwgs, S = (unsigned)H.bn;
    const int64_t pstride = (int64_t)2 * H.bncomp * H.bwgs, cstride = H.bncomp;
    const cplx *q = reinterpret_cast<const cplx *>(H.bnq.get());
    cplx *coef = reinterpret_cast<cplx *>(H.bncoef.get());
    k_hbn_dots<<<dim3(G, (unsigned)kmax, S), EC3D_THREADS, 0, c->stream>>>(M, q, (int64_t)H.bncomp * len, len, hbv(c, 0, HV_R), vs, n,
                                                                          nc, H.bnpart, pstride);
    k_hbn_collapse<<<dim3((unsigned)kmax, S), EC3D_THREADS, 0, c->stream>>>(M, H.bnpart, pstride, H.bwgs, coef, cstride);
    k_hbn_sub<<<dim3(G, S), EC3D_THREADS, 0, c->stream>>>(M, q, (int64_t)H.bncomp * len, len, coef, cstride, hbv(c, 0, HV_R),
                                                         hbv(c, 0, HV_R0), hbv(c, 0, HV_P), vs, n, nc,
                                                         H.bpart.get() + (int64_t)HP_RR * H.bwgs, (int64_t)HP_NSLOT * H.bwgs);
}

// project: every system's left null vectors leave its R first
void batch_launch_begin(ec3d_ctx *c, double tol, bool project)
{
    const Harmonic &H = c->harm;
    const dim3 grid((unsigned)H.bwgs, (unsigned)H.bn);
    const size_t lds = (size_t)c->A.ncls * 16 * sizeof(cplx);
    const HBatch B = batch_of(c);
    k_hb_spmv<3><<<grid, EC3D_THREADS, lds, c->stream>>>(batch_view_of(c), B.state, hbv(c, 0, HV_X), hbv(c, 0, HV_B), hbv(c, 0, HV_R),
                                                         hbv(c, 0, HV_R0), hbv(c, 0, HV_P), c->A.n_pad / EC3D_TILE, B.part,
                                                         (int64_t)HV_N * B.len);
    if (project) batch_launch_project(c);
    k_hb_setup<<<dim3(1, (unsigned)H.bn), EC3D_THREADS, 0, c->stream>>>(B, H.bwgs, tol);
}

// one lock-step iteration: the five launches of launch_iteration, every system in each
void batch_launch_iteration(ec3d_ctx *c, int it)
{
    const Harmonic &H = c->harm;
    const dim3 grid((unsigned)H.bwgs, (unsigned)H.bn);
    const size_t lds = (size_t)c->A.ncls * 16 * sizeof(cplx);
    const int64_t n = c->A.n, nc = c->A.n_pad / EC3D_TILE;
    const HBatch B = batch_of(c);
    const HSav A = batch_view_of(c);
    const int64_t vs = (int64_t)HV_N * B.len;
    hipStream_t s = c->stream;
    k_hb_spmv<1><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, hbv(c, 0, HV_P), hbv(c, 0, HV_R0), hbv(c, 0, HV_AP), nullptr, nullptr, nc,
                                                 B.part, vs);
    k_hb_s<<<grid, EC3D_THREADS, 0, s>>>(B, it, n, nc);
    k_hb_spmv<2><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, hbv(c, 0, HV_S), nullptr, hbv(c, 0, HV_AS), nullptr, nullptr, nc, B.part, vs);
    k_hb_xr<<<grid, EC3D_THREADS, 0, s>>>(B, it, n, nc);
    k_hb_p<<<grid, EC3D_THREADS, 0, s>>>(B, it, n, nc);
}

// run_iterations for a batch: 16 lock-step iterations per poll, all the states in one copy, on while any system runs
int batch_run_iterations(ec3d_ctx *c, int64_t itmax, std::vector<HarmonicState> &st)
{
    const Harmonic &H = c->harm;
    const int64_t total = itmax + 1;
    int64_t launched = 0;
    bool running;
    st.resize((size_t)H.bn);
    do {
        const int64_t m = std::min<int64_t>(16, total - launched);
        for (int64_t i = 0; i < m; ++i) batch_launch_iteration(c, (int)(++launched));
        EC3D_HIP(hipGetLastError());
        EC3D_HIP(hipMemcpyAsync(st.data(), H.bstate, st.size() * sizeof(HarmonicState), hipMemcpyDeviceToHost, c->stream));
        EC3D_HIP(hipStreamSynchronize(c->stream));
        running = false;
        for (const HarmonicState &q : st) running = running || (q.stop_s == INT_MAX && q.stop_r == INT_MAX);
    } while (launched < total && running);
    return 0;
}

// ---- left null vectors inside a batch ----------------------------------------------------------
// the lowest system whose omega has the bits of system s's
int batch_shares_with(const Harmonic &H, int s)
{
    for (int t = 0; t < s; ++t)
        if (std::memcmp(&H.bomega[t], &H.bomega[s], sizeof(double)) == 0) return t;
    return s;
}

// out[d] = the real part of sum <a_d, v_d> over the rows, d < D: a_d = a + d * astride, v_d = v + d * vstride
int batch_dots_to_host(ec3d_ctx *c, int D, const cplx *a, int64_t astride, const cplx *v, int64_t vstride, double *out)
{
    Harmonic &H = c->harm;
    HNSys M{};
    for (int d = 0; d < D; ++d) {
        M.set[d] = d;
        M.kept[d] = 1;
    }
    const int64_t pstride = (int64_t)2 * H.bncomp * H.bwgs, cstride = H.bncomp;
    cplx *coef = reinterpret_cast<cplx *>(H.bncoef.get());
    k_hbn_dots<<<dim3((unsigned)H.bwgs, 1, (unsigned)D), EC3D_THREADS, 0, c->stream>>>(M, a, astride, 0, v, vstride, c->A.n,
                                                                                     c->A.n_pad / EC3D_TILE, H.bnpart, pstride);
    k_hbn_collapse<<<dim3(1, (unsigned)D), EC3D_THREADS, 0, c->stream>>>(M, H.bnpart, pstride, H.bwgs, coef, cstride);
    EC3D_HIP(hipGetLastError());
    std::vector<double> h((size_t)2 * cstride * D);
    EC3D_HIP(hipMemcpyAsync(h.data(), coef, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    for (int d = 0; d < D; ++d) out[d] = h[(size_t)2 * cstride * d];
    return 0;
}

// null_build for the batch: per conducting component the adjoint solves of the D distinct omegas in lock step -- set d
// in the work vectors R, R0, P, AP, S, AS, the partials and the state of system d, its unknown in bny + d * n_pad; X^
// and B^ of no system are touched -- then every step of null_build per set, the decisions on the host from one copy of
// D figures.  A kept vector is copied from the staging vector into its slot of Q: a copy keeps the bits.
int batch_null_build(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    const auto t_start = std::chrono::steady_clock::now();
    batch_null_free(c);
    EC3D_HIP(hipStreamSynchronize(c->stream));
    const int64_t n = c->A.n, len = c->A.n_pad, nc = len / EC3D_TILE, vs = (int64_t)HV_N * len;
    int D = 0;
    for (int s = 0; s < H.bn; ++s) {
        const int f = batch_shares_with(H, s);
        if (f == s) {
            H.bnfirst[D] = s;
            H.bnset_of[s] = D++;
        } else {
            H.bnset_of[s] = H.bnset_of[f];
        }
    }
    H.bnsets = D;
    std::vector<NullSeed> seeds;
    int rc = ec3d_null_seeds(c, seeds);
    if (rc) return rc;
    const int ncomp = (int)seeds.size();
    for (int d = 0; d < D; ++d) {
        H.bnull_last[d].found = ncomp;
        H.bnull_last[d].reported = std::min(ncomp, EC3D_NULL_MAX_REPORT);
    }
    if (ncomp == 0) { // no conductor: the projection is the identity
        H.bnull_built = true;
        return 0;
    }
    const size_t nt = (size_t)c->A.ncls * 16;
    const int G = H.bwgs;
    EC3D_HIP(H.bnq.alloc((size_t)D * ncomp * 2 * len));
    EC3D_HIP(H.bny.alloc((size_t)D * 2 * len));
    EC3D_HIP(H.bntab.alloc((size_t)D * 2 * nt));
    EC3D_HIP(H.bnpart.alloc((size_t)H.bn * 2 * ncomp * G));
    EC3D_HIP(H.bncoef.alloc((size_t)H.bn * 2 * ncomp));
    EC3D_HIP(hipMemsetAsync(H.bnq, 0, (size_t)D * ncomp * 2 * len * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(H.bnpart, 0, (size_t)H.bn * 2 * ncomp * G * sizeof(double), c->stream));
    EC3D_HIP(hipMemsetAsync(H.bncoef, 0, (size_t)H.bn * 2 * ncomp * sizeof(double), c->stream));
    {
        std::vector<double> re(nt), m(nt), tabs;
        EC3D_HIP(hipMemcpy(re.data(), H.re, nt * sizeof(double), hipMemcpyDeviceToHost));
        EC3D_HIP(hipMemcpy(m.data(), H.m, nt * sizeof(double), hipMemcpyDeviceToHost));
        for (int d = 0; d < D; ++d) {
            const std::vector<double> t = h_table(re, m, H.bomega[H.bnfirst[d]]);
            tabs.insert(tabs.end(), t.begin(), t.end());
        }
        EC3D_HIP(hipMemcpy(H.bntab, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    H.bncomp = ncomp;
    const int64_t nbytes = (int64_t)(((size_t)D * ncomp * 2 * len + (size_t)D * 2 * len + (size_t)D * 2 * nt +
                                      (size_t)H.bn * 2 * ncomp * G + (size_t)H.bn * 2 * ncomp) * sizeof(double));
    cplx *Q = reinterpret_cast<cplx *>(H.bnq.get()), *Y = reinterpret_cast<cplx *>(H.bny.get());
    cplx *coef = reinterpret_cast<cplx *>(H.bncoef.get());
    const int64_t cap = (int64_t)(20.0 * std::cbrt((double)c->n_ref)) + 2000, total = cap + 1;
    const int64_t pstride = (int64_t)2 * ncomp * G, cstride = ncomp, qset = (int64_t)ncomp * len;
    const dim3 grid((unsigned)G, (unsigned)D);
    const size_t lds = nt * sizeof(cplx);
    const HBatch B = batch_of(c);
    HSav A = view_of(c);
    A.table = reinterpret_cast<const cplx *>(H.bntab.get());
    hipStream_t s = c->stream;
    std::vector<HarmonicState> st((size_t)D);
    std::vector<double> aw2((size_t)D), w2((size_t)D), w2b((size_t)D);
    for (int ci = 0; ci < ncomp; ++ci) {
        const int64_t row = seeds[(size_t)ci].row;
        for (int d = 0; d < D; ++d) EC3D_HIP(hipMemsetAsync(hbv(c, d, HV_S), 0, (size_t)n * sizeof(cplx), s));
        k_hbn_add_re<<<(unsigned)D, 1, 0, s>>>(hbv(c, 0, HV_S), vs, row, -1.0);
        k_hb_spmv_h<0><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, hbv(c, 0, HV_S), nullptr, hbv(c, 0, HV_AS), nullptr, nullptr, nc,
                                                       B.part, vs, vs);
        EC3D_HIP(hipMemsetAsync(Y, 0, (size_t)D * len * sizeof(cplx), s));
        k_hb_spmv_h<3><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, Y, hbv(c, 0, HV_AS), hbv(c, 0, HV_R), hbv(c, 0, HV_R0),
                                                       hbv(c, 0, HV_P), nc, B.part, vs, len);
        k_hb_setup<<<dim3(1, (unsigned)D), EC3D_THREADS, 0, s>>>(B, G, H.bnull_tol);
        EC3D_HIP(hipGetLastError());
        int64_t launched = 0;
        bool running;
        do { // run_iterations, D adjoint solves in each launch
            const int64_t m = std::min<int64_t>(16, total - launched);
            for (int64_t i = 0; i < m; ++i) {
                const int it = (int)(++launched);
                k_hb_spmv_h<1><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, hbv(c, 0, HV_P), hbv(c, 0, HV_R0), hbv(c, 0, HV_AP), nullptr,
                                                               nullptr, nc, B.part, vs, vs);
                k_hb_s<<<grid, EC3D_THREADS, 0, s>>>(B, it, n, nc);
                k_hb_spmv_h<2><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, hbv(c, 0, HV_S), nullptr, hbv(c, 0, HV_AS), nullptr, nullptr,
                                                               nc, B.part, vs, vs);
                k_hb_xr_at<<<grid, EC3D_THREADS, 0, s>>>(B, it, Y, len, n, nc);
                k_hb_p<<<grid, EC3D_THREADS, 0, s>>>(B, it, n, nc);
            }
            EC3D_HIP(hipGetLastError());
            EC3D_HIP(hipMemcpyAsync(st.data(), H.bstate, st.size() * sizeof(HarmonicState), hipMemcpyDeviceToHost, s));
            EC3D_HIP(hipStreamSynchronize(s));
            running = false;
            for (const HarmonicState &q : st) running = running || (q.stop_s == INT_MAX && q.stop_r == INT_MAX);
        } while (launched < total && running);
        k_hbn_add_re<<<(unsigned)D, 1, 0, s>>>(Y, len, row, 1.0);
        // ||A^H w||, the adjoint system's true residual, and ||w||, per set
        k_hb_spmv_h<0><<<grid, EC3D_THREADS, lds, s>>>(A, B.state, Y, nullptr, hbv(c, 0, HV_AS), nullptr, nullptr, nc, B.part, vs, len);
        if ((rc = batch_dots_to_host(c, D, hbv(c, 0, HV_AS), vs, hbv(c, 0, HV_AS), vs, aw2.data()))) return rc;
        if ((rc = batch_dots_to_host(c, D, Y, len, Y, len, w2.data()))) return rc;
        for (int d = 0; d < D; ++d) { // the rule of null_build, per set
            const HarmonicState &q = st[(size_t)d];
            const bool stopped = q.stop_s != INT_MAX || q.stop_r != INT_MAX;
            const double true_rel = std::sqrt(aw2[(size_t)d]) / q.bnorm;
            if (stopped && true_rel <= 2.0 * H.bnull_tol) continue;
            char msg[480];
            snprintf(msg, sizeof msg, "harmonic batch null projection: the adjoint solve of system %d (omega = %.17g), conducting "
                     "component %d (seed row %lld) did not reach null_tol = %.3g: %s after %lld iterations (cap %lld), true residual "
                     "||A^H w|| / ||A^H e_m|| = %.3g; no left null vector of the batch is used", H.bnfirst[d],
                     H.bomega[H.bnfirst[d]], ci, (long long)seeds[(size_t)ci].seed_ref, H.bnull_tol,
                     stopped ? "the recurrence took an exit" : "no exit",
                     (long long)(stopped ? std::min(q.stop_s, q.stop_r) : cap + 1), (long long)cap, true_rel);
            batch_null_free(c);
            ec3d_set_error(msg);
            return EC3D_NULL_E_SETUP;
        }
        HNSys K{};
        int kmax = 0;
        for (int d = 0; d < D; ++d) {
            K.set[d] = d;
            K.kept[d] = H.bnkept[d];
            kmax = std::max(kmax, K.kept[d]);
        }
        w2b = w2;
        if (kmax > 0) {
            k_hbn_dots<<<dim3((unsigned)G, (unsigned)kmax, (unsigned)D), EC3D_THREADS, 0, s>>>(K, Q, qset, len, Y, len, n, nc, H.bnpart,
                                                                                             pstride);
            k_hbn_collapse<<<dim3((unsigned)kmax, (unsigned)D), EC3D_THREADS, 0, s>>>(K, H.bnpart, pstride, G, coef, cstride);
            k_hbn_sub<<<grid, EC3D_THREADS, 0, s>>>(K, Q, qset, len, coef, cstride, Y, nullptr, nullptr, len, n, nc, nullptr, 0);
            std::vector<double> after((size_t)D);
            if ((rc = batch_dots_to_host(c, D, Y, len, Y, len, after.data()))) return rc;
            for (int d = 0; d < D; ++d)
                if (K.kept[d] > 0) w2b[(size_t)d] = after[(size_t)d];
        }
        HNDiv dv{};
        bool keep[EC3D_HARMONIC_MAX_BATCH] = {false};
        for (int d = 0; d < D; ++d) {
            const double n0 = std::sqrt(w2[(size_t)d]), n1 = std::sqrt(w2b[(size_t)d]);
            keep[d] = std::isfinite(n0) && std::isfinite(n1) && n1 > EC3D_NULL_MIN_KEEP * n0;
            dv.d[d] = keep[d] ? n1 : 0.0;
        }
        k_hbn_div<<<grid, EC3D_THREADS, 0, s>>>(dv, Y, len, n, nc);
        for (int d = 0; d < D; ++d) {
            if (keep[d]) {
                EC3D_HIP(hipMemcpyAsync(Q + (size_t)d * qset + (size_t)H.bnkept[d] * len, Y + (size_t)d * len, (size_t)len * sizeof(cplx),
                                        hipMemcpyDeviceToDevice, s));
                ++H.bnkept[d];
            }
            if (ci < EC3D_NULL_MAX_REPORT) {
                ec3d_null_info &L = H.bnull_last[d];
                const HarmonicState &q = st[(size_t)d];
                L.seed_row[ci] = seeds[(size_t)ci].seed_ref;
                L.iterations[ci] = std::min(q.stop_s, q.stop_r);
                L.was_kept[ci] = keep[d] ? 1 : 0;
                L.residual[ci] = std::sqrt(aw2[(size_t)d]) / std::sqrt(w2[(size_t)d]);
                H.bnull_restarts[d][ci] = q.restarts;
            }
        }
    }
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipStreamSynchronize(s));
    H.bnull_built = true;
    H.bnull_bytes = nbytes;
    H.bnull_setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    for (int d = 0; d < D; ++d) {
        H.bnull_last[d].kept = H.bnkept[d];
        H.bnull_last[d].dropped = ncomp - H.bnkept[d];
        H.bnull_last[d].setup_ms = H.bnull_setup_ms;
    }
    return 0;
}

// null_note per system: removed_s = sqrt(sum_i |c_{s,i}|^2) / ||b^_s|| of the projection that has just run
int batch_null_note(ec3d_ctx *c, const std::vector<HarmonicState> &st)
{
    Harmonic &H = c->harm;
    for (int s = 0; s < H.bn; ++s) H.bnremoved[s] = 0.0;
    if (H.bncomp == 0) return 0;
    std::vector<double> h((size_t)H.bn * 2 * H.bncomp);
    EC3D_HIP(hipMemcpy(h.data(), H.bncoef, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < H.bn; ++s) {
        const int kept = H.bnkept[H.bnset_of[s]];
        const double bnorm = st[(size_t)s].bnorm;
        if (kept == 0 || bnorm == 0.0) continue;
        const double *q = h.data() + (size_t)s * 2 * H.bncomp;
        double sum = 0.0;
        for (int i = 0; i < 2 * kept; i += 2) sum += q[i] * q[i] + q[i + 1] * q[i + 1];
        H.bnremoved[s] = std::sqrt(sum) / bnorm;
    }
    return 0;
}

} // namespace

void ec3d_harmonic_null_free(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    H.nq.reset();
    H.npart.reset();
    H.ncoef.reset();
    H.null_built = false;
    H.null_kept = 0;
    H.null_bytes = 0;
    H.null_last = ec3d_null_info{};
    for (auto &r : H.null_restarts) r = 0;
}

void ec3d_harmonic_free(ec3d_ctx *c)
{
    Harmonic &H = c->harm;
    ec3d_harmonic_null_free(c); // (the setting stays with the handle)
    batch_free(c);
    H.re.reset();
    H.m.reset();
    H.tab.reset();
    H.vec_own.reset();
    for (auto &v : H.vec) v = nullptr;
    H.stage.reset();
    H.part.reset();
    H.state.reset();
    H.ready = false;
    H.omega = 0.0;
    H.wgs = 0;
    H.last = ec3d_harmonic_info{};
}

extern "C" int ec3d_harmonic_setup(ec3d_handle c, double omega)
{
    int rc = h_need(c, "ec3d_harmonic_setup", false);
    if (rc) return rc;
    if (!(omega >= 0.0) || !std::isfinite(omega)) {
        ec3d_set_error("ec3d_harmonic_setup: omega must be finite and not negative");
        return 2;
    }
    Harmonic &H = c->harm;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    if (!(H.ready && omega == H.omega)) ec3d_harmonic_null_free(c); // Q belongs to the matrix and to omega
    const size_t nt = (size_t)c->A.ncls * 16, len = (size_t)c->A.n_pad;
    std::vector<double> re(nt), m(nt);
    EC3D_HIP(hipMemcpy(re.data(), H.re, nt * sizeof(double), hipMemcpyDeviceToHost));
    EC3D_HIP(hipMemcpy(m.data(), H.m, nt * sizeof(double), hipMemcpyDeviceToHost));
    const std::vector<double> tab = h_table(re, m, omega);
    if (!H.tab) EC3D_HIP(H.tab.alloc(2 * nt));
    EC3D_HIP(hipMemcpy(H.tab, tab.data(), 2 * nt * sizeof(double), hipMemcpyHostToDevice));
    if (!H.vec_own) { // the first set-up on this matrix: vectors (zero), staging, partials, state
        H.wgs = ec3d_stream_wgs((int64_t)len);
        EC3D_HIP(H.vec_own.alloc((size_t)HV_N * 2 * len));
        EC3D_HIP(hipMemsetAsync(H.vec_own, 0, (size_t)HV_N * 2 * len * sizeof(double), c->stream));
        for (int w = 0; w < HV_N; ++w) H.vec[w] = H.vec_own.get() + (size_t)w * 2 * len;
        EC3D_HIP(H.stage.alloc(2 * len));
        EC3D_HIP(hipMemsetAsync(H.stage, 0, 2 * len * sizeof(double), c->stream));
        EC3D_HIP(H.part.alloc((size_t)HP_NSLOT * H.wgs));
        EC3D_HIP(hipMemsetAsync(H.part, 0, (size_t)HP_NSLOT * H.wgs * sizeof(double), c->stream));
        EC3D_HIP(H.state.alloc(1));
        EC3D_HIP(hipMemsetAsync(H.state, 0, sizeof(HarmonicState), c->stream));
        EC3D_HIP(hipStreamSynchronize(c->stream));
    }
    H.omega = omega;
    H.ready = true;
    H.last = ec3d_harmonic_info{};
    H.last.ready = 1;
    H.last.omega = omega;
    H.last.device_bytes = (int64_t)(((size_t)HV_N * 2 * len + 2 * len + (size_t)HP_NSLOT * H.wgs + 2 * nt) * sizeof(double) +
                                    sizeof(HarmonicState));
    return 0;
}

extern "C" int ec3d_harmonic_upload(ec3d_handle c, int which, const double *re, const double *im)
{
    int rc = h_need(c, "ec3d_harmonic_upload", true);
    if (rc) return rc;
    if ((rc = h_which(which, "ec3d_harmonic_upload"))) return rc;
    if (!re) {
        ec3d_set_error("ec3d_harmonic_upload: re is NULL");
        return 2;
    }
    if ((rc = h_to_device(c, c->harm.stage, hv(c, which == EC3D_VEC_X ? HV_X : HV_B), re, im))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ec3d_harmonic_download(ec3d_handle c, int which, double *re, double *im)
{
    int rc = h_need(c, "ec3d_harmonic_download", true);
    if (rc) return rc;
    if ((rc = h_which(which, "ec3d_harmonic_download"))) return rc;
    if (!re || !im) {
        ec3d_set_error("ec3d_harmonic_download: re or im is NULL");
        return 2;
    }
    return h_to_host(c, c->harm.stage, hv(c, which == EC3D_VEC_X ? HV_X : HV_B), re, im);
}

extern "C" int ec3d_harmonic_spmv(ec3d_handle c, const double *xre, const double *xim, double *yre, double *yim)
{
    int rc = h_need(c, "ec3d_harmonic_spmv", true);
    if (rc) return rc;
    if (!yre || !yim || (xre && !xim)) {
        ec3d_set_error("ec3d_harmonic_spmv: NULL argument");
        return 2;
    }
    const cplx *x = hv(c, HV_X);
    if (xre) {
        if ((rc = h_to_device(c, c->harm.stage, hv(c, HV_P), xre, xim))) return rc;
        x = hv(c, HV_P);
    }
    launch_spmv<0>(c, H_A, x, nullptr, hv(c, HV_AP), nullptr, nullptr);
    EC3D_HIP(hipGetLastError());
    return h_to_host(c, c->harm.stage, hv(c, HV_AP), yre, yim);
}

extern "C" int ec3d_harmonic_solve(ec3d_handle c, double tol, int32_t itmax, int32_t *iter, double *relres)
{
    int rc = h_need(c, "ec3d_harmonic_solve", true);
    if (rc) return rc;
    Harmonic &H = c->harm;
    if (H.null_on && !H.null_built && (rc = null_build(c))) return rc;
    const auto t_start = std::chrono::steady_clock::now();
    launch_begin(c, H_A, hv(c, HV_X), hv(c, HV_B), tol, H.null_on != 0);
    EC3D_HIP(hipGetLastError());
    HarmonicState st;
    const int64_t total = (int64_t)itmax + 1; // src/solvers.f90:25-29: itmax + 1 iterations
    bool stopped = false;
    if ((rc = run_iterations(c, H_A, hv(c, HV_X), itmax, st, &stopped))) return rc;
    h_report(H.last, st, stopped, total);
    H.last.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (iter) *iter = H.last.iter;
    if (relres) *relres = H.last.relres;
    if (H.null_on) return null_note(c, st.bnorm);
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
    launch_begin(c, H_A, hv(c, HV_X), hv(c, HV_B), 0.0, false);
    EC3D_HIP(hipGetLastError());
    HarmonicState st;
    EC3D_HIP(hipMemcpyAsync(&st, c->harm.state, sizeof st, hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    if (bnorm) *bnorm = st.bnorm;
    *rel = st.bnorm > 0.0 ? st.rnorm / st.bnorm : st.rnorm;
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
    const Harmonic &H = c->harm;
    double *x = c->vec[EC3D_VEC_X], *b = c->vec[EC3D_VEC_B];
    hipStream_t s = c->stream;
    k_h_load<<<blocks(c->A.n), 256, 0, s>>>(hv(c, HV_X), hv(c, HV_B), part, x, b, c->A.n);
    if (c->n_cond) {
        k_h_load_eddy<<<blocks(c->n_cond), 256, 0, s>>>(hv(c, HV_X), c->A.cls, reinterpret_cast<const cplx *>(H.tab.get()),
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
    *out = c->harm.last;
    out->ready = c->harm.ready ? 1 : 0;
    out->omega = c->harm.omega;
    out->device_bytes += c->harm.null_bytes; // Q, its partials and coefficients, while they exist
    return 0;
}

extern "C" int ec3d_harmonic_device_vector(ec3d_handle c, int which, double **device_ptr, int64_t *pairs)
{
    int rc = h_need(c, "ec3d_harmonic_device_vector", true);
    if (rc) return rc;
    if (which < 0 || which >= HV_N || !device_ptr || !pairs) {
        ec3d_set_error("ec3d_harmonic_device_vector: unknown vector or NULL argument");
        return 2;
    }
    *device_ptr = c->harm.vec[which];
    *pairs = c->A.n_pad;
    return 0;
}

// ---- left null vectors of K + j omega M -------------------------------------------------------
extern "C" int ec3d_harmonic_set_null_projection(ec3d_handle c, int32_t on, double null_tol)
{
    if (!c) {
        ec3d_set_error("ec3d_harmonic_set_null_projection: null handle");
        return 2;
    }
    if (!on) {
        c->harm.null_on = 0; // Q stays with the matrix and omega: switching on again costs nothing
        return 0;
    }
    int rc = h_need(c, "ec3d_harmonic_set_null_projection", true);
    if (rc) return rc; // (the setting as it was)
    Harmonic &H = c->harm;
    const double tol = null_tol > 0.0 ? null_tol : 1e-10;
    if (tol != H.null_tol && H.null_built) {
        EC3D_HIP(hipStreamSynchronize(c->stream));
        ec3d_harmonic_null_free(c); // another accuracy: the vectors are made again
    }
    H.null_on = 1;
    H.null_tol = tol;
    return 0;
}

extern "C" int ec3d_get_harmonic_null(ec3d_handle c, ec3d_null_info *info)
{
    if (!c || !info) {
        ec3d_set_error("ec3d_get_harmonic_null: null handle or info");
        return 2;
    }
    *info = c->harm.null_last;
    info->on = c->harm.null_on;
    info->null_tol = c->harm.null_tol;
    info->built = c->harm.null_built ? 1 : 0;
    return 0;
}

extern "C" int ec3d_harmonic_left_null_vector(ec3d_handle c, int32_t index, double *re, double *im)
{
    int rc = h_need(c, "ec3d_harmonic_left_null_vector", true);
    if (rc) return rc;
    Harmonic &H = c->harm;
    if (!H.null_built) {
        if (!H.null_on) {
            ec3d_set_error("ec3d_harmonic_left_null_vector: no vectors yet and the projection is off "
                           "(ec3d_harmonic_set_null_projection)");
            return 2;
        }
        if ((rc = null_build(c))) return rc;
    }
    if (index < 0 || index >= H.null_kept || !re || !im) {
        ec3d_set_error("ec3d_harmonic_left_null_vector: index " + std::to_string(index) + " is outside the " +
                       std::to_string(H.null_kept) + " vectors kept, or a NULL argument");
        return 2;
    }
    return h_to_host(c, H.stage, reinterpret_cast<const cplx *>(H.nq.get()) + (size_t)index * c->A.n_pad, re, im);
}

extern "C" int ec3d_harmonic_spmv_h(ec3d_handle c, const double *xre, const double *xim, double *yre, double *yim)
{
    int rc = h_need(c, "ec3d_harmonic_spmv_h", true);
    if (rc) return rc;
    if (!yre || !yim || (xre && !xim)) {
        ec3d_set_error("ec3d_harmonic_spmv_h: NULL argument");
        return 2;
    }
    const cplx *x = hv(c, HV_X);
    if (xre) {
        if ((rc = h_to_device(c, c->harm.stage, hv(c, HV_P), xre, xim))) return rc;
        x = hv(c, HV_P);
    }
    launch_spmv<0>(c, H_AH, x, nullptr, hv(c, HV_AP), nullptr, nullptr);
    EC3D_HIP(hipGetLastError());
    return h_to_host(c, c->harm.stage, hv(c, HV_AP), yre, yim);
}

extern "C" int ec3d_harmonic_projected_residual(ec3d_handle c, double *rel, double *removed)
{
    int rc = h_need(c, "ec3d_harmonic_projected_residual", true);
    if (rc) return rc;
    Harmonic &H = c->harm;
    if (!H.null_on || !rel) {
        ec3d_set_error(!rel ? "ec3d_harmonic_projected_residual: rel is NULL"
                            : "ec3d_harmonic_projected_residual: the projection is off (ec3d_harmonic_set_null_projection)");
        return 2;
    }
    if (!H.null_built && (rc = null_build(c))) return rc;
    launch_begin(c, H_A, hv(c, HV_X), hv(c, HV_B), 0.0, true);
    EC3D_HIP(hipGetLastError());
    HarmonicState st;
    EC3D_HIP(hipMemcpyAsync(&st, H.state, sizeof st, hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    *rel = st.bnorm > 0.0 ? st.rnorm / st.bnorm : st.rnorm;
    if ((rc = null_note(c, st.bnorm))) return rc;
    if (removed) *removed = H.null_last.removed;
    return 0;
}

extern "C" int ec3d_harmonic_null_restarts(ec3d_handle c, int32_t *restarts)
{
    if (!c || !restarts) {
        ec3d_set_error("ec3d_harmonic_null_restarts: null handle or array");
        return 2;
    }
    for (int i = 0; i < EC3D_NULL_MAX_REPORT; ++i) restarts[i] = c->harm.null_restarts[i];
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
    Harmonic &H = c->harm;
    if (nsys == 0) {
        EC3D_HIP(hipStreamSynchronize(c->stream));
        batch_free(c);
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
    const size_t nt = (size_t)c->A.ncls * 16;
    std::vector<double> re(nt), m(nt), tabs;
    EC3D_HIP(hipMemcpy(re.data(), H.re, nt * sizeof(double), hipMemcpyDeviceToHost));
    EC3D_HIP(hipMemcpy(m.data(), H.m, nt * sizeof(double), hipMemcpyDeviceToHost));
    tabs.reserve((size_t)nsys * 2 * nt);
    for (int32_t s = 0; s < nsys; ++s) {
        const std::vector<double> t = h_table(re, m, omega[s]);
        tabs.insert(tabs.end(), t.begin(), t.end());
    }
    batch_free(c); // nothing is refused from here on: the batch before goes, whatever its size
    if ((rc = batch_alloc(c, nsys, tabs))) {
        batch_free(c);
        return rc;
    }
    H.bn = nsys;
    for (int32_t s = 0; s < nsys; ++s) {
        H.bomega[s] = omega[s];
        H.blast[s].ready = 1;
        H.blast[s].omega = omega[s];
        H.blast[s].device_bytes = H.bbytes;
    }
    return 0;
}

extern "C" int ec3d_harmonic_batch_upload(ec3d_handle c, int32_t sys, int which, const double *re, const double *im)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_upload", sys, false);
    if (rc) return rc;
    if ((rc = h_which(which, "ec3d_harmonic_batch_upload"))) return rc;
    if (!re) {
        ec3d_set_error("ec3d_harmonic_batch_upload: re is NULL");
        return 2;
    }
    if ((rc = h_to_device(c, c->harm.bstage, hbv(c, sys, which == EC3D_VEC_X ? HV_X : HV_B), re, im))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ec3d_harmonic_batch_download(ec3d_handle c, int32_t sys, int which, double *re, double *im)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_download", sys, false);
    if (rc) return rc;
    if ((rc = h_which(which, "ec3d_harmonic_batch_download"))) return rc;
    if (!re || !im) {
        ec3d_set_error("ec3d_harmonic_batch_download: re or im is NULL");
        return 2;
    }
    return h_to_host(c, c->harm.bstage, hbv(c, sys, which == EC3D_VEC_X ? HV_X : HV_B), re, im);
}

extern "C" int ec3d_harmonic_batch_solve(ec3d_handle c, double tol, int32_t itmax, int32_t *iter)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_solve", 0, true);
    if (rc) return rc;
    Harmonic &H = c->harm;
    if (H.null_on) {
        ec3d_set_error("ec3d_harmonic_batch_solve: ec3d_harmonic_set_null_projection is on, and its vectors belong to one omega; "
                       "switch it off, or solve the systems one by one (ec3d_harmonic_batch_select)");
        return 2;
    }
    if (H.bnull_on && !H.bnull_built && (rc = batch_null_build(c))) return rc;
    const auto t_start = std::chrono::steady_clock::now();
    batch_launch_begin(c, tol, H.bnull_on != 0);
    EC3D_HIP(hipGetLastError());
    std::vector<HarmonicState> st;
    if ((rc = batch_run_iterations(c, itmax, st))) return rc;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    for (int s = 0; s < H.bn; ++s) {
        const HarmonicState &q = st[(size_t)s];
        h_report(H.blast[s], q, q.stop_s != INT_MAX || q.stop_r != INT_MAX, (int64_t)itmax + 1);
        H.blast[s].ms = ms;
        if (iter) iter[s] = H.blast[s].iter;
    }
    if (H.bnull_on) return batch_null_note(c, st);
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
    *out = c->harm.blast[sys];
    out->device_bytes += c->harm.bnull_bytes; // the left null vectors of the batch, while they exist
    return 0;
}

extern "C" int ec3d_harmonic_batch_select(ec3d_handle c, int32_t sys)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_select", sys, false);
    if (rc) return rc;
    if ((rc = ec3d_harmonic_setup(c, c->harm.bomega[sys]))) return rc;
    const size_t bytes = (size_t)c->A.n_pad * sizeof(cplx);
    EC3D_HIP(hipMemcpyAsync(hv(c, HV_X), hbv(c, sys, HV_X), bytes, hipMemcpyDeviceToDevice, c->stream));
    EC3D_HIP(hipMemcpyAsync(hv(c, HV_B), hbv(c, sys, HV_B), bytes, hipMemcpyDeviceToDevice, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ec3d_harmonic_batch_device_vector(ec3d_handle c, int32_t sys, int which, double **device_ptr, int64_t *pairs)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_device_vector", sys, false);
    if (rc) return rc;
    if (which < 0 || which >= HV_N || !device_ptr || !pairs) {
        ec3d_set_error("ec3d_harmonic_batch_device_vector: unknown vector or NULL argument");
        return 2;
    }
    *device_ptr = reinterpret_cast<double *>(hbv(c, sys, which));
    *pairs = c->A.n_pad;
    return 0;
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
        c->harm.bnull_on = 0;
        return 0;
    }
    int rc = hb_need(c, "ec3d_harmonic_batch_set_null_projection", 0, true);
    if (rc) return rc; // (the setting as it was)
    Harmonic &H = c->harm;
    const double tol = null_tol > 0.0 ? null_tol : 1e-10;
    if (tol != H.bnull_tol && H.bnull_built) {
        EC3D_HIP(hipStreamSynchronize(c->stream));
        batch_null_free(c); // another accuracy: the vectors are made again
    }
    H.bnull_on = 1;
    H.bnull_tol = tol;
    return 0;
}

extern "C" int ec3d_get_harmonic_batch_null(ec3d_handle c, int32_t sys, ec3d_null_info *info, int32_t *shares_with)
{
    int rc = hb_need(c, "ec3d_get_harmonic_batch_null", sys, false);
    if (rc) return rc;
    if (!info) {
        ec3d_set_error("ec3d_get_harmonic_batch_null: info is NULL");
        return 2;
    }
    const Harmonic &H = c->harm;
    *info = H.bnull_built ? H.bnull_last[H.bnset_of[sys]] : ec3d_null_info{};
    info->on = H.bnull_on;
    info->null_tol = H.bnull_tol;
    info->built = H.bnull_built ? 1 : 0;
    info->removed = H.bnremoved[sys];
    if (shares_with) *shares_with = batch_shares_with(H, sys);
    return 0;
}

extern "C" int ec3d_harmonic_batch_left_null_vector(ec3d_handle c, int32_t sys, int32_t index, double *re, double *im)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_left_null_vector", sys, false);
    if (rc) return rc;
    Harmonic &H = c->harm;
    if (!H.bnull_built) {
        if (!H.bnull_on) {
            ec3d_set_error("ec3d_harmonic_batch_left_null_vector: no vectors yet and the projection is off "
                           "(ec3d_harmonic_batch_set_null_projection)");
            return 2;
        }
        if ((rc = batch_null_build(c))) return rc;
    }
    const int d = H.bnset_of[sys], kept = H.bnkept[d];
    if (index < 0 || index >= kept || !re || !im) {
        ec3d_set_error("ec3d_harmonic_batch_left_null_vector: index " + std::to_string(index) + " is outside the " +
                       std::to_string(kept) + " vectors kept for system " + std::to_string(sys) + ", or a NULL argument");
        return 2;
    }
    return h_to_host(c, H.bstage, reinterpret_cast<const cplx *>(H.bnq.get()) + ((size_t)d * H.bncomp + (size_t)index) * c->A.n_pad,
                     re, im);
}

extern "C" int ec3d_harmonic_batch_null_restarts(ec3d_handle c, int32_t sys, int32_t *restarts)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_null_restarts", sys, false);
    if (rc) return rc;
    if (!restarts) {
        ec3d_set_error("ec3d_harmonic_batch_null_restarts: restarts is NULL");
        return 2;
    }
    const Harmonic &H = c->harm;
    for (int i = 0; i < EC3D_NULL_MAX_REPORT; ++i) restarts[i] = H.bnull_built ? H.bnull_restarts[H.bnset_of[sys]][i] : 0;
    return 0;
}

extern "C" int ec3d_harmonic_batch_projected_residual(ec3d_handle c, double *rel, double *removed)
{
    int rc = hb_need(c, "ec3d_harmonic_batch_projected_residual", 0, true);
    if (rc) return rc;
    Harmonic &H = c->harm;
    if (!H.bnull_on || !rel) {
        ec3d_set_error(!rel ? "ec3d_harmonic_batch_projected_residual: rel is NULL"
                            : "ec3d_harmonic_batch_projected_residual: the projection is off "
                              "(ec3d_harmonic_batch_set_null_projection)");
        return 2;
    }
    if (!H.bnull_built && (rc = batch_null_build(c))) return rc;
    batch_launch_begin(c, 0.0, true);
    EC3D_HIP(hipGetLastError());
    std::vector<HarmonicState> st((size_t)H.bn);
    EC3D_HIP(hipMemcpyAsync(st.data(), H.bstate, st.size() * sizeof(HarmonicState), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    if ((rc = batch_null_note(c, st))) return rc;
    for (int s = 0; s < H.bn; ++s) {
        const HarmonicState &q = st[(size_t)s];
        rel[s] = q.bnorm > 0.0 ? q.rnorm / q.bnorm : q.rnorm;
        if (removed) removed[s] = H.bnremoved[s];
    }
    return 0;
}
