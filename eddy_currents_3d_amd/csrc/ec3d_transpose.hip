// ec3d_transpose.hip — y = A^T x on the structured A-V form (ec3d_spmv_t).
//
// A gather, one row per thread: row j sums table[class(i)][slot] * x[i] over the rows i that hold an entry in column j.
// Seen from the column, the entries of the format (MatView) are
//   band b of row i = j - off[b]                                     (all blocks; the slot is b)
//   column j in A block d, cell q:  U row of cell q - (jj - 1) step_d, slot 7 + 3 d + jj, jj = 0..2
//   column j in the U block, cell q: A_d row of cell q - m step_d,     slot 7 + m + 2,     m = -2..2, d = 0..2
// and the coefficient is looked up under the SOURCE row's class byte.  The terms are added in ascending source row --
// bands from the largest offset down, couplings from the largest shift down, the A blocks before the U block -- which is
// ascending row in the reference's numbering too (the device numbering only spreads the rows out).  The sum starts at
// +0.0, every product and every sum is rounded on its own (-ffp-contract=off), and a zero coefficient is neither
// multiplied nor added (tests/null_projection_numpy.py, Ordered.of_csr_t, restates it).
//
// The class array has no ghosts, so a source row is TESTED before anything of it is read: it lies in [0, n), in the
// block the entry belongs to, and its class is one that owns the slot (a row between two planes or an empty U slot has
// the zero class: no entries).  x is read at such rows only; it needs no ghost zones.
//
// The kernel runs a few hundred times per assembly (the adjoint solves of ec3d_null.hip), not once per iteration: no
// z-march, no register blocking.  Per row about 16 class bytes and up to 16 x values, neighbours in the caches.
#include "ec3d_internal.hpp"

namespace {

struct SavT {
    const uint8_t *cls;
    const double *table;
    int ncls, a0, u0, zero;
    int64_t n, nC, off[7], step[3];
};

__global__ __launch_bounds__(EC3D_THREADS) void k_sav_spmv_t(SavT A, const double *__restrict__ x, double *__restrict__ y)
{
    extern __shared__ double tbl[];
    for (int q = threadIdx.x; q < A.ncls * 16; q += EC3D_THREADS) tbl[q] = A.table[q];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * EC3D_THREADS + threadIdx.x;
    if (j >= A.n) return;
    const int blk = (int)(j / A.nC);
    const int64_t q = j - blk * A.nC;
    double s = 0.0;
    // a band entry of row i: any class below the zero class has band coefficients
    auto bands = [&]() {
        for (int b = 6; b >= 0; --b) {
            const int64_t i = j - A.off[b];
            if (i < 0 || i >= A.n) continue;
            const int cc = A.cls[i];
            if (cc >= A.zero) continue;
            const double t = tbl[cc * 16 + b];
            if (t != 0.0) s = s + t * x[i];
        }
    };
    if (blk < 3) {
        bands();
        for (int jj = 2; jj >= 0; --jj) { // the U rows that reach this A_d column
            const int64_t cu = q - (jj - 1) * A.step[blk];
            if (cu < 0 || cu >= A.nC) continue;
            const int64_t i = 3 * A.nC + cu;
            const int cc = A.cls[i];
            if (cc < A.u0 || cc >= A.zero) continue;
            const double t = tbl[cc * 16 + 7 + 3 * blk + jj];
            if (t != 0.0) s = s + t * x[i];
        }
    } else {
        for (int d = 0; d < 3; ++d)
            for (int m = 2; m >= -2; --m) { // the coupled A_d rows that reach this U column
                const int64_t ca = q - m * A.step[d];
                if (ca < 0 || ca >= A.nC) continue;
                const int64_t i = d * A.nC + ca;
                const int cc = A.cls[i];
                if (cc < A.a0 || cc >= A.u0) continue;
                const double t = tbl[cc * 16 + 7 + m + 2];
                if (t != 0.0) s = s + t * x[i];
            }
        bands();
    }
    y[j] = s;
}

} // namespace

void ec3d_launch_spmv_t(const MatView &A, int64_t n, const double *x, double *y, hipStream_t s)
{
    SavT T;
    T.cls = A.cls;
    T.table = A.table;
    T.ncls = A.ncls;
    T.a0 = A.sav_a0;
    T.u0 = A.sav_u0;
    T.zero = A.sav_zero;
    T.n = n;
    T.nC = A.sav_nC;
    for (int b = 0; b < 7; ++b) T.off[b] = A.off[b];
    for (int d = 0; d < 3; ++d) T.step[d] = A.sav_step[d];
    k_sav_spmv_t<<<(unsigned)((n + EC3D_THREADS - 1) / EC3D_THREADS), EC3D_THREADS, (size_t)A.ncls * 16 * sizeof(double), s>>>(T, x, y);
}

extern "C" int ec3d_spmv_t(ec3d_handle c, const double *x, double *y)
{
    int rc = ec3d_need_matrix(c, "ec3d_spmv_t");
    if (rc) return rc;
    if ((rc = ec3d_null_eligible(c, "ec3d_spmv_t", true))) return rc;
    EC3D_HIP(hipSetDevice(c->device));
    // P and AP serve as scratch (as in ec3d_spmv)
    if ((rc = ec3d_vec_h2d(c, c->vec[EC3D_VEC_P], x))) return rc;
    ec3d_launch_spmv_t(c->A.view(), c->A.n, c->vec[EC3D_VEC_P], c->vec[EC3D_VEC_AP], c->stream);
    EC3D_HIP(hipGetLastError());
    if ((rc = ec3d_vec_d2h(c, y, c->vec[EC3D_VEC_AP]))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
