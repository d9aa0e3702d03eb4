// ec3d_avmg_plan.hpp — what the block multigrid of the structured A-V form (EC3D_PRECOND_BLOCK_MG, ec3d_mg.hip) works out
// on the host from the matrix's class bytes and class table before it allocates (host only: no HIP call, no kernels):
// that the Ax, Ay, Az rows of every cell have the same band coefficients (src/EC3D.f90: valY = valX, valZ = valX), so one
// hierarchy serves the three blocks; the U rows that hold an unknown, by colour; the conducting components (U rows
// joined across a face of the grid) in order of their first row; the U rows' weights in the left null vector of the
// U block; every component's rows cut into chunks, the unit of k_avmg_upart's sums.
// Device row r = k * pitch + j * sdx + i, colour (i + j + k) & 1 (red = 0): a plane may end in padding rows
// (pitch >= sdx * sdy) of a class without coefficients.  tests/test_avmg_plan_host.py checks it against tests/avmg_numpy.py.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#define EC3D_AVMG_UCHUNK 4096 // entries of one component k_avmg_upart sums in one workgroup

struct AvmgPlan {
    std::vector<int32_t> ured, ublack; // U rows that hold an unknown, by colour, ascending
    std::vector<int32_t> ucomp;        // component of every entry of ured, then of ublack
    std::vector<int32_t> plist;        // the U rows ordered by component, ascending within one
    std::vector<double> pw;            // ... and their weights
    std::vector<int32_t> chunks;       // [lo, hi) into plist of every chunk; a chunk lies within one component
    std::vector<int32_t> cco;          // first chunk of every component, and the number of chunks
    std::vector<double> inv_w;         // per component: 1 / sum of its weights, summed in plist's order
};

// cls: the 4 * nCd class bytes (Ax, Ay, Az, U); tab: 16 doubles per class, the 7 band coefficients first.  A rows have
// classes [0, a_hi), U rows [u_lo, u_hi); a row of any other class must have no band coefficients.  Returns the empty
// string and the plan, or the text of the refusal.
inline std::string ec3d_avmg_plan(int sdx, int sdy, int sdz, int pitch, int64_t nCd, const uint8_t *cls, const double *tab,
                                  int a_hi, int u_lo, int u_hi, int uchunk, AvmgPlan &p)
{
    p = AvmgPlan{};
    const auto bands_of = [&](int k, int lo, int hi, double (&b)[7]) { // what the smoothers read for class k
        const bool in = k >= lo && k < hi;
        for (int q = 0; q < 7; ++q) b[q] = in ? tab[(size_t)k * 16 + q] : 0.0;
        if (in) return true;
        for (int q = 0; q < 7; ++q) // a class outside the range is only allowed without band coefficients
            if (tab[(size_t)k * 16 + q] != 0.0) return false;
        return true;
    };
    std::vector<int32_t> comp_of((size_t)nCd, -1); // -1: no unknown; -2: one, not labelled yet
    for (int64_t r = 0; r < nCd; ++r) {
        double b0[7], b1[7], b2[7], bu[7];
        if (!bands_of(cls[(size_t)r], 0, a_hi, b0) || !bands_of(cls[(size_t)(nCd + r)], 0, a_hi, b1) ||
            !bands_of(cls[(size_t)(2 * nCd + r)], 0, a_hi, b2) || memcmp(b0, b1, sizeof b0) || memcmp(b0, b2, sizeof b0))
            return "ec3d_set_preconditioner: the band coefficients of the Ax, Ay, Az rows of device cell " +
                   std::to_string(r) + " differ: one hierarchy cannot serve the three blocks";
        const int ku = cls[(size_t)(3 * nCd + r)];
        if (!bands_of(ku, u_lo, u_hi, bu))
            return "ec3d_set_preconditioner: a U row outside the U classes has band coefficients";
        if (ku >= u_lo && ku < u_hi) {
            const int64_t ij = r % pitch;
            const int i = (int)(ij % sdx), j = (int)(ij / sdx), k = (int)(r / pitch);
            (((i + j + k) & 1) ? p.ublack : p.ured).push_back((int32_t)r);
            comp_of[(size_t)r] = -2;
        }
    }
    // the components, by flood fill from every row no earlier fill has reached
    std::vector<int32_t> stack;
    int nc = 0;
    for (int64_t r0 = 0; r0 < nCd; ++r0) {
        if (comp_of[(size_t)r0] != -2) continue;
        comp_of[(size_t)r0] = nc;
        stack.assign(1, (int32_t)r0);
        while (!stack.empty()) {
            const int64_t r = stack.back();
            stack.pop_back();
            const int64_t ij = r % pitch;
            const int i = (int)(ij % sdx), j = (int)(ij / sdx), k = (int)(r / pitch);
            const int64_t nb[6] = {k > 0 ? r - pitch : -1, j > 0 ? r - sdx : -1, i > 0 ? r - 1 : -1,
                                   i + 1 < sdx ? r + 1 : -1, j + 1 < sdy ? r + sdx : -1, k + 1 < sdz ? r + pitch : -1};
            for (int64_t q : nb)
                if (q >= 0 && comp_of[(size_t)q] == -2) {
                    comp_of[(size_t)q] = nc;
                    stack.push_back((int32_t)q);
                }
        }
        ++nc;
    }
    std::vector<std::vector<int32_t>> rows((size_t)nc);
    for (int64_t r = 0; r < nCd; ++r)
        if (comp_of[(size_t)r] >= 0) rows[(size_t)comp_of[(size_t)r]].push_back((int32_t)r);
    for (int cc = 0; cc < nc; ++cc) {
        p.cco.push_back((int32_t)(p.chunks.size() / 2));
        const int32_t lo = (int32_t)p.plist.size();
        double wsum = 0.0;
        for (int32_t r : rows[(size_t)cc]) {
            const double *t = &tab[(size_t)cls[(size_t)(3 * nCd + r)] * 16];
            double w = 1.0;
            for (int d = 0; d < 3; ++d)
                if (t[2 - d] == 0.0 || t[4 + d] == 0.0) w *= 0.5;
            p.plist.push_back(r);
            p.pw.push_back(w);
            wsum += w;
        }
        const int32_t hi = (int32_t)p.plist.size();
        for (int32_t e = lo; e < hi; e += uchunk) {
            p.chunks.push_back(e);
            p.chunks.push_back(std::min<int32_t>(hi, e + uchunk));
        }
        p.inv_w.push_back(1.0 / wsum);
    }
    p.cco.push_back((int32_t)(p.chunks.size() / 2));
    for (int32_t r : p.ured) p.ucomp.push_back(comp_of[(size_t)r]);
    for (int32_t r : p.ublack) p.ucomp.push_back(comp_of[(size_t)r]);
    return std::string();
}

// The plan of N, the preconditioner of the null projection's adjoint solves (ec3d_set_null_precond): U^T has the
// constants as LEFT null vector, so the projections take the plain mean of a component -- every weight 1 (1.0 * b is b,
// and the sums keep k_avmg_upart / k_avmg_umean's order), inv_w = 1 / cells.  Lists, chunks and components stay.
inline void ec3d_avmg_plain_means(AvmgPlan &p)
{
    std::fill(p.pw.begin(), p.pw.end(), 1.0);
    for (size_t cc = 0; cc < p.inv_w.size(); ++cc) {
        const int32_t lo = p.chunks[2 * (size_t)p.cco[cc]], hi = p.chunks[2 * (size_t)p.cco[cc + 1] - 1];
        p.inv_w[cc] = 1.0 / (double)(hi - lo);
    }
}
