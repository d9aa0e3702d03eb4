// Stand-alone host program of tests/test_avmg_plan_host.py: runs ec3d_avmg_plan on small structured A-V models and
// prints, per case, what it was given and what it planned (doubles as %a, the class bytes as hex digits):
//   case NAME / dims sdx sdy sdz pitch nCd ncls a_hi u_lo u_hi uchunk / cls ... / tab ...
//   then either "refusal TEXT" or the lists ured ublack ucomp plist pw chunks cco inv_w, one per line.
// A model is a set of U cells on the grid.  Its classes: A_GEN, A_TWIN (the same 7 band coefficients, another
// coefficient behind them) and A_ODD (one band coefficient different) for the A rows; one U class per pattern of
// neighbours that are U cells (the coefficient towards any other neighbour is 0); ZERO (no coefficients); STRAY (outside
// both ranges with a band coefficient) and STRAY0 (outside both ranges, a coefficient only behind the bands).
#include "../../eddy_currents_3d_amd/csrc/ec3d_avmg_plan.hpp"

#include <cstdio>
#include <functional>

namespace {

enum { A_GEN = 0, A_TWIN = 1, A_ODD = 2, A_HI = 3 };

struct Model {
    int sdx, sdy, sdz, pitch;
    int64_t nCd;
    std::vector<char> u; // per device row: a U cell
    std::vector<uint8_t> cls;
    std::vector<double> tab;
    int u_hi = A_HI;
    int zero() const { return u_hi; }
    int stray() const { return u_hi + 1; }
    int stray0() const { return u_hi + 2; }

    Model(int sdx_, int sdy_, int sdz_, int pitch_)
        : sdx(sdx_), sdy(sdy_), sdz(sdz_), pitch(pitch_), nCd((int64_t)pitch_ * sdz_), u((size_t)nCd, 0)
    {
    }
    int64_t row(int i, int j, int k) const { return (int64_t)k * pitch + (int64_t)j * sdx + i; }
    void box(int i0, int i1, int j0, int j1, int k0, int k1)
    {
        for (int k = k0; k < k1; ++k)
            for (int j = j0; j < j1; ++j)
                for (int i = i0; i < i1; ++i) u[(size_t)row(i, j, k)] = 1;
    }
    // the class bytes of the four blocks and the class table
    void build()
    {
        std::vector<int> mask((size_t)nCd, -1), cls_of_mask(64, -1), masks;
        for (int k = 0; k < sdz; ++k)
            for (int j = 0; j < sdy; ++j)
                for (int i = 0; i < sdx; ++i) {
                    const int64_t r = row(i, j, k);
                    if (!u[(size_t)r]) continue;
                    const bool nb[6] = {k > 0 && u[(size_t)(r - pitch)],      j > 0 && u[(size_t)(r - sdx)],
                                        i > 0 && u[(size_t)(r - 1)],          i + 1 < sdx && u[(size_t)(r + 1)],
                                        j + 1 < sdy && u[(size_t)(r + sdx)],  k + 1 < sdz && u[(size_t)(r + pitch)]};
                    int m = 0;
                    for (int q = 0; q < 6; ++q) m |= nb[q] << q;
                    if (cls_of_mask[(size_t)m] < 0) {
                        cls_of_mask[(size_t)m] = A_HI + (int)masks.size();
                        masks.push_back(m);
                    }
                    mask[(size_t)r] = m;
                }
        u_hi = A_HI + (int)masks.size();
        const int ncls = u_hi + 3;
        tab.assign((size_t)ncls * 16, 0.0);
        for (int a = 0; a < A_HI; ++a) {
            double *t = &tab[(size_t)a * 16];
            for (int q = 0; q < 7; ++q) t[q] = q == 3 ? 6.5 : -1.0 - 0.125 * q;
        }
        tab[(size_t)A_TWIN * 16 + 9] = 3.0;
        tab[(size_t)A_ODD * 16 + 4] = -1.75;
        for (size_t e = 0; e < masks.size(); ++e) {
            double *t = &tab[(size_t)(A_HI + (int)e) * 16];
            for (int q = 0; q < 6; ++q)
                if (masks[e] >> q & 1) t[q < 3 ? q : q + 1] = -0.5 - 0.25 * q;
            t[3] = 7.0 + (double)e;
        }
        tab[(size_t)stray() * 16 + 2] = -2.0;
        tab[(size_t)stray0() * 16 + 9] = 5.0;
        cls.assign((size_t)(4 * nCd), (uint8_t)zero());
        for (int64_t r = 0; r < nCd; ++r) {
            const bool cell = r % pitch < (int64_t)sdx * sdy;
            cls[(size_t)r] = (uint8_t)(cell ? A_GEN : zero());
            cls[(size_t)(nCd + r)] = (uint8_t)(cell ? A_TWIN : stray0()); // a padding row outside the A range: no band coefficient
            cls[(size_t)(2 * nCd + r)] = (uint8_t)(cell ? A_GEN : zero());
            if (mask[(size_t)r] >= 0) cls[(size_t)(3 * nCd + r)] = (uint8_t)cls_of_mask[(size_t)mask[(size_t)r]];
        }
    }
};

template <class T, class F> void line(const char *name, const std::vector<T> &v, F print)
{
    std::printf("%s", name);
    for (const T &x : v) print(x);
    std::printf("\n");
}

void run(const char *name, Model m, const std::function<void(Model &)> &change = nullptr)
{
    m.build();
    if (change) change(m);
    const auto pi = [](int32_t x) { std::printf(" %d", (int)x); };
    const auto pd = [](double x) { std::printf(" %a", x); };
    std::printf("case %s\ndims %d %d %d %d %lld %d %d %d %d %d\ncls ", name, m.sdx, m.sdy, m.sdz, m.pitch, (long long)m.nCd,
                (int)(m.tab.size() / 16), (int)A_HI, (int)A_HI, m.u_hi, EC3D_AVMG_UCHUNK);
    for (uint8_t b : m.cls) std::printf("%02x", (unsigned)b);
    std::printf("\n");
    line("tab", m.tab, pd);
    AvmgPlan p;
    const std::string refusal = ec3d_avmg_plan(m.sdx, m.sdy, m.sdz, m.pitch, m.nCd, m.cls.data(), m.tab.data(), A_HI, A_HI,
                                               m.u_hi, EC3D_AVMG_UCHUNK, p);
    if (!refusal.empty()) {
        std::printf("refusal %s\n", refusal.c_str());
        return;
    }
    line("ured", p.ured, pi);
    line("ublack", p.ublack, pi);
    line("ucomp", p.ucomp, pi);
    line("plist", p.plist, pi);
    line("pw", p.pw, pd);
    line("chunks", p.chunks, pi);
    line("cco", p.cco, pi);
    line("inv_w", p.inv_w, pd);
}

} // namespace

int main()
{
    {   // 7 x 5 x 4 with five padding rows per plane
        Model m(7, 5, 4, 40);
        m.box(6, 7, 1, 2, 1, 2); // (6, 1, 1) and (0, 2, 1): rows 53 and 54, neighbours in memory only
        m.box(0, 1, 2, 3, 1, 2);
        m.box(2, 5, 3, 5, 0, 2); // 3 x 2 x 2 on the k = 0 face
        m.box(0, 1, 0, 1, 3, 4); // (0, 0, 3) and (1, 1, 3) meet at an edge
        m.box(1, 2, 1, 2, 3, 4);
        run("pitch", m);
    }
    {   // more than one chunk in a component, then a component of one cell
        Model m(19, 18, 18, 19 * 18);
        m.box(1, 18, 1, 17, 1, 17);
        m.box(18, 19, 17, 18, 17, 18);
        run("chunks", m);
    }
    run("no_u", Model(3, 2, 2, 8));
    Model small(4, 3, 2, 12);
    small.box(1, 3, 1, 2, 0, 2);
    run("ay_differs", small, [](Model &m) { m.cls[(size_t)(m.nCd + m.row(2, 1, 1))] = A_ODD; });
    run("u_stray", small, [](Model &m) { m.cls[(size_t)(3 * m.nCd + m.row(3, 2, 0))] = (uint8_t)m.stray(); });
    run("outside_without_coefficients", small, [](Model &m) {
        const int64_t r = m.row(0, 0, 1);
        m.cls[(size_t)r] = (uint8_t)m.zero();
        m.cls[(size_t)(m.nCd + r)] = (uint8_t)m.stray0();
        m.cls[(size_t)(2 * m.nCd + r)] = (uint8_t)m.zero();
        m.cls[(size_t)(3 * m.nCd + m.row(3, 0, 0))] = (uint8_t)m.stray0();
    });
    return 0;
}
