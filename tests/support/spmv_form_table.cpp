// Stand-alone host program of tests/test_spmv_form_host.py: prints the form ec3d_spmv_form picks and the dynamic LDS
// ec3d_form_lds sizes for every combination of the MatView / Sweep fields the rule reads.  One line per case:
//   the 11 inputs, '|', fmt nt zm tail patch il hs lds
#include "../../eddy_currents_3d_amd/csrc/ec3d_form.hpp"

#include <cstdio>

int main()
{
    const int nbs[2] = {3, 7}, nclss[2] = {0, 28}, tpps[2] = {0, 4}, bnds[2] = {-1, 5}, npxs[2] = {0, 2}, rps[2] = {0, 64},
              ils[2] = {0, 8}, nts[3] = {0, 1, 3}, hss[2] = {0, 3};
    for (int sav = 0; sav < 2; ++sav)
    for (int nb : nbs)
    for (int ncls : nclss)
    for (int has_tail = 0; has_tail < 2; ++has_tail)
    for (int zm_tpp : tpps)
    for (int bnd_last : bnds)
    for (int patch_npx : npxs)
    for (int rp_px : rps)
    for (int il_planes : ils)
    for (int nt : nts)
    for (int halo_store : hss) {
        MatView A{};
        A.sav = sav;
        A.nb = nb;
        A.ncls = ncls;
        A.has_tail = has_tail;
        Sweep sw{};
        sw.zm_tpp = zm_tpp;
        sw.bnd_last = bnd_last;
        sw.patch_npx = patch_npx;
        sw.rp_px = rp_px;
        sw.il_planes = il_planes;
        sw.nt = nt;
        sw.halo_store = halo_store;
        const SpmvForm f = ec3d_spmv_form(A, sw);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d %zu\n", sav, nb, ncls, has_tail, zm_tpp, bnd_last,
                    patch_npx, rp_px, il_planes, nt, halo_store, f.fmt, (int)f.nt, (int)f.zm, (int)f.tail, (int)f.patch,
                    (int)f.il, (int)f.hs, ec3d_form_lds(A, f));
    }
    return 0;
}
