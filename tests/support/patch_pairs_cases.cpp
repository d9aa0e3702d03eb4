// Stand-alone host program of tests/test_patch_pairs_host.py: the pairing rule of the 2-D tiles (ec3d_patch_pairs_ok) and
// the map from a paired launch's physical workgroups to the virtual workgroups they host (ec3d_patch_pair_virtual), both
// from csrc/ec3d_sweep_lists.hpp.  One line per layout given on the command line as sdx:sdy:planes:nblk:pps:slab:dist --
//   layout <the seven numbers> | ok tpp npx
// and, where the rule pairs, one line per physical workgroup:  wg <phys> <virtual of half 0> <virtual of half 1>
#include "../../eddy_currents_3d_amd/csrc/ec3d_sweep_lists.hpp"

#include <cstdio>

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        long long sdx, sdy, planes, nblk, pps;
        int slab, dist;
        if (std::sscanf(argv[a], "%lld:%lld:%lld:%lld:%lld:%d:%d", &sdx, &sdy, &planes, &nblk, &pps, &slab, &dist) != 7) return 2;
        const int64_t tpp = sdx * sdy / 512, npx = sdx / 128;
        const bool ok = ec3d_patch_pairs_ok(tpp, npx, planes, pps, nblk, slab != 0, dist != 0);
        std::printf("layout %lld %lld %lld %lld %lld %d %d | %d %lld %lld\n", sdx, sdy, planes, nblk, pps, slab, dist, (int)ok,
                    (long long)tpp, (long long)npx);
        if (!ok) continue;
        // the virtual ids, through a vector sized to the launch: an id out of range is the sanitizer's to report
        std::vector<int> hosted((size_t)nblk, 0);
        for (int phys = 0; phys < (int)(nblk / 2); ++phys) {
            const int v0 = ec3d_patch_pair_virtual((int)tpp, (int)npx, phys, 0), v1 = ec3d_patch_pair_virtual((int)tpp, (int)npx, phys, 1);
            ++hosted.at((size_t)v0);
            ++hosted.at((size_t)v1);
            std::printf("wg %d %d %d\n", phys, v0, v1);
        }
    }
    return 0;
}
