// Stand-alone host program of tests/test_mg_agg_host.py: runs ec3d_mg_plan (the hierarchy rule of EC3D_PRECOND_MG) on the
// boxes named on its command line (SDXxSDYxSDZ) under both coarsening rules, at the coarse solver's cap of 4096 rows,
// and prints one line per box and rule:
//   plan SDX SDY SDZ RULE OK LEVELS  then per level: sdx sdy sdz kind
// RULE: 0 = rediscretize, 1 = aggregate; OK: 0 when the rule refuses the box (the levels reached are still printed).
#include "../../eddy_currents_3d_amd/csrc/ec3d_mg_plan.hpp"

#include <cstdio>

int main(int argc, char **argv)
{
    for (int q = 1; q < argc; ++q) {
        int sdx, sdy, sdz;
        if (sscanf(argv[q], "%dx%dx%d", &sdx, &sdy, &sdz) != 3) {
            fprintf(stderr, "not a box: %s\n", argv[q]);
            return 2;
        }
        for (int rule = 0; rule < 2; ++rule) {
            MgPlan p;
            const bool ok = ec3d_mg_plan(sdx, sdy, sdz, rule == 1, 4096, p);
            if (p.dims.size() != p.kinds.size()) return 3;
            printf("plan %d %d %d %d %d %zu", sdx, sdy, sdz, rule, ok ? 1 : 0, p.dims.size());
            for (size_t l = 0; l < p.dims.size(); ++l)
                printf("  %d %d %d %d", p.dims[l][0], p.dims[l][1], p.dims[l][2], p.kinds[l]);
            printf("\n");
        }
    }
    return 0;
}
