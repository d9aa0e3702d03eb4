// Stand-alone host program of tests/test_mg_csr_host.py: runs ec3d_mg_plan_matrix (the hierarchy rule of EC3D_PRECOND_MG
// over a 7-point matrix that came as CSR with its box, ec3d_set_precond_grid) on the boxes named on its command line
// (SDXxSDYxSDZ), at the coarse solver's cap of 4096 rows, and prints one line per box:
//   plan SDX SDY SDZ LEVELS  then per level: sdx sdy sdz kind
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
        MgPlan p;
        ec3d_mg_plan_matrix(sdx, sdy, sdz, 4096, p);
        if (p.dims.size() != p.kinds.size()) return 3;
        printf("plan %d %d %d %zu", sdx, sdy, sdz, p.dims.size());
        for (size_t l = 0; l < p.dims.size(); ++l)
            printf("  %d %d %d %d", p.dims[l][0], p.dims[l][1], p.dims[l][2], p.kinds[l]);
        printf("\n");
    }
    return 0;
}
