// ec3d_mg_plan.hpp — the hierarchy rule of the multigrid preconditioner of the single-component operator
// (EC3D_PRECOND_MG, ec3d_mg.hip): the dims of every level and how each level's operator is made, worked out on the host
// before anything is allocated (host only: no HIP call, no kernels).  tests/test_mg_agg_host.py checks it against
// tests/mg_numpy_agg.py.
//
// EC3D_COARSEN_REDISCRETIZE (the default): an axis halves while it is even and >= 8; coarsening stops when no axis can
// halve or a level has <= `cap` rows.  Every coarse level is a rediscretisation.  The rule fails (false) when the
// coarsest level is over the cap.
//
// EC3D_COARSEN_AGGREGATE: every axis whose extent is > 1 is ceil-halved (aggregates of 2 cells, the last one 1 cell on
// an odd axis) until a level has <= `cap` rows, which always happens.  Level l + 1 is a rediscretisation while no
// Galerkin level has appeared and every axis of level l is even and >= 8 (the halving is exact, and the assembly's
// preconditions hold); from the first level that fails this, level l + 1 and every coarser one is the Galerkin product
// of piecewise-constant aggregation.  Where the default rule halves every axis at every level the two rules give the
// same hierarchy.
//
// A 7-point matrix supplied as CSR with its box (ec3d_set_precond_grid; ec3d_mg_plan_matrix): there is no BND and no
// spacing to rediscretise with, so the dims are the aggregate rule's ceil-halving and every coarse level is a Galerkin
// product, whatever the parity of the axes.  tests/test_mg_csr_host.py checks it against tests/mg_numpy_csr.py.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

enum { EC3D_MG_LEVEL_MATRIX = 0, EC3D_MG_LEVEL_REDISCRETIZED = 1, EC3D_MG_LEVEL_GALERKIN = 2 };

struct MgPlan {
    std::vector<std::array<int, 3>> dims; // sdx, sdy, sdz of every level, finest first
    std::vector<int> kinds;               // EC3D_MG_LEVEL_*: level 0 is the handle's matrix
};

// aggregate: EC3D_COARSEN_AGGREGATE, else EC3D_COARSEN_REDISCRETIZE.  cap >= 1.
inline bool ec3d_mg_plan(int sdx, int sdy, int sdz, bool aggregate, int64_t cap, MgPlan &p)
{
    p.dims.assign(1, {sdx, sdy, sdz});
    p.kinds.assign(1, EC3D_MG_LEVEL_MATRIX);
    bool galerkin = false;
    for (;;) {
        const std::array<int, 3> d = p.dims.back();
        if ((int64_t)d[0] * d[1] * d[2] <= cap) return true;
        std::array<int, 3> e = d;
        int halves = 0;
        for (int a = 0; a < 3; ++a)
            if (d[a] % 2 == 0 && d[a] >= 8) {
                e[a] = d[a] / 2;
                ++halves;
            }
        if (!aggregate) {
            if (!halves) return false;
        } else if (galerkin || halves < 3) {
            galerkin = true;
            for (int a = 0; a < 3; ++a) e[a] = d[a] > 1 ? (d[a] + 1) / 2 : d[a];
        }
        p.dims.push_back(e);
        p.kinds.push_back(galerkin ? EC3D_MG_LEVEL_GALERKIN : EC3D_MG_LEVEL_REDISCRETIZED);
    }
}

// The hierarchy over a matrix that is all there is (no assembly to rerun): ceil-halving, every coarse level Galerkin.
inline void ec3d_mg_plan_matrix(int sdx, int sdy, int sdz, int64_t cap, MgPlan &p)
{
    p.dims.assign(1, {sdx, sdy, sdz});
    p.kinds.assign(1, EC3D_MG_LEVEL_MATRIX);
    for (;;) {
        std::array<int, 3> e = p.dims.back();
        if ((int64_t)e[0] * e[1] * e[2] <= cap) return;
        for (int a = 0; a < 3; ++a)
            if (e[a] > 1) e[a] = (e[a] + 1) / 2;
        p.dims.push_back(e);
        p.kinds.push_back(EC3D_MG_LEVEL_GALERKIN);
    }
}
