"""Numpy restatement of the multigrid preconditioner over a 7-point matrix that came as CSR with its box
(ec3d_set_matrix_csr + ec3d_set_precond_grid; eddy_currents_3d_amd/csrc/ec3d_mg.hip, ec3d_mg_plan.hpp).

The hierarchy is made from the matrix alone (plan()):

  dims        avmg_numpy.level_dims: every axis whose extent is > 1 is ceil-halved until a level has <= 4096 rows
  kinds       level 0 is the matrix (0), every coarser level the Galerkin product of the level above (2:
              avmg_numpy.galerkin, in k_mg_galerkin's arithmetic and order) -- there is no BND and no spacing to
              rediscretise with

Level 0 is the (7, n) band array of the matrix in offset order (-z, -y, -x, diag, +x, +y, +z), a band the matrix does
not have being zeros.  The cycle is mg_numpy_agg.AggMG's operation by operation (mg_numpy.Level's half_sweep and
residual on the bands, avmg_numpy.restrict / prolong), so on a box whose aggregate hierarchy is Galerkin from level 1
(33x31x29) CsrMG over oracle.poisson_csr's bands is AggMG bit for bit.  CsrMG32 is the fp32 cycle (EC3D_PRECOND_FP32)
after mg_numpy_f32: every level's fp64 coefficients narrowed once, the right-hand side narrowed once, the cycle in
float32; levels stays the fp64 hierarchy (the outer iteration's A).

mg_numpy.pbicgstab and pbicgstab_gpuorder run unchanged with either (levels[0].spmv sums a row in offset order from
the -z term)."""
from __future__ import annotations

import numpy as np

import avmg_numpy as AV
import mg_numpy as M
import mg_numpy_agg as A

MATRIX, GALERKIN = A.MATRIX, A.GALERKIN


def plan(sdx, sdy, sdz):
    """(dims, kinds) of every level, finest first."""
    dims = AV.level_dims(sdx, sdy, sdz)
    return dims, [MATRIX] + [GALERKIN] * (len(dims) - 1)


class CsrMG(A.AggMG):
    def __init__(self, dims, c, pre=0, post=0, coarse_sweeps=0):
        self.dims, self.kinds = plan(*dims)
        c = np.asarray(c, np.float64)
        assert c.shape == (7, int(np.prod(dims))) and (c[3] != 0.0).all()
        self.levels = [A.CoefLevel(dims, c)]
        for d in self.dims[1:]:
            g = AV.galerkin(self.levels[-1], d)
            assert (g.c[3] != 0.0).all()
            self.levels.append(A.CoefLevel(d, g.c))
        self.pre = pre or M.DEFAULT_PRE
        self.post = post or M.DEFAULT_POST
        self.coarse = coarse_sweeps or M.DEFAULT_COARSE


class CsrMG32(CsrMG):
    """levels stays the fp64 hierarchy; levels32 is what the cycle reads (as mg_numpy_agg.AggMG32)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.levels32 = [A.CoefLevel(l.dims, l.c.astype(A.F32)) for l in self.levels]   # k_mg_narrow

    _restrict = staticmethod(A.restrict32)
    dtype = A.F32
    _levels = A.AggMG32._levels
    apply32 = A.AggMG32.apply32
    apply = A.AggMG32.apply
