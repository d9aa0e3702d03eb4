"""Numpy restatement of N, the block multigrid preconditioner of the ADJOINT solve of the null projection
(ec3d_set_null_precond, eddy_currents_3d_amd/csrc/ec3d_mg.hip): N ~ (A^T)^-1, block diagonal over
[Ax | Ay | Az | U].

AdjointAVMG is tests/avmg_numpy.AVMG built from the transposed CSR (null_projection_numpy.csr_transpose), so its A
bands and its U bands are those of A^T, with three differences in the U block:

  weights     the U block of A has the constants as right null vector and the 1/2-weights of section 10 as left null
              vector; U^T has them the other way round.  So the right-hand side of the sweeps on U^T is projected with
              weight 1 -- b - mean_c(b), the plain mean of every conducting component, inv_w = 1 / cells -- through
              k_avmg_upart / k_avmg_umean's fixed order (project_u of AVMG with uweight = 1: 1.0 * b is b);
  sweeps      pre + post sweeps of (red, black) from zero on U^T (k_avmg_usweep_t: the coefficient towards a neighbour
              is the neighbour's row's coefficient towards this cell);
  output      the same plain mean taken out of the swept z (k_avmg_upart / k_avmg_umean over z, then k_avmg_usub):
              without it the iterate leaves range(A^T).

transposed_a=False is EC3D_NULL_PRECOND_BLOCK_MG_A: the A blocks' hierarchy is that of A as it stands (section 10's),
the U part as above.  spmv is A^T, so mg_numpy.pbicgstab runs the preconditioned adjoint iteration with this N
unchanged.  apply() is expected to equal ec3d_null_precond_apply bit for bit.

No test lives here (the name does not start with test_)."""
from __future__ import annotations

import numpy as np

import null_projection_numpy as NP
from avmg_numpy import AVMG, BandLevel, bands_from_csr, galerkin, level_dims


class AdjointAVMG(AVMG):
    def __init__(self, valA, irow, jcol, dims, ucell, pre=0, post=0, coarse_sweeps=0, transposed_a=True):
        valT, irowT, jcolT = NP.csr_transpose(valA, irow, jcol)
        super().__init__(valT, irowT, jcolT, dims, ucell, pre, post, coarse_sweeps)
        self.transposed_a = bool(transposed_a)
        if not self.transposed_a:       # the A blocks of A itself; the U block stays that of A^T
            ca, _ = bands_from_csr(valA, irow, jcol, self.dims, self.ucell)
            self.levels = [BandLevel(self.dims, ca)]
            for d in level_dims(*self.dims)[1:]:
                self.levels.append(galerkin(self.levels[-1], d))
            self.levels[0].spmv = self.spmv
        self.uweight = np.ones(self.nC)

    def apply_u(self, bu_cells):
        """project, sweep, project the output"""
        return self.project_u(super().apply_u(bu_cells))
