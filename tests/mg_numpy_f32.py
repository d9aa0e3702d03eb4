"""Numpy restatement of the fp32 V-cycle (EC3D_PRECOND_FP32; eddy_currents_3d_amd/csrc/ec3d_mg.hip with T = float).

MG32 is mg_numpy.MG with M computed in numpy float32, operation by operation in the order mg_numpy states (and the
kernels run), so ec3d_precond_apply on an fp32 hierarchy is expected to equal MG32.apply() bit for bit:

  coefficients     every level's fp64 band coefficients (its own rediscretisation), narrowed once with round to nearest;
  right-hand side  the fp64 r narrowed once per application (k_mg_init_f32; the coarse solve on a single-level grid);
  the cycle        every vector, product, difference and division in float32 -- float32 * float32 rounds once to
                   float32 and no product is fused into the subtraction that follows (-ffp-contract=off); division is
                   IEEE correctly rounded on both sides; 1 / children is a power of two;
  z                widened to float64, exactly.

MG32.levels stays the fp64 hierarchy: mg_numpy.pbicgstab_gpuorder takes A = levels[0].spmv in fp64 and calls apply(),
so it runs unchanged with the fp32 M plugged in (the outer iteration is fp64 in every operation; p^ and s^ are float32
values widened on load).  Inputs must keep every intermediate in the float32 normal range."""
from __future__ import annotations

import numpy as np

import mg_numpy as M

F32 = np.float32

# case -> (fp32 twin, fp64 twin) outer iterations to 1e-8, measured with
# pbicgstab_gpuorder and asserted by tests/test_mg_f32_host.py; tests/test_gpu_mg_f32.py takes its cap from them
TWIN_ITERS = {
    "bar32": (7, 7),
    "bar64": (7, 7),
    "random_48x40x33": (11, 11),   # standard_normal of PCG64(11), x0 = 0
}
# no case's difference is near a third of the fp64 count (the issue's threshold for a finding)
assert all(3 * abs(a - b) <= b for a, b in TWIN_ITERS.values())


class Level32(M.Level):
    """A level of mg_numpy with float32 coefficients: half_sweep and residual then run in float32 on float32 vectors."""

    def __init__(self, level):
        self.dims = level.dims
        self.sdx, self.sdy, self.sdz = level.dims
        self.n = level.n
        self.c = level.c.astype(F32)      # round to nearest even: k_mg_narrow
        self.ijk = level.ijk
        self.colour = level.colour


def restrict32(fine, coarse, r):
    fx, fy, fz = (fine.sdx // coarse.sdx, fine.sdy // coarse.sdy, fine.sdz // coarse.sdz)
    R = r.reshape(fine.sdz, fine.sdy, fine.sdx)
    s = np.zeros((coarse.sdz, coarse.sdy, coarse.sdx), F32)
    for dk in range(fz):
        for dj in range(fy):
            for di in range(fx):
                s = s + R[dk::fz, dj::fy, di::fx]
    return (s * (F32(1) / F32(fx * fy * fz))).reshape(-1)


class MG32(M.MG):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.levels32 = [Level32(l) for l in self.levels]

    def _cycle(self, l, b):
        L = self.levels32[l]
        assert b.dtype == F32
        x = np.zeros(L.n, F32)
        if l == len(self.levels32) - 1:
            for _ in range(self.coarse):
                for col in (0, 1, 1, 0):
                    x = L.half_sweep(x, b, col)
            return x
        for _ in range(self.pre):
            x = L.half_sweep(x, b, 0)
            x = L.half_sweep(x, b, 1)
        C = self.levels32[l + 1]
        bc = restrict32(L, C, L.residual(x, b))
        xc = self._cycle(l + 1, bc)
        x = M.prolong(L, C, x, xc)
        for _ in range(self.post):
            x = L.half_sweep(x, b, 1)
            x = L.half_sweep(x, b, 0)
        assert x.dtype == F32 and bc.dtype == F32
        return x

    def apply32(self, r):
        """z = M r as the float32 vector the device stores (p^, s^)."""
        return self._cycle(0, np.asarray(r, np.float64).astype(F32))

    def apply(self, r):
        return self.apply32(r).astype(np.float64)
