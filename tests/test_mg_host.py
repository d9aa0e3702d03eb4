"""Multigrid preconditioner, host side (no GPU): the numpy restatement of the V-cycle (tests/mg_numpy.py) converges
in a grid-independent number of outer iterations, the hierarchy rule gives the documented level dims, and the built
library exports the C ABI of the feature (include/ec3d_hip.h, ec3d_set_preconditioner)."""
import ctypes
import os

import numpy as np
import pytest

import mg_numpy as M


@pytest.mark.parametrize("N", [32, 64])
def test_restatement_converges_in_few_outer_iterations(oracle, N):
    mg = M.MG(N, N, N)
    b = oracle.bar_rhs(N)
    x, it = M.pbicgstab(mg, b, tol=1e-8)
    rel = np.linalg.norm(b - mg.spmv(x)) / np.linalg.norm(b)
    print(f"{N}^3: {it} outer iterations, levels {[l.dims for l in mg.levels]}, true residual {rel:.2e}")
    assert it <= 12
    assert rel < 1e-8


@pytest.mark.parametrize("dims, levels, ok", [
    ((64, 64, 64), [(64, 64, 64), (32, 32, 32), (16, 16, 16)], True),
    ((96, 80, 72), [(96, 80, 72), (48, 40, 36), (24, 20, 18), (12, 10, 9)], True),
    ((48, 40, 33), [(48, 40, 33), (24, 20, 33), (12, 10, 33)], True),
    ((67, 67, 67), [(67, 67, 67)], False),
])
def test_hierarchy_rule(dims, levels, ok):
    got, deltas, good = M.hierarchy_dims(*dims, delta=(1.0, 2.0, 4.0))
    assert got == levels and good == ok
    for a in range(3):  # twice the spacing exactly on the axes that halve
        for l in range(1, len(got)):
            f = got[l - 1][a] // got[l][a]
            assert deltas[l][a] == deltas[l - 1][a] * f


def test_library_exports_the_preconditioner():
    from eddy_currents_3d_amd import build as B
    from eddy_currents_3d_amd.solver import LIBPATH
    assert os.path.exists(LIBPATH) or B.build()
    lib = ctypes.CDLL(LIBPATH)
    for name in ("ec3d_set_preconditioner", "ec3d_get_preconditioner", "ec3d_precond_apply"):
        assert hasattr(lib, name), name
