"""Block multigrid preconditioner of the structured A-V form, host side (no GPU): the Galerkin coarse operator of the
numpy restatement (tests/avmg_numpy.py) is the 2h rediscretisation on a conductor-free interior, the restatement's
preconditioned BiCGSTAB needs fewer iterations than the reference's on every captured step of the small fixtures, the
U projection uses the U rows' left null vector, and
the public interface declares the new kind (C header, Fortran module, Python, run.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import avmg_numpy as AV
import mg_numpy as M
from conftest import REPO, load_golden


@pytest.mark.parametrize("dims, delta", [((16, 16, 16), (0.00333, 0.00333, 0.00333)),
                                         ((20, 12, 16), (0.004, 0.005, 0.003))])
def test_galerkin_interior_is_the_2h_rediscretisation(oracle, dims, delta):
    fine = AV.BandLevel(dims, M.bands_of(*dims, delta))
    cdims = tuple(a // 2 for a in dims)
    coarse = AV.galerkin(fine, cdims)
    ref = M.bands_of(*cdims, tuple(2 * d for d in delta))
    sdx, sdy, sdz = cdims
    k, j, i = np.meshgrid(np.arange(sdz), np.arange(sdy), np.arange(sdx), indexing="ij")
    interior = ((i > 0) & (i < sdx - 1) & (j > 0) & (j < sdy - 1) & (k > 0) & (k < sdz - 1)).reshape(-1)
    assert interior.sum() > 0
    for q in range(7):
        np.testing.assert_allclose(coarse.c[q][interior], ref[q][interior], rtol=1e-13, atol=0)


def test_level_dims_ceil_halve_to_4096_cells():
    assert AV.level_dims(256, 256, 256) == [(256, 256, 256), (128, 128, 128), (64, 64, 64), (32, 32, 32),
                                            (16, 16, 16)]
    assert AV.level_dims(102, 102, 24) == [(102, 102, 24), (51, 51, 12), (26, 26, 6)]
    assert AV.level_dims(176, 32, 22) == [(176, 32, 22), (88, 16, 11), (44, 8, 6)]
    assert AV.level_dims(37, 29, 23) == [(37, 29, 23), (19, 15, 12)]
    assert AV.level_dims(16, 15, 14) == [(16, 15, 14)]
    assert AV.level_dims(5000, 1, 1) == [(5000, 1, 1), (2500, 1, 1)]


def test_restriction_and_prolongation_on_odd_axes():
    fine = AV.BandLevel((5, 3, 1), np.ones((7, 15)))
    coarse = AV.BandLevel((3, 2, 1), np.ones((7, 6)))
    r = np.arange(15, dtype=np.float64)
    got = AV.restrict(fine, coarse, r).reshape(2, 3)
    R = r.reshape(3, 5)
    want = np.array([[R[0:2, 0:2].mean(), R[0:2, 2:4].mean(), R[0:2, 4].mean()],
                     [R[2, 0:2].mean(), R[2, 2:4].mean(), R[2, 4]]])
    np.testing.assert_allclose(got, want, rtol=1e-15)
    x = AV.prolong(fine, coarse, np.zeros(15), np.arange(6, dtype=np.float64)).reshape(3, 5)
    assert np.array_equal(x, np.array([[0, 0, 1, 1, 2], [0, 0, 1, 1, 2], [3, 3, 4, 4, 5]], np.float64))


SMALL = ["g1_nonconducting_8x7x6", "g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14",
         "g3_moving_coil_18x16x12"]


@pytest.mark.parametrize("name, k", [(n, k) for n in SMALL for k in range(len(load_golden(n)["iters"]))])
def test_preconditioned_twin_needs_fewer_iterations(oracle, name, k):
    g = load_golden(name)
    mg = AV.AVMG.from_golden(g)
    tol, itmax = float(g["tol"]), int(g["itmax"])
    b, x0 = g[f"b{k}"], g[f"xin{k}"]
    _, it_ref, _, _ = oracle.bicgstab_wr(g["valA"], g["irow"], g["jcol"], b, x0, tol, itmax)
    x, it = M.pbicgstab(mg, b, x0=x0, tol=tol, itmax=it_ref)   # (an itmax exit returns it_ref + 1)
    rel = np.linalg.norm(b - mg.spmv(x)) / np.linalg.norm(b)
    print(f"{name} step {k}: {it} preconditioned iterations, reference {it_ref}; true residual {rel:.2e}")
    assert it < it_ref
    assert rel < tol


@pytest.mark.parametrize("name", ["g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12"])
def test_u_weights_are_the_left_null_vector(oracle, name):
    """A constant U on a component is a null vector of the whole operator; w (1/2 per axis with a missing neighbour)
    annihilates g3's U rows' U columns; the projected right-hand side is orthogonal to w on every component."""
    g = load_golden(name)
    mg = AV.AVMG.from_golden(g)
    nA = 3 * mg.nC
    assert len(mg.ucomps) >= 1
    for cells in mg.ucomps:
        e = np.zeros(mg.n)
        on = np.isin(mg.ucell, cells)
        e[nA:][on] = 1.0
        assert np.abs(mg.spmv(e)).max() <= 1e-12 * np.abs(g["valA"]).max()
        w = np.zeros(mg.n)
        w[nA:][on] = mg.uweight[mg.ucell[on]]
        # w^T A restricted to the U columns: the U rows' transpose product
        irow, jcol, val = g["irow"], g["jcol"] - 1, g["valA"]
        rows = np.repeat(np.arange(mg.n), np.diff(irow))
        wt = np.zeros(mg.n)
        np.add.at(wt, jcol, w[rows] * val)
        if name == "g3_moving_coil_18x16x12":   # (around g2's hole the one-sided rows make w an approximation)
            assert np.abs(wt[nA:]).max() <= 1e-12 * np.abs(val).max()
    bu = np.zeros(mg.nC)
    bu[mg.ucell] = np.random.Generator(np.random.PCG64(3)).standard_normal(len(mg.ucell))
    p = mg.project_u(bu)
    for cells in mg.ucomps:
        assert abs(mg.uweight[cells] @ p[cells]) <= 1e-12 * np.abs(bu).sum()


def test_twin_keeps_the_u_block_on_its_unknowns(oracle):
    """M maps the U unknowns' entries through the U sweeps only, the A blocks through their V-cycles only."""
    g = load_golden("g2_conducting_hole_16x15x14")
    mg = AV.AVMG.from_golden(g)
    nC = mg.nC
    r = np.zeros(mg.n)
    r[3 * nC:] = np.random.Generator(np.random.PCG64(5)).standard_normal(mg.n - 3 * nC)
    z = mg.apply(r)
    assert not z[:3 * nC].any() and z[3 * nC:].any()
    r[3 * nC:] = 1.0   # a constant on the conductor lies along the U rows' left null vector: projected away
    assert not mg.apply(r).any()
    r = np.zeros(mg.n)
    r[nC:2 * nC] = 1.0
    z = mg.apply(r)
    assert not z[:nC].any() and not z[2 * nC:].any() and z[nC:2 * nC].any()


def test_the_interface_declares_block_mg():
    from eddy_currents_3d_amd import solver
    assert solver.PRECOND["block-mg"] == 2
    with open(os.path.join(REPO, "include", "ec3d_hip.h")) as f:
        assert re.search(r"EC3D_PRECOND_BLOCK_MG\s*=\s*2\b", f.read())
    with open(os.path.join(REPO, "eddy_currents_3d_amd", "fortran", "ec3d_hip_mod.f90")) as f:
        src = f.read()
    assert re.search(r"parameter\s*::\s*EC3D_PRECOND_BLOCK_MG\s*=\s*2\b", src)
    public = re.search(r"public\s*::(.*?)\n\s*integer", src, re.S)
    assert public and "EC3D_PRECOND_BLOCK_MG" in public.group(1)


def test_run_lists_precond():
    out = subprocess.run([sys.executable, "-m", "eddy_currents_3d_amd.run", "--help"], cwd=REPO, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--precond" in out.stdout and "block-mg" in out.stdout
