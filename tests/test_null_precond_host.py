"""CPU: N, the block multigrid preconditioner of the null projection's adjoint solves, on its numpy twin
(tests/avmg_adjoint_numpy.py), and the new entry points declared everywhere a host looks for them.

* on g2, g2v, g3, g8a (both components), g8d, g9a and g9b the twin's N inside mg_numpy.pbicgstab solves
  A^T y = -A^T e_m to 1e-10 in no more iterations than null_projection_numpy.left_null_vectors' plain solve of the same
  component, computed beside it, and every resulting normalised w lies within 1e-6 of the span of the plain twin's Q (the
  bound tests/test_gpu_null_projection.py::test_setup uses between device and twin);
* the U part of N r has a plain mean of at most 1e-12 * max |z_U| on every conducting component, for random r, in both
  forms;
* the transposed U block has the constants as LEFT null vector on g3 (why the projections take plain means);
* header, library, solver.EXPORTS, run.build_parser(), host.run and the measuring tool have the feature; the kinds'
  values and the refusal codes are the header's."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mg_numpy as M
import null_projection_numpy as NP
from avmg_adjoint_numpy import AdjointAVMG
from avmg_numpy import bands_from_csr
from conftest import REPO, load_golden

SEVEN = ["g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14", "g3_moving_coil_18x16x12",
         "g8a_two_plates_18x16x16", "g8d_g3_split_18x16x12", "g9a_two_moving_mixed_bnd_20x16x14",
         "g9b_L_hole_near_faces_17x16x16"]
NAMES = ("ec3d_set_null_precond", "ec3d_get_null_precond", "ec3d_null_precond_apply")

_TWINS = {}


def twin_for(name, g, transposed_a=True):
    """AdjointAVMG of fixture `name`, built once per process and form."""
    key = (name, bool(transposed_a))
    if key not in _TWINS:
        _TWINS[key] = AdjointAVMG.from_golden(g, transposed_a=transposed_a)
    return _TWINS[key]


def preconditioned_adjoint_solve(mg, At, n, seed, null_tol=NP.DEFAULT_NULL_TOL, itmax=None):
    """(w normalised, iterations, reached) of A^T y = -A^T e_seed through mg_numpy.pbicgstab with N = mg."""
    cap = NP.adjoint_cap(n) if itmax is None else itmax
    e = np.zeros(n)
    e[seed] = 1.0
    y, it = M.pbicgstab(mg, -At(e), tol=null_tol, itmax=cap)
    w = y + e
    return w / np.linalg.norm(w), it, it <= cap


@pytest.mark.parametrize("name", SEVEN)
def test_preconditioned_twin_reaches_null_tol_in_no_more_iterations(oracle, name):
    g = load_golden(name)
    s = NP.setup_for(oracle, name, g)
    n = len(g["irow"]) - 1
    mg = twin_for(name, g)
    Q = np.array(s["Q"])
    assert len(s["seeds"]) == len(s["info"]) >= 1
    for seed, rec in zip(s["seeds"], s["info"]):
        w, it, reached = preconditioned_adjoint_solve(mg, s["At"], n, seed)
        d = np.linalg.norm(w - Q.T @ (Q @ w))
        print(f"{name} seed {seed}: preconditioned {it} iterations, plain {rec['iterations']}; "
              f"distance of w from span(Q) {d:.3e}")
        assert rec["reached"]
        assert reached
        assert it <= rec["iterations"]
        assert d <= 1e-6


@pytest.mark.parametrize("transposed_a", [True, False], ids=["block-mg", "block-mg-a"])
@pytest.mark.parametrize("name", ["g2_conducting_hole_16x15x14", "g8a_two_plates_18x16x16"])
def test_u_part_has_no_plain_mean(oracle, name, transposed_a):
    g = load_golden(name)
    mg = twin_for(name, g, transposed_a)
    nA = 3 * mg.nC
    rng = np.random.default_rng(7)
    assert len(mg.ucomps) == (2 if name.startswith("g8a") else 1)
    for _ in range(2):
        z = mg.apply(rng.standard_normal(mg.n))
        zu = np.zeros(mg.nC)
        zu[mg.ucell] = z[nA:]
        assert np.abs(z[nA:]).max() > 0.0
        for cells in mg.ucomps:
            assert abs(zu[cells].mean()) <= 1e-12 * np.abs(z[nA:]).max()


def test_constants_are_the_left_null_vector_of_the_transposed_u_block(oracle):
    """U has the constants as right null vector, so U^T has them as left null vector: the sweeps on U^T need a
    right-hand side without a plain mean, and the twin's U bands are those of A^T."""
    g = load_golden("g3_moving_coil_18x16x12")
    mg = twin_for("g3_moving_coil_18x16x12", g)
    U = mg.ulevel
    one = mg.urows.astype(np.float64)
    # 1^T U^T x = (U 1) . x: column sums of U^T = row sums of U
    x = np.random.default_rng(3).standard_normal(mg.nC) * one
    ut_x = U.c[3] * x
    for q, v in zip((0, 1, 2, 4, 5, 6), U.neighbours(x)):
        ut_x = ut_x + U.c[q] * v
    assert abs(one @ ut_x) <= 1e-12 * np.abs(U.c).max() * np.abs(x).sum()
    assert np.all(mg.uweight == 1.0)
    # and the U bands are the transposed ones: band q of a cell is band 6 - q of the neighbour's row of A
    _, cu = bands_from_csr(g["valA"], g["irow"], g["jcol"], mg.dims, mg.ucell)
    offs = (-mg.dims[0] * mg.dims[1], -mg.dims[0], -1, 0, 1, mg.dims[0], mg.dims[0] * mg.dims[1])
    for q, o in enumerate(offs):
        cells = np.flatnonzero(U.c[q])
        assert np.array_equal(U.c[q][cells], cu[6 - q][cells + o])


def test_declared_bound_and_exported():
    from eddy_currents_3d_amd import build, host, run, solver
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ec3d_hip.h")).read(), flags=re.S)
    build.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", solver.LIBPATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in solver.EXPORTS
        assert re.search(r" T " + name + r"\b", nm), name
    for text, value in (("EC3D_NULL_PRECOND_NONE", 0), ("EC3D_NULL_PRECOND_BLOCK_MG", 1), ("EC3D_NULL_PRECOND_BLOCK_MG_A", 2),
                        ("EC3D_NULL_PRECOND_MAX_LEVELS", solver.NULL_PRECOND_MAX_LEVELS)):
        assert re.search(r"#define\s+" + text + r"\s+" + str(value) + r"\b", hdr), text
    assert solver.NULL_PRECOND == {"none": 0, "block-mg": 1, "block-mg-a": 2}
    assert (solver.NULL_E_MATRIX, solver.NULL_E_SETUP, solver.PRECOND_E_MATRIX) == (22, 23, 20)
    for m in ("null_precond", "null_precond_apply"):
        assert hasattr(solver.EC3DSolver, m), m
    sig = inspect.signature(solver.EC3DSolver.set_null_projection)
    assert sig.parameters["precond"].default is None
    ap = run.build_parser()
    assert ap.parse_args(["m.vxc"]).null_precond is None
    a = ap.parse_args(["m.vxc", "--null-projection", "--null-precond", "block-mg"])
    assert a.null_projection is True and a.null_precond == "block-mg"
    assert ap.parse_args(["m.vxc", "--null-projection", "--null-precond", "block-mg-a"]).null_precond == "block-mg-a"
    assert inspect.signature(host.run).parameters["null_precond"].default is None
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tight_tolerance_time_loop.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--null-precond" in out.stdout and "block-mg-a" in out.stdout


def test_struct_of_the_projection_keeps_its_layout():
    """ec3d_null_info is untouched: what the new setting reports goes through ec3d_get_null_precond."""
    import ctypes as C
    from eddy_currents_3d_amd.solver import NullInfo
    assert [f[0] for f in NullInfo._fields_] == ["on", "built", "found", "kept", "dropped", "reported", "null_tol", "removed",
                                                 "setup_ms", "seed_row", "iterations", "was_kept", "residual"]
    assert C.sizeof(NullInfo) == 6 * 4 + 3 * 8 + 32 * (8 + 4 + 4 + 8)
