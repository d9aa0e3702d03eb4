"""CPU: the left-null-vector projection of the A-V system on the numpy twin (tests/null_projection_numpy.py), and the
new entry points declared everywhere a host looks for them.

* Ordered.of_csr_t is the transpose: equal to an unordered scatter of the CSR to 1e-13 * sum |terms|, and
  x.(A y) = (A^T x).y;
* on g2, g3, g8a and g9b the twin's w has ||A^T w|| / ||w|| <= BOUND, the adjoint solves end below their cap, the
  vectors kept are orthonormal and their count is 1, 1, 2, 1;
* with the projection the twin reaches tol = 1e-8 within itmax = 2000 on every captured step and the projected true
  residual is at most 2e-8; without it no step gets there (the premise: the floor |w.b| / ||w|| ||b|| lies above);
* components(): two separated plates are two, touching domains (g8c, g8d) one, the L-shaped hole one -- against a
  labelling by repeated minimum over the neighbours;
* ec3d_null_info has the layout solver.NullInfo gives it; header, library, solver.EXPORTS, the Fortran module,
  run.build_parser() and host.run have the feature."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import null_projection_numpy as NP
from conftest import REPO, load_golden

FOUR = ["g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12", "g8a_two_plates_18x16x16",
        "g9b_L_hole_near_faces_17x16x16"]
KEPT = dict(zip(FOUR, (1, 1, 2, 1)))
# ||A^T w|| / ||w|| of the twin's vectors.  The issue's bound is 1e-3 "or, if the twin's own order lands above it, the
# measured maximum x 2".  This twin, null_tol = 1e-10 (python tests/null_projection_numpy.py's left_null_vectors through
# oracle.spmv_csr):  g2 6.01e-04 (103 iterations), g3 5.23e-04 (137), g8a 4.16e-04 (140) and 1.17e-03 (172),
# g9b 1.49e-03 (89).  Maximum 1.494e-03, so:
BOUND = 2.99e-3
NAMES = ("ec3d_spmv_t", "ec3d_set_null_projection", "ec3d_get_null_projection", "ec3d_left_null_vector")


@pytest.mark.parametrize("name", ["g2v_conducting_moving_16x15x14", "g8a_two_plates_18x16x16"])
def test_ordered_transpose_is_the_transpose(oracle, name):
    g = load_golden(name)
    valA, irow, jcol = g["valA"], g["irow"], g["jcol"]
    n = len(irow) - 1
    At, A = NP.Ordered.of_csr_t(valA, irow, jcol), NP.Ordered.of_csr(valA, irow, jcol)
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    row = np.repeat(np.arange(n), np.diff(irow.astype(np.int64)))
    ref = np.zeros(n)
    np.add.at(ref, jcol.astype(np.int64) - 1, valA * x[row])
    got = At(x)
    assert np.all(np.abs(got - ref) <= 1e-13 * At.abs_sum(x))
    assert np.array_equal(A(y), oracle.spmv_csr(valA, irow, jcol, y))     # the forward order is the reference's
    T = NP.csr_transpose(valA, irow, jcol)
    assert np.array_equal(got, oracle.spmv_csr(T[0], T[1], T[2], x))      # ... and the fast transposed product the twin's
    assert abs(x @ A(y) - got @ y) <= 1e-12 * (np.abs(x) @ A.abs_sum(y))


@pytest.mark.parametrize("name", FOUR)
def test_twin_left_null_vectors(oracle, name):
    g = load_golden(name)
    s = NP.setup_for(oracle, name, g)
    n = len(g["irow"]) - 1
    for rec in s["info"]:
        print(name, rec)
        assert rec["reached"] and rec["iterations"] <= NP.adjoint_cap(n)
        assert rec["residual"] <= BOUND
    assert len(s["Q"]) == KEPT[name] == sum(r["kept"] for r in s["info"])
    gram = np.array([[u @ v for v in s["Q"]] for u in s["Q"]])
    assert np.abs(gram - np.eye(len(gram))).max() <= 1e-12
    nA = 3 * g["geoPHYS"].size
    for q in s["Q"]:       # weight on the A rows too: a U-only w cannot be exact
        assert np.abs(q[:nA]).max() > 0.1 * np.abs(q[nA:]).max()


@pytest.mark.parametrize("name", FOUR)
def test_projected_twin_reaches_1e_8_and_the_plain_one_does_not(oracle, name):
    g = load_golden(name)
    s = NP.setup_for(oracle, name, g)
    for k in range(len(g["iters"])):
        b, x0 = g[f"b{k}"], g[f"xin{k}"]
        x, it, removed = NP.bicgstab(s["A"], b, x0, 1e-8, 2000, s["Q"])
        res = np.linalg.norm(NP.project(s["Q"], b - s["A"](x))[0]) / np.linalg.norm(b)
        xp, itp, _ = NP.bicgstab(s["A"], b, x0, 1e-8, 2000)
        resp = np.linalg.norm(b - s["A"](xp)) / np.linalg.norm(b)
        print(f"{name} step {k}: projected {it} iterations, removed {removed:.2e}, projected true residual {res:.2e}; "
              f"plain {itp} iterations, true residual {resp:.2e}")
        assert it <= 2000 and res <= 2e-8
        assert itp == 2001 and resp > 1e-8
        assert removed > 1e-8       # the floor the plain solve cannot get below


def _labels_by_minimum(cond):
    lab = np.where(cond, np.arange(cond.size).reshape(cond.shape), cond.size)
    while True:
        new = lab.copy()
        for ax in range(3):
            for sgn in (1, -1):
                sh = np.full_like(lab, cond.size)
                src, dst = [slice(None)] * 3, [slice(None)] * 3
                src[ax], dst[ax] = (slice(None, -1), slice(1, None)) if sgn > 0 else (slice(1, None), slice(None, -1))
                sh[tuple(dst)] = lab[tuple(src)]
                new = np.minimum(new, sh)
        new = np.where(cond, new, cond.size)
        if np.array_equal(new, lab):
            return lab.reshape(-1)
        lab = new


@pytest.mark.parametrize("name, count", [("g8a_two_plates_18x16x16", 2), ("g8c_side_by_side_20x18x14", 1),
                                         ("g8d_g3_split_18x16x12", 1), ("g9b_L_hole_near_faces_17x16x16", 1)])
def test_components(name, count):
    g = load_golden(name)
    comps = NP.components(g["geoPHYS_C"])
    assert len(comps) == count
    lab = _labels_by_minimum(np.asarray(g["geoPHYS_C"]) > 0)
    firsts = []
    for cells in comps:
        assert np.all(np.diff(cells) > 0)
        assert np.all(lab[cells] == cells[0])                       # one component, named by its first cell
        assert np.count_nonzero(lab == cells[0]) == len(cells)      # ... and all of it
        firsts.append(cells[0])
    assert firsts == sorted(firsts)
    assert sum(len(c) for c in comps) == np.count_nonzero(g["geoPHYS_C"])
    if name in ("g8c_side_by_side_20x18x14", "g8d_g3_split_18x16x12"):   # two conducting domains that touch
        assert len(set(np.asarray(g["geoPHYS"]).reshape(-1)[comps[0]].tolist())) == 2
    seeds = NP.seed_rows(g["geoPHYS_C"])
    nC = g["geoPHYS"].size
    cond = np.flatnonzero(np.asarray(g["geoPHYS_C"]).reshape(-1) > 0)
    assert [cond[m - 3 * nC] for m in seeds] == [c[len(c) // 2] for c in comps]


def test_struct_layout_matches_ctypes(tmp_path):
    from eddy_currents_3d_amd.solver import NullInfo
    fields = [f[0] for f in NullInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ec3d_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ec3d_null_info));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(ec3d_null_info, {f}));\n' for f in fields)
                   + "    return EC3D_NULL_MAX_REPORT == 32 && EC3D_NULL_E_MATRIX == 22 && EC3D_NULL_E_SETUP == 23 ? 0 : 1;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0
    got = [int(v) for v in r.stdout.split()]
    assert got[0] == C.sizeof(NullInfo)
    assert got[1:] == [getattr(NullInfo, f).offset for f in fields]


def test_declared_bound_and_exported():
    from eddy_currents_3d_amd import build, host, run, solver
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ec3d_hip.h")).read(), flags=re.S)
    f90 = open(os.path.join(REPO, "eddy_currents_3d_amd", "fortran", "ec3d_hip_mod.f90")).read()
    build.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", solver.LIBPATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in solver.EXPORTS
        assert re.search(r" T " + name + r"\b", nm), name
        assert f'bind(C, name="{name}")' in f90 and re.search(r"public ::.*?\b" + name + r"\b", f90, flags=re.S), name
    assert re.search(r"#define\s+EC3D_NULL_MIN_KEEP\s+1e-6\b", hdr) and NP.MIN_KEEP == 1e-6
    for m in ("spmv_t", "set_null_projection", "null_projection", "left_null_vector"):
        assert hasattr(solver.EC3DSolver, m), m
    assert (solver.NULL_E_MATRIX, solver.NULL_E_SETUP) == (22, 23)
    ap = run.build_parser()
    a = ap.parse_args(["m.vxc"])
    assert a.null_projection is False and a.tol is None
    a = ap.parse_args(["m.vxc", "--null-projection", "--tol", "1e-8"])
    assert a.null_projection is True and a.tol == 1e-8
    sig = inspect.signature(host.run)
    assert sig.parameters["null_projection"].default is None and sig.parameters["tol"].default is None
