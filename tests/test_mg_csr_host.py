"""CPU-only: the multigrid preconditioner over a 7-point matrix that came as CSR with its box (ec3d_set_precond_grid).

* the C++ hierarchy rule (ec3d_mg_plan_matrix of csrc/ec3d_mg_plan.hpp, run through the stand-alone program
  tests/support/mg_plan_matrix_cases.cpp, built with the address and undefined-behaviour sanitizers) == the twin's
  (mg_numpy_csr.plan) on a list of boxes: ceil-halved dims, every coarse level Galerkin;
* the generated operators (tests/csr_grid_generate.py) are what they say: symmetric / M-matrix, diagonally dominant,
  CSR == bands;
* on 33x31x29 with oracle.poisson_csr the twin is mg_numpy_agg's bit for bit, in both precisions (that box is Galerkin
  from level 1 under the aggregate rule);
* the twin's solves (mg_numpy.pbicgstab_gpuorder, tol 1e-8, itmax 60, b = standard_normal of PCG64(5), x0 = 0) converge
  on every case and shape, in fp64 and fp32, in exactly the outer iterations ITERS records -- the counts this twin gave
  when the test was written, not chosen in advance -- and in fewer than the same operator takes without a
  preconditioner (mg_numpy.Identity; its iteration is cut at 300, so 301 stands for "at least 301")."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import csr_grid_generate as G
import mg_numpy as M
import mg_numpy_agg as A
import mg_numpy_csr as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "mg_plan_matrix_cases.cpp")
TOL, ITMAX, ID_ITMAX = 1e-8, 60, 300

BOXES = [(45, 43, 41), (34, 18, 70), (70, 66, 2), (33, 31, 29), (2, 2, 2), (16, 16, 16), (17, 16, 16), (64, 64, 64),
         (48, 40, 36), (100, 100, 100), (250, 250, 250), (256, 256, 256), (500, 500, 500), (2, 2, 4097), (8193, 2, 2),
         (6, 1024, 6), (101, 99, 97), (130, 126, 2)]
SHAPES = [(45, 43, 41), (34, 18, 70), (70, 66, 2), (33, 31, 29)]
# (case, shape) -> (fp64, fp32) outer iterations of the twin, and of mg_numpy.Identity on the same operator
ITERS = {
    ("poisson", (45, 43, 41)): ((10, 10), 301), ("jump", (45, 43, 41)): ((17, 17), 301),
    ("convect", (45, 43, 41)): ((15, 15), 67),
    ("poisson", (34, 18, 70)): ((8, 8), 256), ("jump", (34, 18, 70)): ((13, 14), 301),
    ("convect", (34, 18, 70)): ((13, 13), 50),
    ("poisson", (70, 66, 2)): ((4, 4), 91), ("jump", (70, 66, 2)): ((7, 7), 301),
    ("convect", (70, 66, 2)): ((9, 9), 55),
    ("poisson", (33, 31, 29)): ((12, 12), 281), ("jump", (33, 31, 29)): ((16, 16), 301),
    ("convect", (33, 31, 29)): ((13, 13), 57),
}


def _id(d):
    return "x".join(map(str, d))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{box: (dims, kinds)} as the C++ program prints them."""
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("mg_plan_matrix") / "mg_plan_matrix_cases")
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe] + [_id(b) for b in BOXES], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    found = {}
    for line in out.stdout.splitlines():
        key, *v = line.split()
        assert key == "plan"
        v = [int(a) for a in v]
        assert len(v) == 4 + 4 * v[3]
        levels = [tuple(v[4 + 4 * l:8 + 4 * l]) for l in range(v[3])]
        found[tuple(v[:3])] = ([l[:3] for l in levels], [l[3] for l in levels])
    assert len(found) == len(BOXES)
    return found


@pytest.mark.parametrize("box", BOXES, ids=[_id(b) for b in BOXES])
def test_cxx_plan_equals_the_twins(plans, box):
    dims, kinds = plans[box]
    tdims, tkinds = K.plan(*box)
    assert dims == tdims and kinds == tkinds
    assert kinds == [K.MATRIX] + [K.GALERKIN] * (len(dims) - 1)
    assert dims[-1][0] * dims[-1][1] * dims[-1][2] <= M.MAX_COARSE_ROWS
    assert dims == A.hierarchy(*box)[0]              # the aggregate rule's dims, whatever its kinds


def test_documented_hierarchies(plans):
    assert plans[45, 43, 41][0] == [(45, 43, 41), (23, 22, 21), (12, 11, 11)]
    assert plans[34, 18, 70][0] == [(34, 18, 70), (17, 9, 35), (9, 5, 18)]
    assert plans[70, 66, 2][0] == [(70, 66, 2), (35, 33, 1)]
    assert plans[33, 31, 29][0] == [(33, 31, 29), (17, 16, 15)]
    assert plans[2, 2, 2] == ([(2, 2, 2)], [K.MATRIX])
    assert plans[256, 256, 256][1] == [0, 2, 2, 2, 2]    # Galerkin even where the aggregate rule would rediscretise
    assert A.hierarchy(256, 256, 256)[1] == [0, 1, 1, 1, 1]


@pytest.mark.parametrize("dims", SHAPES, ids=[_id(d) for d in SHAPES])
@pytest.mark.parametrize("name", G.CASES)
def test_generated_operators(oracle, name, dims):
    valA, irow, jcol, c = G.case(name, dims)
    n = int(np.prod(dims))
    offs = G.offsets(dims)
    rows = np.repeat(np.arange(n), np.diff(irow))
    off = (jcol - 1) - rows
    assert irow[0] == 1 and len(irow) == n + 1 and np.isin(off, offs).all()
    assert all((np.diff(jcol[irow[r] - 1:irow[r + 1] - 1]) > 0).all() for r in range(0, n, 97))   # ascending columns
    back = np.zeros((7, n))
    back[np.searchsorted(offs, off), rows] = valA
    assert np.array_equal(back, c)                    # CSR == bands; nothing of c lies beyond the box
    i, j = np.arange(n) % dims[0], (np.arange(n) // dims[0]) % dims[1]
    for q, m in ((2, i == 0), (4, i == dims[0] - 1), (1, j == 0), (5, j == dims[1] - 1)):
        assert (c[q][m] == 0.0).all()                 # the wrap slots
    if name == "poisson":
        return
    offd = np.delete(c, 3, 0)
    assert (offd <= 0.0).all() and (c[3] > 0.0).all()
    slack = c[3] - np.abs(offd).sum(0)
    assert (slack >= -1e-9 * c[3]).all() and (slack > 1e-3 * c[3]).any()      # diagonally dominant, strictly somewhere
    sym = all(np.array_equal(c[6 - q][max(0, -offs[6 - q]):n - max(0, offs[6 - q])],
                             c[q][max(0, -offs[q]):n - max(0, offs[q])]) for q in (4, 5, 6))
    assert sym == (name == "jump")
    if name == "jump":
        assert c[3].max() / c[3].min() > 500.0        # the jump is there


@pytest.mark.parametrize("cls, agg", [(K.CsrMG, A.AggMG), (K.CsrMG32, A.AggMG32)], ids=["fp64", "fp32"])
def test_same_hierarchy_as_the_aggregate_rule(oracle, cls, agg):
    dims = (33, 31, 29)
    r = np.random.Generator(np.random.PCG64(3)).standard_normal(int(np.prod(dims)))
    ours, ref = cls(dims, G.case("poisson", dims)[3]), agg(*dims)
    assert ours.dims == ref.dims and ours.kinds == ref.kinds == [0, 2]
    for a, b in zip(ours.levels, ref.levels):
        assert np.array_equal(a.c, b.c)
    assert np.array_equal(ours.apply(r), ref.apply(r))


@pytest.mark.parametrize("dims", SHAPES, ids=[_id(d) for d in SHAPES])
@pytest.mark.parametrize("name", G.CASES)
def test_twin_solves_converge(oracle, name, dims):
    c = G.case(name, dims)[3]
    n = int(np.prod(dims))
    b = np.random.Generator(np.random.PCG64(5)).standard_normal(n)
    its = []
    for cls in (K.CsrMG, K.CsrMG32):
        mg = cls(dims, c)
        x, it, _, _, _, kind = M.pbicgstab_gpuorder(mg, b, np.zeros(n), TOL, ITMAX)
        rel = np.linalg.norm(b - mg.levels[0].spmv(x)) / np.linalg.norm(b)
        its.append(it)
        assert kind in (M.EXIT_S, M.EXIT_R) and it <= ITMAX and rel < TOL, (name, dims, it, rel)
    _, plain, _, _, _, _ = M.pbicgstab_gpuorder(M.Identity(mg.levels[0]), b, np.zeros(n), TOL, ID_ITMAX)
    print(f"{name} {dims}: levels {mg.dims}, outer iterations fp64 / fp32 {its[0]} / {its[1]}, unpreconditioned "
          f"{plain if plain <= ID_ITMAX else f'> {ID_ITMAX}'}")
    assert (tuple(its), plain) == ITERS[name, dims]
    assert max(its) < plain
