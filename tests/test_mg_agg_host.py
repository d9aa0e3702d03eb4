"""CPU-only: the aggregate coarsening rule of the multigrid preconditioner (EC3D_COARSEN_AGGREGATE).

* the C++ hierarchy rule (csrc/ec3d_mg_plan.hpp, run through the stand-alone program tests/support/mg_plan_cases.cpp,
  built with the address and undefined-behaviour sanitizers) == the twin's (mg_numpy_agg.hierarchy) on a list of boxes,
  and under the default rule == mg_numpy.hierarchy_dims, refusals included;
* where the default rule halves every axis at every level the aggregate twin's apply is mg_numpy.MG.apply bit for bit;
* the twin's solves on the grids the feature was proposed with converge: true residual < 1e-8 within itmax = 60.

Outer iterations of the twin (mg_numpy.pbicgstab_gpuorder, tol 1e-8; a block of ones / standard_normal of PCG64(5)),
recorded for the record, not asserted:
  32x32x32 8/8, 48x40x36 6/6, 72x56x40 9/7, 48x40x33 8/8, 33x31x29 11/12, 45x43x41 10/10, 42x38x34 8/8, 50x50x50 9/10,
  70x66x5 7/7, 100x100x100 10/11, 127x127x127 11 and 128x128x128 9 (the block of ones only); with spacings (0.002, 0.003,
  0.005) and faces (-0.95, 0, 1, -1, 0.5, -0.3): 33x31x29 15/15, 42x38x34 20/17, 45x43x41 20/18."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mg_numpy as M
import mg_numpy_agg as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "mg_plan_cases.cpp")
TOL, ITMAX = 1e-8, 60

BOXES = [(100, 100, 100), (250, 250, 250), (500, 500, 500), (255, 255, 255), (48, 40, 33), (70, 66, 5), (130, 126, 2),
         (64, 64, 64), (48, 40, 36), (72, 56, 40), (33, 31, 29), (45, 43, 41), (42, 38, 34), (50, 50, 50),
         (127, 127, 127), (128, 128, 128), (16, 16, 16), (17, 16, 16), (3, 3, 3), (4097, 1, 1), (1, 1, 8193),
         (6, 1024, 6), (101, 99, 97), (512, 512, 512), (8, 8, 66)]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(box, rule): (ok, dims, kinds)} as the C++ program prints them."""
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("mg_plan") / "mg_plan_cases")
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe] + ["x".join(map(str, b)) for b in BOXES], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    found = {}
    for line in out.stdout.splitlines():
        key, *v = line.split()
        assert key == "plan"
        v = [int(a) for a in v]
        levels = [tuple(v[6 + 4 * l:10 + 4 * l]) for l in range(v[5])]
        assert len(v) == 6 + 4 * v[5]
        found[tuple(v[:3]), v[3]] = (bool(v[4]), [l[:3] for l in levels], [l[3] for l in levels])
    assert len(found) == 2 * len(BOXES)
    return found


@pytest.mark.parametrize("box", BOXES, ids=["x".join(map(str, b)) for b in BOXES])
def test_cxx_rule_equals_the_twins(plans, box):
    ok, dims, kinds = plans[box, 1]
    tdims, tkinds = A.hierarchy(*box)
    assert ok and dims == tdims and kinds == tkinds
    assert dims[-1][0] * dims[-1][1] * dims[-1][2] <= M.MAX_COARSE_ROWS
    ok, dims, kinds = plans[box, 0]
    ddims, _, dok = M.hierarchy_dims(*box)
    assert ok == dok and dims == ddims and kinds == [A.MATRIX] + [A.REDISCRETIZED] * (len(dims) - 1)


def test_documented_hierarchies(plans):
    G, R = A.GALERKIN, A.REDISCRETIZED
    expect = {
        (100, 100, 100): ([(50,) * 3, (25,) * 3, (13,) * 3], [R, R, G]),
        (250, 250, 250): ([(125,) * 3, (63,) * 3, (32,) * 3, (16,) * 3], [R, G, G, G]),
        (500, 500, 500): ([(250,) * 3, (125,) * 3, (63,) * 3, (32,) * 3, (16,) * 3], [R, R, G, G, G]),
        (255, 255, 255): ([(128,) * 3, (64,) * 3, (32,) * 3, (16,) * 3], [G, G, G, G]),
        (48, 40, 33): ([(24, 20, 17), (12, 10, 9)], [G, G]),
        (70, 66, 5): ([(35, 33, 3)], [G]),
        (130, 126, 2): ([(65, 63, 1)], [G]),
        (42, 38, 34): ([(21, 19, 17), (11, 10, 9)], [R, G]),
        (48, 40, 36): ([(24, 20, 18), (12, 10, 9)], [R, R]),
        (64, 64, 64): ([(32,) * 3, (16,) * 3], [R, R]),
    }
    for box, (dims, kinds) in expect.items():
        assert plans[box, 1] == (True, [box] + dims, [A.MATRIX] + kinds), box
    for box in ((100,) * 3, (250,) * 3, (500,) * 3, (255,) * 3, (101, 99, 97), (33, 31, 29)):
        assert not plans[box, 0][0], box            # what the default rule refuses
    for box in ((64,) * 3, (48, 40, 36), (72, 56, 40), (128,) * 3, (512,) * 3):
        assert plans[box, 0][:2] == plans[box, 1][:2], box   # the same hierarchy under both rules


@pytest.mark.parametrize("dims", [(48, 40, 36), (64, 64, 64)], ids=["48x40x36", "64"])
def test_same_hierarchy_same_bits(oracle, dims):
    r = np.random.Generator(np.random.PCG64(3)).standard_normal(int(np.prod(dims)))
    ref, agg, agg32 = M.MG(*dims), A.AggMG(*dims), A.AggMG32(*dims)
    assert agg.dims == [l.dims for l in ref.levels] and agg.kinds == [0, 1, 1]
    assert np.array_equal(agg.apply(r), ref.apply(r))
    import mg_numpy_f32 as M32
    assert np.array_equal(agg32.apply(r), M32.MG32(*dims).apply(r))


def _rhs(dims):
    n = int(np.prod(dims))
    ones = np.zeros(dims[::-1])
    ones[tuple(slice(a // 3, a // 3 + max(1, a // 4)) for a in dims[::-1])] = 1.0
    return ones.reshape(-1), np.random.Generator(np.random.PCG64(5)).standard_normal(n)


CASES = [(d, (0.00333,) * 3, -0.95) for d in A.TABLE_GRIDS] + [(d, A.SKEW_DELTA, A.SKEW_BND) for d in A.SKEW_GRIDS]
ONE_RHS = [(127, 127, 127), (128, 128, 128)]   # the block of ones only, as they were proposed (2 M rows in numpy)


@pytest.mark.parametrize("dims, delta, bnd", CASES,
                         ids=["x".join(map(str, c[0])) + ("" if c[2] == -0.95 else "-skew") for c in CASES])
def test_twin_solves_converge(oracle, dims, delta, bnd):
    mg = A.AggMG(*dims, delta=delta, bnd=bnd)
    its = []
    for b in _rhs(dims)[:1 if dims in ONE_RHS else 2]:
        x, it, _, _, _, kind = M.pbicgstab_gpuorder(mg, b, np.zeros(len(b)), TOL, ITMAX)
        rel = np.linalg.norm(b - mg.spmv(x)) / np.linalg.norm(b)
        its.append(it)
        assert kind in (M.EXIT_S, M.EXIT_R) and it <= ITMAX and rel < TOL, (dims, it, rel)
    print(f"{dims}: kinds {mg.kinds}, levels {mg.dims}, outer iterations {' / '.join(map(str, its))}")
