"""The aggregate coarsening rule of the multigrid-preconditioned Poisson solve (ec3d_set_precond_coarsening,
EC3D_COARSEN_AGGREGATE; csrc/ec3d_mg.hip, csrc/ec3d_mg_plan.hpp) against its numpy twin (tests/mg_numpy_agg.py), bit for
bit, in both cycle precisions, and the setting's semantics.

* one application (ec3d_precond_apply) == AggMG / AggMG32.apply: a Galerkin level that is the coarsest (33x31x29:
  ragged in x and z, exact in y), two Galerkin levels (45x43x41: a band-form level is smoothed, restricted from and
  prolonged to), a Galerkin level made from a dictionary-form rediscretised level (42x38x34, 50^3), an axis going
  5 -> 3 (70x66x5), three spacings with six distinct faces, and a band-form level 0 (ec3d_set_format(h, 0));
* where the default rule halves every axis at every level (48x40x36) both rules give the same bits;
* whole solves == mg_numpy.pbicgstab_gpuorder with the aggregate twin (x, iterations, both history columns, restarts,
  exit kind), and reach the true residual;
* the setting belongs to the handle, in_use and the level kinds to the hierarchy."""
import numpy as np
import pytest

import mg_numpy as M
import mg_numpy_agg as A
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL, ITMAX = 1e-8, 60
BND32 = np.array(A.SKEW_BND).reshape(2, 3).T   # BND(axis, 1 | 2) as solver.assemble_poisson takes it
PLAIN = ((0.00333, 0.00333, 0.00333), -0.95)
SKEW = (A.SKEW_DELTA, A.SKEW_BND)


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


@pytest.fixture(scope="module")
def twins():
    """The numpy hierarchies, built once per grid, operator and precision (never modified)."""
    cache = {}

    def get(dims, op=PLAIN, precision="fp64"):
        key = (tuple(dims), op, precision)
        if key not in cache:
            cls = A.AggMG32 if precision == "fp32" else A.AggMG
            cache[key] = cls(*dims, delta=op[0], bnd=op[1])
        return cache[key]
    return get


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _handle(E, dims, op=PLAIN, dictionary=True, precision="fp64", coarsening="aggregate"):
    s = E.EC3DSolver(dictionary=dictionary)
    s.assemble_poisson(*dims, delta=op[0], bnd=op[1] if np.isscalar(op[1]) else BND32)
    s.set_preconditioner("mg", precision=precision, coarsening=coarsening)
    return s


# ---- 1: one application -----------------------------------------------------------------------------------------------
APPLY = [
    ((33, 31, 29), PLAIN, True, [0, 2]),
    ((45, 43, 41), PLAIN, True, [0, 2, 2]),
    ((42, 38, 34), PLAIN, True, [0, 1, 2]),
    ((50, 50, 50), PLAIN, True, [0, 1, 2]),
    ((70, 66, 5), PLAIN, True, [0, 2]),
    ((33, 31, 29), SKEW, True, [0, 2]),
    ((45, 43, 41), SKEW, True, [0, 2, 2]),
    ((33, 31, 29), PLAIN, False, [0, 2]),
]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("dims, op, dictionary, kinds", APPLY,
                         ids=["x".join(map(str, c[0])) + ("-skew" if c[1] is SKEW else "") + ("" if c[2] else "-bands")
                              for c in APPLY])
def test_precond_apply_equals_twin(E, oracle, twins, dims, op, dictionary, kinds, precision):
    mg = twins(dims, op, precision)
    assert mg.kinds == kinds
    r = _rng(13).standard_normal(int(np.prod(dims)))   # far inside the fp32 normal range, and so is M r
    with _handle(E, dims, op, dictionary, precision) as s:
        assert s.preconditioner() == ("mg", mg.dims)
        assert s.precond_coarsening() == ("aggregate", "aggregate", kinds)
        assert s.precond_precision() == (precision, precision)
        z = s.precond_apply(r)
    zt = mg.apply(r)
    assert np.array_equal(z, zt), np.abs(z - zt).max()


# ---- 2: same hierarchy, same bits -------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_same_hierarchy_same_bits(E, oracle, precision):
    dims = (48, 40, 36)
    r = _rng(14).standard_normal(int(np.prod(dims)))
    with _handle(E, dims, precision=precision, coarsening="rediscretize") as s:
        assert s.precond_coarsening() == ("rediscretize", "rediscretize", [0, 1, 1])
        levels, zd = s.preconditioner(), s.precond_apply(r)
    with _handle(E, dims, precision=precision) as s:
        assert s.precond_coarsening() == ("aggregate", "aggregate", [0, 1, 1])
        assert s.preconditioner() == levels
        assert np.array_equal(s.precond_apply(r), zd)


# ---- 3: whole solves --------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("dims", [(33, 31, 29), (42, 38, 34), (45, 43, 41)], ids=["33x31x29", "42x38x34", "45x43x41"])
def test_solve_equals_twin(E, oracle, twins, dims, precision):
    mg = twins(dims, PLAIN, precision)
    n = int(np.prod(dims))
    b, x0, cap = _rng(11).standard_normal(n), np.zeros(n), 64
    with _handle(E, dims, precision=precision) as s:
        xt, itt, hst, hrt, rst, kt = M.pbicgstab_gpuorder(mg, b, x0, TOL, ITMAX, oracle.geoms_of(s)[1], hist_cap=cap)
        x, it, h = s.solve(b, x0, TOL, ITMAX, hist_cap=cap)
        s.upload("B", b)
        s.upload("X", x)
        rs, kind, true = s.restart_count(), s.read_state()[1], s.true_residual()[0]
    print(f"{dims} {precision}: it {it} (twin {itt}), restarts {rs} ({rst}), exit {kind} ({kt}), true residual {true:.3e}")
    assert it == itt and kind == kt and rs == rst
    assert np.array_equal(h[:, 0], hst, equal_nan=True) and np.array_equal(h[:, 1], hrt, equal_nan=True)
    assert np.array_equal(x, xt), np.abs(x - xt).max()
    assert kind in (M.EXIT_S, M.EXIT_R) and it <= ITMAX and true < TOL


# ---- 4: the setting ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_setting_semantics(E, oracle, twins):
    import ctypes as C
    from eddy_currents_3d_amd.solver import PRECOND_E_COARSE, EC3DError
    d1, d2 = (33, 31, 29), (70, 66, 5)
    n1 = int(np.prod(d1))
    r1, r2 = _rng(18).standard_normal(n1), _rng(19).standard_normal(int(np.prod(d2)))
    with E.EC3DSolver() as fresh:
        fresh.assemble_poisson(*d1)
        xf, itf, hf = fresh.solve(r1, np.zeros(n1), TOL, 2000, hist_cap=400)
    with E.EC3DSolver() as s:
        assert s.precond_coarsening() == ("rediscretize", "rediscretize", [])   # the default, no hierarchy
        s.assemble_poisson(*d1)
        with pytest.raises(EC3DError) as e:                                      # today's refusal
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_COARSE
        assert s.preconditioner() == ("none", []) and s.precond_coarsening() == ("rediscretize", "rediscretize", [])
        x, it, h = s.solve(r1, np.zeros(n1), TOL, 2000, hist_cap=400)           # ... and the handle stays usable
        assert it == itf and np.array_equal(x, xf) and np.array_equal(h, hf, equal_nan=True)
        s.set_precond_coarsening("aggregate")
        assert s.precond_coarsening() == ("aggregate", "rediscretize", [])      # in_use follows the hierarchy: none yet
        s.set_preconditioner("mg")                                               # the same call succeeds
        assert s.preconditioner() == ("mg", twins(d1).dims)
        assert s.precond_coarsening() == ("aggregate", "aggregate", [0, 2])
        assert np.array_equal(s.precond_apply(r1), twins(d1).apply(r1))
        for bad in (2, -1, 7):                                                   # an unknown rule changes nothing
            assert s.L.ec3d_set_precond_coarsening(s.h, C.c_int32(bad)) == 2
            assert s.precond_coarsening() == ("aggregate", "aggregate", [0, 2])
        with pytest.raises(ValueError):
            s.set_precond_coarsening("galerkin")
        s.set_precond_coarsening("rediscretize")                                 # does not rebuild the hierarchy that is set
        assert s.precond_coarsening() == ("rediscretize", "aggregate", [0, 2])
        assert np.array_equal(s.precond_apply(r1), twins(d1).apply(r1))
        s.set_precond_coarsening("aggregate")
        s.assemble_poisson(*d2)                                                  # a new matrix: the hierarchy goes, the setting stays
        assert s.preconditioner() == ("none", []) and s.precond_coarsening() == ("aggregate", "rediscretize", [])
        s.set_preconditioner("mg")
        assert s.preconditioner() == ("mg", twins(d2).dims)
        assert np.array_equal(s.precond_apply(r2), twins(d2).apply(r2))
        s.set_preconditioner("none")
        assert s.precond_coarsening() == ("aggregate", "rediscretize", [])
        s.set_preconditioner("mg")
        assert s.precond_coarsening() == ("aggregate", "aggregate", [0, 2])
        with pytest.raises(EC3DError) as e:                                      # coarsening= is restored after a refusal
            s.set_preconditioner("mg", coarsening="rediscretize")
        assert e.value.status == PRECOND_E_COARSE
        assert s.precond_coarsening() == ("aggregate", "aggregate", [0, 2])
        assert np.array_equal(s.precond_apply(r2), twins(d2).apply(r2))


@pytest.mark.timeout(120)
def test_av_handle_and_block_mg(E, oracle):
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX, EC3DError
    import avmg_numpy as AV
    g = load_golden("g2_conducting_hole_16x15x14")
    with E.EC3DSolver() as s:
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        with pytest.raises(EC3DError) as e:                                      # an A-V matrix is refused as before
            s.set_preconditioner("mg", coarsening="aggregate")
        assert e.value.status == PRECOND_E_MATRIX
        assert s.preconditioner() == ("none", []) and s.precond_coarsening() == ("rediscretize", "rediscretize", [])
        r = _rng(21).standard_normal(s.n)
        zs = []
        for rule in ("rediscretize", "aggregate"):                               # block-mg ignores the setting
            s.set_preconditioner("block-mg", coarsening=rule)
            levels = s.preconditioner()[1]
            assert s.precond_coarsening() == (rule, "aggregate", [0] + [2] * (len(levels) - 1))
            zs.append(s.precond_apply(r))
        assert np.array_equal(zs[0], zs[1])
        sdz, sdy, sdx = g["geoPHYS"].shape
        assert np.array_equal(zs[0], AV.AVMG.from_solver(s, (sdx, sdy, sdz)).apply(r))
