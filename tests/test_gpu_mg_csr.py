"""The multigrid preconditioner over a 7-point matrix that came as CSR with its box (ec3d_set_matrix_csr +
ec3d_set_precond_grid; csrc/ec3d_mg.hip) against its numpy twin (tests/mg_numpy_csr.py), bit for bit, in both cycle
precisions.

* one application (ec3d_precond_apply) == CsrMG / CsrMG32.apply for the generated operators (tests/csr_grid_generate.py:
  constant coefficients, a coefficient with a jump of 10^3, diffusion + upwind convection) on three-level boxes with
  ragged axes (45x43x41, 34x18x70), a two-plane box (70x66x2) and a two-level one (33x31x29); dictionary on (level 0 a
  view of the handle's matrix where it has at most 32 classes, a gathered copy otherwise) and ec3d_set_format(h, 0); a
  5-band matrix (the +-z bands of the two-plane box dropped) through the gather;
* whole solves == mg_numpy.pbicgstab_gpuorder with the twin (x, iterations, both history columns, restarts, exit kind)
  and reach the true residual;
* the CSR route on 33x31x29 == ec3d_assemble_poisson + coarsening="aggregate": same application, same solve;
* refusals leave the handle as it was; the grid belongs to the matrix.  (The library has no public call that frees the
  matrix alone: the grid is cleared in the one internal routine every new matrix and assembly goes through, and the
  test covers those two routes.)"""
import ctypes as C

import numpy as np
import pytest

import csr_generate as W
import csr_grid_generate as G
import mg_numpy as M
import mg_numpy_csr as K

pytestmark = pytest.mark.gpu
TOL, ITMAX = 1e-8, 60
SHAPES = [(45, 43, 41), (34, 18, 70), (70, 66, 2), (33, 31, 29)]
MG_MAXCLS = 32      # EC3D_MG_MAXCLS: classes the smoothers' table holds


def _id(d):
    return "x".join(map(str, d))


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


@pytest.fixture(scope="module")
def twins():
    """The numpy hierarchies, built once per operator, box and precision (never modified)."""
    cache = {}

    def get(name, dims, precision="fp64"):
        key = (name, tuple(dims), precision)
        if key not in cache:
            c = five_band(dims)[3] if name == "jump5" else G.case(name, dims)[3]
            cache[key] = (K.CsrMG32 if precision == "fp32" else K.CsrMG)(dims, c)
        return cache[key]
    return get


def five_band(dims):
    return G.drop_bands(G.case("jump", dims)[3], dims, (0, 6))


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _handle(E, csr, dims, dictionary=True, precision="fp64"):
    s = E.EC3DSolver(dictionary=dictionary)
    s.set_matrix_csr(*csr[:3])
    s.set_preconditioner("mg", precision=precision, grid=dims)
    return s


# ---- 1: one application -----------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("dictionary", [True, False], ids=["dict", "bands"])
@pytest.mark.parametrize("dims", SHAPES, ids=[_id(d) for d in SHAPES])
@pytest.mark.parametrize("name", G.CASES)
def test_precond_apply_equals_twin(E, oracle, twins, name, dims, dictionary, precision):
    mg = twins(name, dims, precision)
    r = _rng(13).standard_normal(int(np.prod(dims)))   # far inside the fp32 normal range, and so is M r
    with _handle(E, G.case(name, dims), dims, dictionary, precision) as s:
        info = s.info
        assert info.nbands == 7 and info.tail_rows == 0
        if not dictionary:
            assert info.dict_classes == 0
        elif name == "jump":                           # more classes than the smoothers' table: the gathered copy
            assert info.dict_classes == 0 or info.dict_classes > MG_MAXCLS
        else:                                          # level 0 is the handle's own dictionary form
            assert 0 < info.dict_classes <= MG_MAXCLS
        assert s.precond_grid() == dims
        assert s.preconditioner() == ("mg", mg.dims)
        assert s.precond_coarsening() == ("rediscretize", "aggregate", mg.kinds)
        assert s.precond_precision() == (precision, precision)
        z = s.precond_apply(r)
    zt = mg.apply(r)
    assert np.array_equal(z, zt), np.abs(z - zt).max()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("dictionary", [True, False], ids=["dict", "bands"])
def test_five_band_matrix(E, oracle, twins, dictionary, precision):
    dims = (70, 66, 2)
    mg = twins("jump5", dims, precision)
    r = _rng(15).standard_normal(int(np.prod(dims)))
    with _handle(E, five_band(dims), dims, dictionary, precision) as s:
        info = s.info
        assert info.nbands == 5 and info.tail_rows == 0 and info.dict_classes == 0
        assert s.preconditioner() == ("mg", mg.dims)
        z = s.precond_apply(r)
    assert np.array_equal(z, mg.apply(r))


# ---- 2: whole solves --------------------------------------------------------------------------------------------------
def _solve(s, b, cap):
    x, it, h = s.solve(b, np.zeros(len(b)), TOL, ITMAX, hist_cap=cap)
    s.upload("B", b)
    s.upload("X", x)
    return x, it, h, s.restart_count(), s.read_state()[1], s.true_residual()[0]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("dims", SHAPES[:2], ids=[_id(d) for d in SHAPES[:2]])
@pytest.mark.parametrize("name", ["jump", "convect"])
def test_solve_equals_twin(E, oracle, twins, name, dims, precision):
    mg = twins(name, dims, precision)
    n = int(np.prod(dims))
    b, cap = _rng(11).standard_normal(n), 64
    with _handle(E, G.case(name, dims), dims, precision=precision) as s:
        xt, itt, hst, hrt, rst, kt = M.pbicgstab_gpuorder(mg, b, np.zeros(n), TOL, ITMAX, oracle.geoms_of(s)[1], hist_cap=cap)
        x, it, h, rs, kind, true = _solve(s, b, cap)
    print(f"{name} {dims} {precision}: it {it} (twin {itt}), restarts {rs} ({rst}), exit {kind} ({kt}), true residual {true:.3e}")
    assert it == itt and kind == kt and rs == rst
    assert np.array_equal(h[:, 0], hst, equal_nan=True) and np.array_equal(h[:, 1], hrt, equal_nan=True)
    assert np.array_equal(x, xt), np.abs(x - xt).max()
    assert kind in (M.EXIT_S, M.EXIT_R) and it <= ITMAX and true < TOL


# ---- 3: the CSR route == the assembled route --------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_csr_route_equals_assembled_route(E, oracle, precision):
    dims = (33, 31, 29)
    n = int(np.prod(dims))
    r, b = _rng(14).standard_normal(n), _rng(16).standard_normal(n)
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_preconditioner("mg", precision=precision, coarsening="aggregate")
        assert s.precond_coarsening()[1:] == ("aggregate", [0, 2])
        levels, za, sa = s.preconditioner(), s.precond_apply(r), _solve(s, b, 64)
    with _handle(E, G.case("poisson", dims), dims, precision=precision) as s:
        assert s.preconditioner() == levels and s.precond_coarsening()[1:] == ("aggregate", [0, 2])
        zc, sc = s.precond_apply(r), _solve(s, b, 64)
    assert np.array_equal(zc, za)
    assert sc[1] == sa[1] and sc[3:5] == sa[3:5] and np.array_equal(sc[0], sa[0])
    assert np.array_equal(sc[2], sa[2], equal_nan=True)
    assert sc[5] < TOL and sa[5] < TOL


# ---- 4: refusals ------------------------------------------------------------------------------------------------------
GOOD = (45, 43, 41)


def _refused_matrices():
    valA, irow, jcol, _ = G.case("jump", GOOD)
    n = int(np.prod(GOOD))
    mid = n // 2 + 77
    w = W.case("wrap128_dict")
    return {
        "wrap_slot": (w[:3], (128, 16, 12)),
        "tail_entry": (G.with_entry(valA, irow, jcol, mid, 5, 0.625), GOOD),
        "zero_diagonal": (G.set_entry(valA, irow, jcol, mid, mid, 0.0), GOOD),
        "offset_not_the_boxs": ((valA, irow, jcol), (43, 45, 41)),
    }


@pytest.mark.timeout(120)
@pytest.mark.parametrize("what", ["wrap_slot", "tail_entry", "zero_diagonal", "offset_not_the_boxs"])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_matrix_refusals(E, oracle, what, precision):
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX, EC3DError
    csr, grid = _refused_matrices()[what]
    n = len(csr[1]) - 1
    b = _rng(17).standard_normal(n)
    with E.EC3DSolver() as fresh:
        fresh.set_matrix_csr(*csr)
        xf, itf, hf = fresh.solve(b, np.zeros(n), TOL, 25, hist_cap=30)
    with E.EC3DSolver() as s:
        s.set_matrix_csr(*csr)
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg", precision=precision, coarsening="aggregate", grid=grid)
        print(e.value)
        assert e.value.status == PRECOND_E_MATRIX and "row " in str(e.value)
        assert s.preconditioner() == ("none", [])
        assert s.precond_grid() is None                                  # grid=, precision= and coarsening= are undone
        assert s.precond_precision() == ("fp64", "fp64") and s.precond_coarsening() == ("rediscretize", "rediscretize", [])
        s.set_precond_grid(*grid)                                        # the C call by itself: the grid stays, nothing is built
        assert s.L.ec3d_set_preconditioner(s.h, 1, 0, 0, 0) == PRECOND_E_MATRIX
        assert s.precond_grid() == grid and s.preconditioner() == ("none", [])
        x, it, h = s.solve(b, np.zeros(n), TOL, 25, hist_cap=30)
    assert it == itf and np.array_equal(x, xf, equal_nan=True) and np.array_equal(h, hf, equal_nan=True)


@pytest.mark.timeout(120)
def test_grid_refusals_and_block_mg(E, oracle, twins):
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX, EC3DError
    n = int(np.prod(GOOD))
    csr = G.case("convect", GOOD)
    r, b = _rng(18).standard_normal(n), _rng(19).standard_normal(n)
    with E.EC3DSolver() as fresh:
        fresh.set_matrix_csr(*csr[:3])
        xf, itf, hf = fresh.solve(b, np.zeros(n), TOL, 200, hist_cap=210)
    with E.EC3DSolver() as s:
        assert s.precond_grid() is None
        assert s.L.ec3d_set_precond_grid(s.h, *GOOD) == 2                # no matrix at all
        s.assemble_poisson(*GOOD)
        assert s.L.ec3d_set_precond_grid(s.h, *GOOD) == 2                # an assembled handle
        assert s.precond_grid() is None
        s.set_matrix_csr(*csr[:3])
        for bad in ((45, 43, 40), (45 * 43 * 41, 1, 1), (45 * 43, 41, 1), (1, 45 * 43, 41), (-45, -43, 41), (0, 0, 41)):
            assert s.L.ec3d_set_precond_grid(s.h, *bad) == 2, bad         # sdx sdy sdz != n, an extent < 2
            assert s.precond_grid() is None
        with pytest.raises(EC3DError) as e:                              # without a grid: today's refusal
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_MATRIX
        s.set_preconditioner("mg", grid=GOOD)
        z = s.precond_apply(r)
        assert np.array_equal(z, twins("convect", GOOD).apply(r))
        for bad in ((45, 43, 40), (45 * 43 * 41, 1, 1)):                  # a refused grid changes nothing
            with pytest.raises(EC3DError) as e:
                s.set_precond_grid(*bad)
            assert e.value.status == 2 and s.precond_grid() == GOOD
        with pytest.raises(EC3DError) as e:                              # block-mg is for the structured A-V form
            s.set_preconditioner("block-mg", grid=GOOD)
        assert e.value.status == PRECOND_E_MATRIX
        assert s.preconditioner() == ("mg", twins("convect", GOOD).dims) and s.precond_grid() == GOOD
        assert np.array_equal(s.precond_apply(r), z)
        s.set_preconditioner("none")
        x, it, h = s.solve(b, np.zeros(n), TOL, 200, hist_cap=210)
    assert it == itf and np.array_equal(x, xf) and np.array_equal(h, hf, equal_nan=True)


# ---- 5: lifetime ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_grid_belongs_to_the_matrix(E, oracle, twins):
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX, EC3DError
    d1, d2 = (33, 31, 29), (70, 66, 2)
    r1 = _rng(20).standard_normal(int(np.prod(d1)))
    with E.EC3DSolver() as s:
        s.set_precond_coarsening("rediscretize")
        s.set_matrix_csr(*G.case("jump", d1)[:3])
        s.set_preconditioner("mg", grid=d1)
        assert s.precond_coarsening() == ("rediscretize", "aggregate", [0, 2])   # the handle's setting: ignored, unchanged
        assert np.array_equal(s.precond_apply(r1), twins("jump", d1).apply(r1))
        s.set_matrix_csr(*G.case("jump", d1)[:3])                                # a new matrix, even the same one
        assert s.precond_grid() is None and s.preconditioner() == ("none", [])
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_MATRIX
        s.set_precond_grid(*d1)
        s.assemble_poisson(70, 66, 5)                                            # an assembly
        assert s.precond_grid() is None
        s.set_matrix_csr(*G.case("convect", d2)[:3])
        assert s.precond_grid() is None
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg", coarsening="aggregate")
        assert e.value.status == PRECOND_E_MATRIX
        assert s.precond_coarsening() == ("rediscretize", "rediscretize", [])
        s.set_precond_grid(*d2)
        s.set_precond_grid(0, 0, 0)                                              # taken back
        assert s.precond_grid() is None
        s.set_preconditioner("mg", grid=d2)
        assert s.preconditioner() == ("mg", twins("convect", d2).dims)
        assert s.precond_coarsening() == ("rediscretize", "aggregate", [0, 2])
