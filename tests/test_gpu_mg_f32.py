"""The fp32 V-cycle of the multigrid-preconditioned Poisson solve (ec3d_set_precond_precision, EC3D_PRECOND_FP32;
csrc/ec3d_mg.hip) against its numpy float32 twin (tests/mg_numpy_f32.py), bit for bit, and its setting's semantics.

* one application (ec3d_precond_apply: r narrowed on the way in, z widened on the way out) == MG32.apply on every
  coarsening pattern, odd extents, a coarsest level that is no multiple of 64 rows, single-level grids, both forms,
  non-default sweeps, and 128^3 (levels beyond the caches);
* the solve == mg_numpy.pbicgstab_gpuorder with the fp32 M: x, iterations, both history columns, restarts, exit kind,
  through ec3d_solve and ec3d_solve_resident, on the ||R||, ||S|| and itmax exits; converged solves reach the true
  residual;
* the fp64 path is bit for bit what a handle that never touched the setting computes;
* the setting belongs to the handle, in_use to the hierarchy; fp32 + block-mg is refused and leaves the handle alone;
* the fp32 iteration count stays within the cap taken from the twins' counts (mg_numpy_f32.TWIN_ITERS, asserted by tests/test_mg_f32_host.py)."""
import numpy as np
import pytest

import mg_numpy as M
import mg_numpy_f32 as M32
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


@pytest.fixture(scope="module")
def twins():
    """The numpy hierarchies, built once per grid and sweep counts (never modified)."""
    cache = {}

    def get(dims, sweeps=(0, 0, 0), f32=True):
        key = (tuple(dims), tuple(sweeps), f32)
        if key not in cache:
            cls = M32.MG32 if f32 else M.MG
            cache[key] = cls(*dims, pre=sweeps[0], post=sweeps[1], coarse_sweeps=sweeps[2])
        return cache[key]
    return get


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _handle(E, dims, dictionary=True, sweeps=(0, 0, 0), precision="fp32"):
    s = E.EC3DSolver(dictionary=dictionary)
    s.assemble_poisson(*dims)
    s.set_preconditioner("mg", *sweeps, precision=precision)
    return s


# ---- 1: one application -----------------------------------------------------------------------------------------------
SHAPES = [
    (40, 24, 16),    # (2, 2, 2)
    (32, 32, 33),    # (2, 2, 1), odd z
    (33, 32, 32),    # (1, 2, 2), odd x
    (32, 33, 32),    # (2, 1, 2), odd y
    (9, 9, 128),     # (1, 1, 2) twice; coarsest 9x9x32 = 2592 rows (not a multiple of 64)
    (256, 8, 8),     # thin: 128x4x4
    (16, 16, 16),    # single level, 4096 rows exactly: the coarse kernel narrows r itself
    (7, 9, 11),      # single level, 693 rows
    (3, 3, 3),       # single level, the assembly's minimum
]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dictionary", [True, False])
@pytest.mark.parametrize("dims", SHAPES, ids=["x".join(map(str, d)) for d in SHAPES])
def test_apply_equals_twin_on_shapes(E, oracle, twins, dims, dictionary):
    mg = twins(dims)
    r = _rng(13).standard_normal(int(np.prod(dims)))
    with _handle(E, dims, dictionary=dictionary) as s:
        assert s.preconditioner() == ("mg", [l.dims for l in mg.levels])
        assert s.precond_precision() == ("fp32", "fp32")
        z = s.precond_apply(r)
    zt = mg.apply(r)
    assert np.array_equal(z, zt), np.abs(z - zt).max()
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64))   # every entry is a float32 value


@pytest.mark.timeout(120)
def test_apply_equals_twin_at_128(E, oracle, twins):
    dims = (128, 128, 128)
    mg = twins(dims)
    r = _rng(14).standard_normal(int(np.prod(dims)))
    with _handle(E, dims) as s:
        assert np.array_equal(s.precond_apply(r), mg.apply(r))


@pytest.mark.timeout(120)
def test_apply_equals_twin_at_other_sweep_counts(E, oracle, twins):
    dims, sweeps = (40, 24, 16), (1, 3, 4)
    mg = twins(dims, sweeps)
    r = _rng(15).standard_normal(int(np.prod(dims)))
    for dictionary in (True, False):
        with _handle(E, dims, dictionary=dictionary, sweeps=sweeps) as s:
            assert np.array_equal(s.precond_apply(r), mg.apply(r))


# ---- 2: the solve -----------------------------------------------------------------------------------------------------
def _device_solves(s, b, x0, tol, itmax, hist_cap):
    """The same solve through ec3d_solve and ec3d_solve_resident: [(x, it, hist, restarts, stop_kind, true residual)]."""
    out = []
    x, it, h = s.solve(b, x0, tol, itmax, hist_cap=hist_cap)
    s.upload("B", b)
    s.upload("X", x)
    out.append((x, it, h, s.restart_count(), s.read_state()[1], s.true_residual()[0]))
    s.upload("B", b)
    s.upload("X", x0)
    it, h = s.solve_resident(tol, itmax, hist_cap=hist_cap)
    rs, kind = s.restart_count(), s.read_state()[1]
    out.append((s.download("X"), it, h, rs, kind, s.true_residual()[0]))
    return out


def _assert_twin(s, mg, b, x0, tol, itmax, hist_cap, oracle, converged=True):
    tw = M.pbicgstab_gpuorder(mg, b, x0, tol, itmax, oracle.geoms_of(s)[1], hist_cap=hist_cap)
    xt, itt, hst, hrt, rst, kt = tw
    for how, (x, it, h, rs, kind, true) in zip(("solve", "solve_resident"),
                                               _device_solves(s, b, x0, tol, itmax, hist_cap)):
        print(f"{how}: it {it} (twin {itt}), restarts {rs} ({rst}), exit {kind} ({kt}), true residual {true:.3e}")
        assert it == itt, how
        assert kind == kt, how
        assert rs == rst, how
        assert np.array_equal(h[:, 0], hst, equal_nan=True), how
        assert np.array_equal(h[:, 1], hrt, equal_nan=True), how
        assert np.array_equal(x, xt), (how, np.abs(x - xt).max())
        if converged:
            assert kind in (M.EXIT_S, M.EXIT_R) and true < tol, (how, true)
    return tw


@pytest.mark.timeout(300)
def test_bar_rhs_64_solve_equals_twin(E, oracle, twins):
    from bench import bar_rhs
    N = 64
    with _handle(E, (N, N, N)) as s:
        _assert_twin(s, twins((N, N, N)), bar_rhs(N), np.zeros(N ** 3), TOL, 100, 32, oracle)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dictionary", [True, False])
def test_random_rhs_warm_start_solve_equals_twin(E, oracle, twins, dictionary):
    dims = (48, 40, 33)   # (2, 2, 1) coarsening, odd z
    n = int(np.prod(dims))
    b = _rng(11).standard_normal(n)
    x0 = 1e-6 * _rng(12).standard_normal(n)   # about the solution's scale
    with _handle(E, dims, dictionary=dictionary) as s:
        _assert_twin(s, twins(dims), b, x0, TOL, 100, 40, oracle)


@pytest.mark.timeout(300)
def test_s_exit_equals_twin(E, oracle, twins):
    """tol 2e-6 lies between ||S|| of the fp32 twin's iteration 6 (9.7e-7 ||b||) and every norm before it (||R|| of
    iteration 5: 4.5e-6 ||b||): the ||S|| exit, x += alpha p^ only."""
    from bench import bar_rhs
    N, tol = 64, 2e-6
    with _handle(E, (N, N, N)) as s:
        tw = _assert_twin(s, twins((N, N, N)), bar_rhs(N), np.zeros(N ** 3), tol, 40, 41, oracle)
    assert tw[5] == M.EXIT_S and np.isnan(tw[3][tw[1] - 1])


@pytest.mark.timeout(300)
def test_itmax_exit_equals_twin(E, oracle, twins):
    """tol 1e-30, itmax 2: three iterations, no exit taken (the vectors stay far inside the float32 normal range)."""
    from bench import bar_rhs
    N = 64
    with _handle(E, (N, N, N)) as s:
        _, it, _, _, _, kind = _assert_twin(s, twins((N, N, N)), bar_rhs(N), np.zeros(N ** 3), 1e-30, 2, 8, oracle,
                                            converged=False)
    assert it == 3 and kind == M.EXIT_NONE


# ---- 3: fp64 is what it was -------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dims", [(64, 64, 64), (48, 40, 33)], ids=["64", "48x40x33"])
def test_fp64_is_unchanged(E, oracle, dims):
    from bench import bar_rhs
    n = int(np.prod(dims))
    b = bar_rhs(64) if dims == (64, 64, 64) else _rng(11).standard_normal(n)
    x0 = np.zeros(n)
    with E.EC3DSolver() as s:              # never touches the setting
        s.assemble_poisson(*dims)
        s.set_preconditioner("mg")
        ref = s.solve(b, x0, TOL, 100, hist_cap=40)
        zref = s.precond_apply(b)
    with _handle(E, dims, precision="fp64") as s:      # FP64 set explicitly
        assert s.precond_precision() == ("fp64", "fp64")
        explicit = s.solve(b, x0, TOL, 100, hist_cap=40)
        zexp = s.precond_apply(b)
    with _handle(E, dims, precision="fp32") as s:      # FP32, a solve, then back to FP64
        x32, _, _ = s.solve(b, x0, TOL, 100, hist_cap=40)
        s.set_preconditioner("mg", precision="fp64")
        assert s.precond_precision() == ("fp64", "fp64")
        back = s.solve(b, x0, TOL, 100, hist_cap=40)
        zback = s.precond_apply(b)
    assert not np.array_equal(x32, ref[0])             # the fp32 solve was another computation
    for name, (x, it, h), z in (("explicit", explicit, zexp), ("back", back, zback)):
        assert it == ref[1], name
        assert np.array_equal(x, ref[0]), name
        assert np.array_equal(h, ref[2], equal_nan=True), name
        assert np.array_equal(z, zref), name


# ---- 4: the setting ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_setting_semantics(E, oracle, twins):
    import ctypes as C
    d1, d2 = (32, 32, 33), (40, 24, 16)
    r2 = _rng(19).standard_normal(int(np.prod(d2)))
    with E.EC3DSolver() as s:
        assert s.precond_precision() == ("fp64", "fp64")            # the default, no hierarchy
        s.set_precond_precision("fp32")
        assert s.precond_precision() == ("fp32", "fp64")            # in_use follows the hierarchy: none yet
        for bad in (2, -1, 7):
            assert s.L.ec3d_set_precond_precision(s.h, C.c_int32(bad)) == 2
            assert s.precond_precision() == ("fp32", "fp64")
        with pytest.raises(ValueError):
            s.set_precond_precision("fp16")
        s.assemble_poisson(*d1)
        s.set_preconditioner("mg")
        assert s.precond_precision() == ("fp32", "fp32")
        s.set_precond_precision("fp64")                             # does not rebuild the hierarchy that is set
        assert s.precond_precision() == ("fp64", "fp32")
        r1 = _rng(18).standard_normal(int(np.prod(d1)))
        assert np.array_equal(s.precond_apply(r1), twins(d1).apply(r1))
        s.set_precond_precision("fp32")
        s.assemble_poisson(*d2)                                     # another size: the hierarchy goes, the setting stays
        assert s.preconditioner() == ("none", []) and s.precond_precision() == ("fp32", "fp64")
        s.set_preconditioner("mg")
        assert s.precond_precision() == ("fp32", "fp32")
        assert np.array_equal(s.precond_apply(r2), twins(d2).apply(r2))
        s.set_preconditioner("none")
        assert s.precond_precision() == ("fp32", "fp64")
        s.set_preconditioner("mg")
        assert s.precond_precision() == ("fp32", "fp32")
        s.set_preconditioner("mg", precision="fp64")
        assert s.precond_precision() == ("fp64", "fp64")
        assert np.array_equal(s.precond_apply(r2), twins(d2, f32=False).apply(r2))


@pytest.mark.timeout(120)
def test_fp32_block_mg_is_refused(E, oracle):
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX, EC3DError
    g = load_golden("g2_conducting_hole_16x15x14")
    tol, itmax = float(g["tol"]), int(g["itmax"])
    b, x0 = g["b0"], g["xin0"]

    def assemble(s):
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))

    with E.EC3DSolver() as fresh:
        assemble(fresh)
        xf, itf, hf = fresh.solve(b, x0, tol, itmax, hist_cap=64)
    with E.EC3DSolver() as s:
        assemble(s)
        with pytest.raises(EC3DError, match="EC3D_PRECOND_MG only") as e:
            s.set_preconditioner("block-mg", precision="fp32")
        assert e.value.status == PRECOND_E_MATRIX and "fp32" in str(e.value)
        assert s.preconditioner() == ("none", []) and s.precond_precision() == ("fp64", "fp64")   # as it was
        s.set_precond_precision("fp32")                             # ... and the same through the C calls alone
        assert s.L.ec3d_set_preconditioner(s.h, 2, 0, 0, 0) == PRECOND_E_MATRIX
        assert s.preconditioner() == ("none", []) and s.precond_precision() == ("fp32", "fp64")
        x, it, h = s.solve(b, x0, tol, itmax, hist_cap=64)
        assert it == itf and np.array_equal(x, xf) and np.array_equal(h, hf, equal_nan=True)
        s.set_preconditioner("block-mg", precision="fp64")          # the fp64 block multigrid is still there
        assert s.preconditioner()[0] == "block-mg" and s.precond_precision() == ("fp64", "fp64")


# ---- 5: iteration count against fp64 ----------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", ["bar64", "random_48x40x33"])
def test_iteration_count_against_fp64(E, oracle, case):
    """Cap: the device's fp64 count of the same input + the twins' own difference (TWIN_ITERS: 7 and 7 outer iterations
    on the 64^3 bar right-hand side, 11 and 11 on the random one at 48x40x33, so 0) + 2."""
    from bench import bar_rhs
    if case == "bar64":
        dims, b = (64, 64, 64), bar_rhs(64)
    else:
        dims = (48, 40, 33)
        b = _rng(11).standard_normal(int(np.prod(dims)))
    t32, t64 = M32.TWIN_ITERS[case]
    assert 3 * (t32 - t64) <= t64
    its = {}
    for precision in ("fp64", "fp32"):
        with _handle(E, dims, precision=precision) as s:
            x, it, _ = s.solve(b, np.zeros(len(b)), TOL, 100)
            s.upload("B", b)
            s.upload("X", x)
            its[precision] = it
            assert s.true_residual()[0] < TOL
    print(f"{case}: fp32 {its['fp32']} outer iterations, fp64 {its['fp64']} (twins {t32}, {t64})")
    assert its["fp32"] <= its["fp64"] + max(t32 - t64, 0) + 2
