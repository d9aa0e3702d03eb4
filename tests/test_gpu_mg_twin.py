"""Multigrid-preconditioned solve (ec3d_set_preconditioner, csrc/ec3d_mg.hip) against its GPU-order twin, bit for bit.

* the outer iteration (k_mg_spmv_dot, k_mg_s, k_mg_xr, k_mg_p, k_mg_scalar and the exit gating inside solve_core's
  polling chunks) == tests/mg_numpy.pbicgstab_gpuorder: x, the iteration count, the ||S|| / ||R|| history, the
  restart count and which exit fired, through ec3d_solve and ec3d_solve_resident, on both exits, the itmax exit
  (partway through a polling chunk), itmax = -1, a history shorter than the solve, ||b|| = 0 and a forced restart;
* one V-cycle (ec3d_precond_apply) == mg_numpy.MG bit for bit at non-default sweep counts, with three distinct spacings
  and six distinct BND faces (the coarse levels' reassembly), on every coarsening-factor pattern, odd extents on each
  axis, thin boxes, single-level grids (the coarse kernel straight from r to z, in both formats) and coarse levels
  whose row count is not a multiple of 64;
* above the undivided-launch and vector-placement thresholds (384x384x256) the same, and 512^3 solves to 1e-8;
* re-assembly drops the hierarchy, and setting the preconditioner again replaces it."""
import numpy as np
import pytest

import mg_numpy as M

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _handle(E, dims, dictionary=True, delta=(0.00333, 0.00333, 0.00333), bnd=-0.95, sweeps=(0, 0, 0)):
    s = E.EC3DSolver(dictionary=dictionary)
    s.assemble_poisson(*dims, delta=delta, bnd=bnd)
    s.set_preconditioner("mg", *sweeps)
    return s


def _device_solves(s, b, x0, tol, itmax, hist_cap):
    """The same solve through ec3d_solve and ec3d_solve_resident: [(x, it, hist, restarts, stop_kind)]."""
    out = []
    x, it, h = s.solve(b, x0, tol, itmax, hist_cap=hist_cap)
    out.append((x, it, h, s.restart_count(), s.read_state()[1]))
    s.upload("B", b)
    s.upload("X", x0)
    it, h = s.solve_resident(tol, itmax, hist_cap=hist_cap)
    out.append((s.download("X"), it, h, s.restart_count(), s.read_state()[1]))
    return out


def _assert_twin(s, mg, b, x0, tol, itmax, hist_cap, oracle):
    tw = M.pbicgstab_gpuorder(mg, b, x0, tol, itmax, oracle.geoms_of(s)[1], hist_cap=hist_cap)
    xt, itt, hst, hrt, rst, kt = tw
    for how, (x, it, h, rs, kind) in zip(("solve", "solve_resident"), _device_solves(s, b, x0, tol, itmax, hist_cap)):
        print(f"{how}: it {it} (twin {itt}), restarts {rs} ({rst}), exit {kind} ({kt})")
        assert it == itt, how
        assert kind == kt, how
        assert rs == rst, how
        assert np.array_equal(h[:, 0], hst, equal_nan=True), how
        assert np.array_equal(h[:, 1], hrt, equal_nan=True), how
        assert np.array_equal(x, xt), (how, np.abs(x - xt).max())
    return tw


# ---- A / B1: the outer iteration against the twin -----------------------------------------------------------------
@pytest.mark.timeout(300)
def test_bar_rhs_64_equals_twin(E, oracle):
    from bench import bar_rhs
    N = 64
    mg = M.MG(N, N, N)
    with _handle(E, (N, N, N)) as s:
        _, it, _, _, _, kind = _assert_twin(s, mg, bar_rhs(N), np.zeros(N ** 3), TOL, 100, 32, oracle)
        assert kind in (M.EXIT_S, M.EXIT_R) and it <= 20
        # a history shorter than the solve: the first entries only
        _assert_twin(s, mg, bar_rhs(N), np.zeros(N ** 3), TOL, 100, 3, oracle)


@pytest.mark.timeout(300)
def test_random_rhs_warm_start_band_form_equals_twin(E, oracle):
    dims = (48, 40, 33)   # (2, 2, 1) coarsening, odd z
    n = int(np.prod(dims))
    mg = M.MG(*dims)
    b = _rng(11).standard_normal(n)
    x0 = 1e-6 * _rng(12).standard_normal(n)   # about the solution's scale
    for dictionary in (False, True):
        with _handle(E, dims, dictionary=dictionary) as s:
            _assert_twin(s, mg, b, x0, TOL, 100, 40, oracle)


@pytest.mark.timeout(300)
def test_forced_restart_equals_twin(E, oracle):
    from bench import bar_rhs
    N = 64
    mg = M.MG(N, N, N)
    with _handle(E, (N, N, N)) as s:
        _, _, _, _, restarts, _ = _assert_twin(s, mg, bar_rhs(N) * 1e-6, np.zeros(N ** 3), 1e-2, 100, 64, oracle)
    assert restarts >= 1


@pytest.mark.timeout(300)
def test_s_exit_equals_twin(E, oracle):
    """A tolerance between ||S|| of some iteration and every norm before it: the ||S|| exit (x += alpha p^ only)."""
    from bench import bar_rhs
    N = 64
    mg = M.MG(N, N, N)
    b = bar_rhs(N)
    x0 = np.zeros(N ** 3)
    _, it, hs, hr, _, _ = M.pbicgstab_gpuorder(mg, b, x0, 1e-12, 40, hist_cap=41)
    bn = np.sqrt(M.mg_dot(b, b))
    tol = None
    for k in range(1, it):
        before = min(np.nanmin(hs[:k]), np.nanmin(hr[:k]))
        if hs[k] < before:
            cand = np.sqrt(hs[k] * before) / bn
            if M.pbicgstab_gpuorder(mg, b, x0, cand, 40)[5] == M.EXIT_S:
                tol = cand
                break
    assert tol is not None, "no iteration whose ||S|| alone is below the others"
    with _handle(E, (N, N, N)) as s:
        tw = M.pbicgstab_gpuorder(mg, b, x0, tol, 40, oracle.geoms_of(s)[1], hist_cap=41)
        assert tw[5] == M.EXIT_S and np.isnan(tw[3][tw[1] - 1])
        _assert_twin(s, mg, b, x0, tol, 40, 41, oracle)


@pytest.mark.timeout(400)
@pytest.mark.parametrize("itmax, sweeps, exit_kind", [
    (-1, (0, 0, 0), M.EXIT_NONE),
    (0, (0, 0, 0), M.EXIT_NONE),
    (2, (0, 0, 0), M.EXIT_NONE),
    (20, (1, 1, 1), M.EXIT_NONE),
    (20, (0, 0, 0), M.EXIT_S),   # the default V-cycle takes ||S|| / ||b|| below 1e-30 in the last allowed iteration
])
def test_itmax_exit_equals_twin(E, oracle, itmax, sweeps, exit_kind):
    """tol 1e-30: itmax + 1 iterations (ec3d_mg_chunk gives 4 at 64^3: 21 ends partway through a chunk)."""
    from bench import bar_rhs
    N = 64
    mg = M.MG(N, N, N, pre=sweeps[0], post=sweeps[1], coarse_sweeps=sweeps[2])
    with _handle(E, (N, N, N), sweeps=sweeps) as s:
        _, it, _, _, _, kind = _assert_twin(s, mg, bar_rhs(N), np.zeros(N ** 3), 1e-30, itmax, 24, oracle)
    assert it == itmax + 1 and kind == exit_kind


@pytest.mark.timeout(120)
def test_zero_rhs_returns_x0_unchanged(E, oracle):
    dims = (32, 32, 32)
    n = int(np.prod(dims))
    x0 = _rng(5).standard_normal(n)
    with _handle(E, dims) as s:
        for x, it, h, rs, kind in _device_solves(s, np.zeros(n), x0, TOL, 100, 8):
            assert it == 0 and rs == 0 and kind == M.EXIT_NONE
            assert np.array_equal(x, x0)
            assert np.isnan(h).all()
    xt, itt, _, _, _, kt = M.pbicgstab_gpuorder(M.MG(*dims), np.zeros(n), x0, TOL, 100)
    assert itt == 0 and kt == M.EXIT_NONE and np.array_equal(xt, x0)


# ---- B2: determinism ------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_solve_is_deterministic(E, oracle):
    dims = (48, 40, 33)
    n = int(np.prod(dims))
    b = _rng(21).standard_normal(n)
    runs = []
    with _handle(E, dims) as s:
        runs.append(s.solve(b, np.zeros(n), TOL, 100, hist_cap=40))
        runs.append(s.solve(b, np.zeros(n), TOL, 100, hist_cap=40))
    with _handle(E, dims) as s:
        runs.append(s.solve(b, np.zeros(n), TOL, 100, hist_cap=40))
    for x, it, h in runs[1:]:
        assert it == runs[0][1]
        assert np.array_equal(x, runs[0][0])
        assert np.array_equal(h, runs[0][2], equal_nan=True)


# ---- B3: sweep counts -----------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("sweeps", [(1, 1, 1), (1, 3, 4), (3, 1, 16), (2, 2, 33)])
def test_precond_apply_at_sweep_counts(E, oracle, sweeps):
    dims = (48, 40, 33)
    mg = M.MG(*dims, pre=sweeps[0], post=sweeps[1], coarse_sweeps=sweeps[2])
    r = _rng(7).standard_normal(int(np.prod(dims)))
    with _handle(E, dims, sweeps=sweeps) as s:
        assert np.array_equal(s.precond_apply(r), mg.apply(r))


@pytest.mark.timeout(300)
def test_solve_at_other_sweep_counts_equals_twin(E, oracle):
    from bench import bar_rhs
    N = 64
    sweeps = (1, 3, 4)
    mg = M.MG(N, N, N, pre=sweeps[0], post=sweeps[1], coarse_sweeps=sweeps[2])
    with _handle(E, (N, N, N), sweeps=sweeps) as s:
        _assert_twin(s, mg, bar_rhs(N), np.zeros(N ** 3), TOL, 100, 32, oracle)


# ---- B4: spacing and BND reach the coarse levels --------------------------------------------------------------------
DELTA3 = (0.0021, 0.0033, 0.0047)
BND32 = np.array([[-0.91, -0.62], [-0.83, -0.74], [-0.55, -0.97]])   # BND(axis, 1 | 2) as solver.assemble_poisson takes it
BND6 = BND32.T.reshape(-1)                                            # column-major: what oracle.poisson_csr takes


@pytest.mark.timeout(300)
def test_spacing_and_bnd_on_every_level(E, oracle):
    dims = (48, 40, 33)   # levels 48x40x33, 24x20x33, 12x10x33: z keeps its spacing, x and y double
    mg = M.MG(*dims, delta=DELTA3, bnd=BND6)
    assert mg.levels[1].dims == (24, 20, 33)
    r = _rng(8).standard_normal(int(np.prod(dims)))
    for dictionary in (True, False):
        with _handle(E, dims, dictionary=dictionary, delta=DELTA3, bnd=BND32) as s:
            valA, irow, jcol = s.export_csr()
            va, ir, jc = oracle.poisson_csr(*dims, DELTA3, BND6)
            assert np.array_equal(irow, ir) and np.array_equal(jcol, jc) and np.array_equal(valA, va)
            assert s.preconditioner()[1] == [l.dims for l in mg.levels]
            assert np.array_equal(s.precond_apply(r), mg.apply(r))
            b = _rng(9).standard_normal(int(np.prod(dims)))
            if dictionary:
                _assert_twin(s, mg, b, np.zeros(len(b)), TOL, 12, 16, oracle)


# ---- B5: shapes -----------------------------------------------------------------------------------------------------
SHAPES = [
    (40, 24, 16),    # (2, 2, 2)
    (32, 32, 33),    # (2, 2, 1), odd z
    (33, 32, 32),    # (1, 2, 2), odd x
    (32, 33, 32),    # (2, 1, 2), odd y
    (9, 9, 128),     # (1, 1, 2) twice; coarsest 9x9x32 = 2592 rows (not a multiple of 64)
    (128, 9, 9),     # (2, 1, 1) twice
    (9, 128, 9),     # (1, 2, 1) twice
    (256, 8, 8),     # thin: 128x4x4
    (512, 4, 4),     # thin: 256x4x4 (4096 rows)
    (16, 16, 16),    # single level, 4096 rows exactly
    (7, 9, 11),      # single level, 693 rows
    (3, 3, 3),       # single level, the assembly's minimum
]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dictionary", [True, False])
@pytest.mark.parametrize("dims", SHAPES, ids=["x".join(map(str, d)) for d in SHAPES])
def test_precond_apply_on_shapes(E, oracle, dims, dictionary):
    mg = M.MG(*dims)
    r = _rng(13).standard_normal(int(np.prod(dims)))
    with _handle(E, dims, dictionary=dictionary) as s:
        kind, levels = s.preconditioner()
        assert kind == "mg" and levels == M.hierarchy_dims(*dims)[0] == [l.dims for l in mg.levels]
        assert np.array_equal(s.precond_apply(r), mg.apply(r))


@pytest.mark.timeout(120)
def test_all_odd_grid_over_the_cap_is_refused(E, oracle):
    from eddy_currents_3d_amd.solver import PRECOND_E_COARSE, EC3DError
    dims = (17, 17, 15)   # 4335 rows, no axis halves
    n = int(np.prod(dims))
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_COARSE
        assert s.preconditioner() == ("none", [])
        b = _rng(3).standard_normal(n)
        x, it, h = s.solve(b, np.zeros(n), TOL, 2000, hist_cap=2000)
    with E.EC3DSolver() as fresh:
        fresh.assemble_poisson(*dims)
        xf, itf, hf = fresh.solve(b, np.zeros(n), TOL, 2000, hist_cap=2000)
    assert it == itf and np.array_equal(x, xf) and np.array_equal(h, hf, equal_nan=True)


@pytest.mark.timeout(120)
def test_unit_vectors_at_corners_and_edges(E, oracle):
    dims = (48, 40, 33)
    sx, sy, sz = dims
    mg = M.MG(*dims)
    n = int(np.prod(dims))
    at = lambda i, j, k: k * sx * sy + j * sx + i
    probes = [at(i, j, k) for i in (0, sx - 1) for j in (0, sy - 1) for k in (0, sz - 1)]   # the corners
    probes += [at(sx // 2, 0, 0), at(0, sy // 2, sz - 1), at(sx - 1, sy - 1, sz // 2), at(1, 0, 1), at(sx - 2, sy - 1, 0)]
    with _handle(E, dims) as s:
        for q in probes:
            e = np.zeros(n)
            e[q] = 1.0
            assert np.array_equal(s.precond_apply(e), mg.apply(e)), q


# ---- B6: large ------------------------------------------------------------------------------------------------------
# The numpy side at 384x384x256 (37.7 M rows, 6 levels), measured: building the levels 6.6 s, one V-cycle 7.5 s and
# 11.5 GB peak resident memory on an 8-core build host; the whole test took 60 s on an MI355X machine.  The timeout
# leaves 10x that.
@pytest.mark.timeout(600)
def test_large_grid_two_iterations_equal_twin(E, oracle):
    dims = (384, 384, 256)   # above the undivided three-launch threshold (20 Mi rows) and the placement search (32 Mi)
    n = int(np.prod(dims))
    mg = M.MG(*dims)
    b = _rng(17).standard_normal(n)
    with _handle(E, dims) as s:
        assert s.preconditioner()[1] == [l.dims for l in mg.levels]
        assert np.array_equal(s.precond_apply(b), mg.apply(b))
        _assert_twin(s, mg, b, np.zeros(n), TOL, 1, 4, oracle)


@pytest.mark.timeout(600)
def test_bar_rhs_512_solves(E, oracle):
    from bench import bar_rhs
    N = 512
    b = bar_rhs(N)
    with _handle(E, (N, N, N)) as s:
        x1, it1, h1 = s.solve(b, np.zeros(N ** 3), TOL, 1000, hist_cap=64)
        x2, it2, h2 = s.solve(b, np.zeros(N ** 3), TOL, 1000, hist_cap=64)
        s.upload("B", b)
        s.upload("X", x1)
        res = s.true_residual()[0]
    print(f"512^3: {it1} outer iterations, true residual {res:.2e}")
    assert it1 <= 20 and res < TOL
    assert it1 == it2 and np.array_equal(x1, x2) and np.array_equal(h1, h2, equal_nan=True)


# ---- B7: lifecycle --------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_reassembly_drops_the_hierarchy(E, oracle):
    d1, d2 = (32, 32, 32), (40, 24, 16)
    n2 = int(np.prod(d2))
    b = _rng(19).standard_normal(n2)
    with E.EC3DSolver() as fresh:
        fresh.assemble_poisson(*d2)
        xf, itf, hf = fresh.solve(b, np.zeros(n2), TOL, 2000, hist_cap=400)
    with _handle(E, d1) as s:
        s.assemble_poisson(*d2)
        assert s.preconditioner() == ("none", [])
        x, it, h = s.solve(b, np.zeros(n2), TOL, 2000, hist_cap=400)
        assert it == itf and np.array_equal(x, xf) and np.array_equal(h, hf, equal_nan=True)
        s.set_preconditioner("mg")
        mg = M.MG(*d2)
        assert s.preconditioner() == ("mg", [l.dims for l in mg.levels])
        assert np.array_equal(s.precond_apply(b), mg.apply(b))


@pytest.mark.timeout(120)
def test_setting_again_replaces_the_sweep_counts(E, oracle):
    dims = (48, 40, 33)
    r = _rng(23).standard_normal(int(np.prod(dims)))
    with _handle(E, dims, sweeps=(3, 1, 16)) as s:
        s.set_preconditioner("mg", 1, 3, 4)
        assert np.array_equal(s.precond_apply(r), M.MG(*dims, pre=1, post=3, coarse_sweeps=4).apply(r))
        s.set_preconditioner("mg")
        assert np.array_equal(s.precond_apply(r), M.MG(*dims).apply(r))
