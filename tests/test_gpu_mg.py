"""Multigrid-preconditioned solve of the single-component operator (ec3d_set_preconditioner, csrc/ec3d_mg.hip).

* precond_apply (one V-cycle) == the numpy restatement tests/mg_numpy.py BIT FOR BIT: no reduction enters a V-cycle
  and every elementwise operation is restated in the kernels' order, with fused multiply-add off on both sides;
* the level operators are the oracle's poisson_csr at the level's dims and spacing: the restatement builds its levels
  from oracle.poisson_csr, so the bitwise equality above on a 4-level hierarchy (96x80x72: every axis halves at every
  level, so the spacing stays isotropic), on a semi-coarsened one (48x40x33: z keeps its cells and spacing) and on
  unit vectors at a small size holds only if every device level has the same coefficients (distinct spacings per axis
  and distinct BND faces: tests/test_gpu_mg_twin.py);
* solves to 1e-8 with the bar RHS at 64^3, 128^3, 256^3 in <= 20 outer iterations, the true residual below tol, and at
  256^3 x at g5_cube256's probes within 10 tol of the reference's converged x (4 097 reference iterations);
* warm start and a forced restart converge; switching back to EC3D_PRECOND_NONE gives a fresh handle's result bit
  for bit; A-V, CSR and slab handles are refused with their status and stay usable."""
import numpy as np
import pytest

import mg_numpy as M

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dims, dictionary", [((64, 64, 64), True), ((96, 80, 72), True), ((48, 40, 33), False)])
def test_precond_apply_equals_restatement(E, oracle, dims, dictionary):
    mg = M.MG(*dims)
    r = np.random.Generator(np.random.PCG64(7)).standard_normal(int(np.prod(dims)))
    with E.EC3DSolver(dictionary=dictionary) as s:
        s.assemble_poisson(*dims)
        s.set_preconditioner("mg")
        kind, levels = s.preconditioner()
        assert kind == "mg" and levels == [l.dims for l in mg.levels]
        z = s.precond_apply(r)
    zr = mg.apply(r)
    rel = np.linalg.norm(z - zr) / np.linalg.norm(zr)
    print(f"{dims} dictionary={dictionary}: levels {levels}, rel diff {rel:.2e}, bitwise {np.array_equal(z, zr)}")
    assert rel <= 1e-13
    assert np.array_equal(z, zr)


@pytest.mark.timeout(120)
def test_level_operators_through_unit_vectors(E, oracle):
    dims = (32, 16, 16)  # two levels: 32x16x16, 16x8x8 (spacing doubled on every axis)
    mg = M.MG(*dims)
    n = int(np.prod(dims))
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_preconditioner("mg")
        for q in (0, 1, 31, 32 * 16 * 8 + 16 * 8 + 7, n - 1):
            e = np.zeros(n)
            e[q] = 1.0
            assert np.array_equal(s.precond_apply(e), mg.apply(e)), q


@pytest.mark.timeout(480)
@pytest.mark.parametrize("N", [64, 128, 256])
def test_bar_rhs_solves_in_few_iterations(E, oracle, N):
    from bench import bar_rhs
    with E.EC3DSolver() as s:
        s.assemble_poisson(N, N, N)
        s.set_preconditioner("mg")
        s.upload("B", bar_rhs(N))
        s.upload("X", np.zeros(N ** 3))
        it, hist = s.solve_resident(TOL, 1000, hist_cap=64)
        res, _ = s.true_residual()
        x = s.download("X")
    print(f"{N}^3: {it} outer iterations, true residual {res:.2e}, ||R|| history {hist[:it, 1]}")
    assert it <= 20
    assert res < TOL
    if N == 256:
        from conftest import load_golden
        g = load_golden("g5_cube256")
        d = np.abs(x[g["probes"]] - g["xprobe"]).max() / np.abs(g["xprobe"]).max()
        print(f"probes vs the reference's converged x: max diff {d:.2e} of the largest")
        assert d <= 10 * TOL


@pytest.mark.timeout(120)
def test_warm_start_and_forced_restart(E, oracle):
    from bench import bar_rhs
    N = 64
    b = bar_rhs(N)
    with E.EC3DSolver() as s:
        s.assemble_poisson(N, N, N)
        s.set_preconditioner("mg")
        x0, it0, _ = s.solve(b, np.zeros(N ** 3), TOL, 100)
        # warm start from a perturbed solution
        xw = x0 + 1e-3 * np.abs(x0).max() * np.random.Generator(np.random.PCG64(3)).standard_normal(N ** 3)
        x1, it1, _ = s.solve(b, xw, TOL, 100)
        s.upload("B", b)
        s.upload("X", x1)
        assert s.true_residual()[0] < TOL and 1 <= it1 <= 20
        # a tolerance the restart test (|r.r0| / ||b|| < tol) meets long before the residual one does: restarts fire
        x2, it2, _ = s.solve(b * 1e-6, np.zeros(N ** 3), 1e-2, 100)
        s.upload("B", b * 1e-6)
        s.upload("X", x2)
        assert s.restart_count() >= 1
        assert s.true_residual()[0] < 1e-2
    print(f"cold {it0}, warm {it1}, restart case {it2}")


@pytest.mark.timeout(120)
def test_switching_back_to_none_is_a_fresh_handle(E, oracle):
    from bench import bar_rhs
    N = 32
    b = bar_rhs(N)
    with E.EC3DSolver() as fresh:
        fresh.assemble_poisson(N, N, N)
        xf, itf, hf = fresh.solve(b, np.zeros(N ** 3), TOL, 2000, hist_cap=2000)
    with E.EC3DSolver() as s:
        s.assemble_poisson(N, N, N)
        s.set_preconditioner("mg")
        xm, itm, _ = s.solve(b, np.zeros(N ** 3), TOL, 2000)
        s.set_preconditioner("none")
        assert s.preconditioner() == ("none", [])
        xn, itn, hn = s.solve(b, np.zeros(N ** 3), TOL, 2000, hist_cap=2000)
    assert itm < itf
    assert itn == itf and np.array_equal(xn, xf) and np.array_equal(hn, hf, equal_nan=True)


@pytest.mark.timeout(120)
def test_other_matrices_are_refused_and_stay_usable(E, oracle):
    from eddy_currents_3d_amd.solver import PRECOND_E_COARSE, PRECOND_E_MATRIX, EC3DError
    from conftest import load_golden
    g = load_golden("g2_conducting_hole_16x15x14")
    with E.EC3DSolver() as s:  # A-V
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_MATRIX
        assert s.preconditioner() == ("none", [])
        x, it, _ = s.solve(g["b0"], g["xin0"], float(g["tol"]), int(g["itmax"]))
        assert it == int(g["iters"][0])
    valA, irow, jcol = oracle.poisson_csr(32, 32, 32)
    with E.EC3DSolver() as s:  # CSR of the same operator
        s.set_matrix_csr(valA, irow, jcol)
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_MATRIX
        b = oracle.bar_rhs(32)
        x, it, _ = s.solve(b, np.zeros(32 ** 3), TOL, 2000)
        assert it > 20
    with E.EC3DSolver() as s:  # a z-slab
        s.assemble_poisson(32, 32, 32, slab=(0, 16))
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_MATRIX
    with E.EC3DSolver() as s:  # a prime-sized box: the coarsest level would be the grid itself
        s.assemble_poisson(67, 67, 67)
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_COARSE
        assert s.preconditioner() == ("none", [])
    with E.EC3DMulti(nranks=1) as m:  # the slab handle of ec3d_multi
        m.assemble_poisson(32, 32, 32)
        h, _, _ = m.slab(0)
        with pytest.raises(EC3DError) as e:
            h.set_preconditioner("mg")
        assert e.value.status == PRECOND_E_MATRIX
