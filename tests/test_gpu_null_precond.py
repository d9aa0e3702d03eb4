"""N, the block multigrid preconditioner of the null projection's adjoint solves, on the device (ec3d_set_null_precond;
csrc/ec3d_mg.hip, csrc/ec3d_null.hip).  Shapes: the captured fixtures of 10-15 k unknowns, the
smallest with a conductor with a hole, two components, velocity terms and mixed BND (g3: one level; g8a, g9b: two).

1. null_precond_apply == the twin (tests/avmg_adjoint_numpy.py) BIT FOR BIT on two random r, both forms, with and
   without padded planes; the same handle's precond_apply and a plain solve afterwards are a fresh handle's bits;
2. THE TEST THAT SHOWS THE FEATURE DOES SOMETHING: the set-up with precond="block-mg" at null_tol 1e-10 keeps KEPT
   vectors, every component in strictly fewer adjoint iterations than the same handle with precond="none", residuals
   below the CPU test's BOUND, every vector within 1e-6 of the unpreconditioned device vector up to the sign,
   orthonormal to 1e-12, null_precond() reporting the twin's level dims;
3. with that Q every captured step reaches tol 1e-8 within itmax 2000 and ||P (b - A x)|| / ||b|| <= 2e-8;
4. block-mg-a reaches null_tol on g2, g3, g8a; on g9b the outcome is printed (the twin stalls there);
5. refusals leave the handle usable, the block hierarchy's own (five conducting domains) come back from the setter; 6. the setting survives a new assembly and changing it clears the vectors;
7. canaries and ghosts stay clean; 8. host.run on the shipped LIM input with null_precond="block-mg"."""
import numpy as np
import pytest

import guard_zones as Z
import null_projection_numpy as NP
from avmg_adjoint_numpy import AdjointAVMG
from avmg_numpy import level_dims
from conftest import load_golden
from eddy_currents_3d_amd.solver import NULL_E_MATRIX, NULL_E_SETUP
from test_null_precond_host import preconditioned_adjoint_solve, twin_for
from test_null_projection_host import BOUND, FOUR, KEPT

pytestmark = pytest.mark.gpu
G2, G3, G8A, G9B = FOUR
KINDS = {"block-mg": True, "block-mg-a": False}     # transposed_a of the twin


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _assemble(s, g):
    s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
    sdz, sdy, sdx = g["geoPHYS"].shape
    return (sdx, sdy, sdz)


_FRESH = {}


def _fresh(E, name, pitched, g, r):
    """M r of EC3D_PRECOND_BLOCK_MG and the unpreconditioned solve of step 0 on a handle that never saw N (the same
    plane pitch: the solve's sums follow the device layout)."""
    name = (name, pitched)
    if name not in _FRESH:
        with E.EC3DSolver() as s:
            _assemble(s, g)
            x, it, _ = s.solve(g["b0"], g["xin0"], float(g["tol"]), int(g["itmax"]))
            s.set_preconditioner("block-mg")
            _FRESH[name] = (s.precond_apply(r), x, it)
    return _FRESH[name]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name, pitched", [(G2, False), ("g2v_conducting_moving_16x15x14", False), (G3, False), (G8A, False),
                                           (G9B, False), (G2, True), (G3, True)])
def test_null_precond_apply_equals_the_twin_bit_for_bit(E, oracle, monkeypatch, name, pitched, kind):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    g = load_golden(name)
    r0 = np.random.default_rng(5).standard_normal(len(g["irow"]) - 1)
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    fresh_z, fresh_x, fresh_it = _fresh(E, name, pitched, g, r0)
    with E.EC3DSolver() as s:
        dims = _assemble(s, g)
        rm = s.row_map()
        assert (rm[dims[0] * dims[1]] - rm[0] > dims[0] * dims[1]) == pitched
        s.set_preconditioner("block-mg")                       # the caller's own M: N must leave it alone
        s.set_null_projection(True, precond=kind)
        twin = AdjointAVMG.from_solver(s, dims, transposed_a=KINDS[kind])
        rng = np.random.default_rng(11)
        for _ in range(2):
            r = rng.standard_normal(s.n)
            z, want = s.null_precond_apply(r), twin.apply(r)
            print(f"{name} pitched={pitched} {kind}: levels {len(twin.levels)}, components {len(twin.ucomps)}, "
                  f"rel diff {np.linalg.norm(z - want) / np.linalg.norm(want):.2e}")
            assert np.array_equal(z, want), f"{np.count_nonzero(z != want)} rows differ, max {np.abs(z - want).max():.3e}"
        assert s.preconditioner()[0] == "block-mg"
        assert not s.null_projection()["built"] and s.null_precond()[1] == []    # apply builds no Q and keeps no N
        zm = s.precond_apply(r0)
        assert np.array_equal(zm.view(np.uint64), fresh_z.view(np.uint64))
        s.set_preconditioner("none")
        s.set_null_projection(False)
        x, it, _ = s.solve(g["b0"], g["xin0"], float(g["tol"]), int(g["itmax"]))
        assert it == fresh_it and np.array_equal(x.view(np.uint64), fresh_x.view(np.uint64))


def _device_setup(s, precond, null_tol=1e-10):
    s.set_null_projection(True, null_tol, precond=precond)
    assert not s.null_projection()["built"]
    W = [s.left_null_vector(0)]
    info = s.null_projection()
    W += [s.left_null_vector(i) for i in range(1, info["kept"])]
    return info, W


@pytest.fixture(scope="module")
def setups(E, oracle):
    """Per fixture of FOUR, on one handle: the unpreconditioned set-up, then the one with block-mg."""
    out = {}
    for name in FOUR:
        g = load_golden(name)
        with E.EC3DSolver() as s:
            dims = _assemble(s, g)
            plain = _device_setup(s, "none")
            assert s.null_precond() == ("none", [], 0.0)
            pre = _device_setup(s, "block-mg")
            out[name] = dict(g=g, dims=dims, plain=plain, pre=pre, reported=s.null_precond())
    return out


@pytest.mark.parametrize("name", FOUR)
def test_setup_with_block_mg(oracle, setups, name):
    c = setups[name]
    g, (info, W), (pinfo, PW) = c["g"], c["pre"], c["plain"]
    n = len(g["irow"]) - 1
    twin = NP.setup_for(oracle, name, g)
    mg = twin_for(name, g)
    print(name, info)
    assert info["on"] and info["built"] and info["null_tol"] == 1e-10
    assert (info["found"], info["kept"], info["dropped"]) == (KEPT[name], KEPT[name], 0)
    assert pinfo["kept"] == KEPT[name]
    assert [r["seed_row"] for r in info["components"]] == twin["seeds"]
    for rec, prec, seed in zip(info["components"], pinfo["components"], twin["seeds"]):
        _, it_twin, _ = preconditioned_adjoint_solve(mg, twin["At"], n, seed)
        print(f"{name} seed {seed}: preconditioned adjoint solve {rec['iterations']} iterations (twin {it_twin}), "
              f"unpreconditioned {prec['iterations']}; residual {rec['residual']:.3e} (unpreconditioned {prec['residual']:.3e})")
        assert rec["kept"]
        assert 0 < rec["iterations"] <= NP.adjoint_cap(n)        # null_tol was reached
        assert rec["iterations"] < prec["iterations"]
        assert rec["residual"] <= BOUND
    for w, q in zip(W, PW):
        sign = 1.0 if w @ q > 0 else -1.0
        d = np.linalg.norm(sign * w - q)
        print(f"{name}: |w - w_unpreconditioned| = {d:.3e}")
        assert d <= 1e-6
    gram = np.array([[u @ v for v in W] for u in W])
    assert np.abs(gram - np.eye(len(W))).max() <= 1e-12
    kind, levels, ms = c["reported"]
    assert kind == "block-mg" and levels == level_dims(*c["dims"]) and ms > 0.0


@pytest.mark.parametrize("name", FOUR)
def test_reaches_1e_8_on_every_captured_step_with_the_preconditioned_q(E, oracle, setups, name):
    g = setups[name]["g"]
    A = NP.setup_for(oracle, name, g)["A"]
    tol, itmax = 1e-8, 2000
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.set_null_projection(True, precond="block-mg")
        W = None
        for k in range(len(g["iters"])):
            b, x0 = g[f"b{k}"], g[f"xin{k}"]
            x, it, _ = s.solve(b, x0, tol, itmax)
            if W is None:
                W = [s.left_null_vector(i) for i in range(s.null_projection()["kept"])]
                assert len(W) == KEPT[name] and s.null_precond()[0] == "block-mg"
            res = np.linalg.norm(NP.project(W, b - A(x))[0]) / np.linalg.norm(b)
            print(f"{name} step {k}: {it} iterations, ||P (b - A x)|| / ||b|| = {res:.3e}")
            assert it <= itmax
            assert res <= 2e-8


@pytest.mark.parametrize("name", FOUR)
def test_block_mg_a(E, name):
    g = load_golden(name)
    n = len(g["irow"]) - 1
    with E.EC3DSolver() as s:
        _assemble(s, g)
        try:
            info, W = _device_setup(s, "block-mg-a")
        except E.EC3DError as e:
            print(f"{name} block-mg-a: {e}")
            assert name == G9B and e.status == NULL_E_SETUP     # the twin stalls there: printed, not asserted
            return
        print(f"{name} block-mg-a: adjoint iterations {[c['iterations'] for c in info['components']]}, residuals "
              f"{[c['residual'] for c in info['components']]}")
        if name != G9B:
            assert info["kept"] == KEPT[name]
            assert all(0 < c["iterations"] <= NP.adjoint_cap(n) for c in info["components"])
        assert s.null_precond()[0] == "block-mg-a"


def test_refusals_leave_the_handle_usable(E):
    g = load_golden(G2)
    g8c = load_golden("g8c_side_by_side_20x18x14")
    tol, itmax = float(g["tol"]), int(g["itmax"])

    def refused(s, status, kind="block-mg"):
        with pytest.raises(E.EC3DError) as e:
            s.set_null_projection(True, precond=kind)
        assert e.value.status == status
        assert s.null_precond()[0] == "none" and not s.null_projection()["on"]
        with pytest.raises(E.EC3DError) as e:
            s.null_precond_apply(np.ones(s.n))
        assert e.value.status == status

    with E.EC3DSolver() as s:                        # Poisson
        s.assemble_poisson(16, 16, 16)
        refused(s, NULL_E_MATRIX)
        _, it, _ = s.solve(np.ones(s.n), np.zeros(s.n), 1e-8, 1000)
        assert it <= 1000
    with E.EC3DSolver() as s:                        # CSR
        s.set_matrix_csr(g["valA"], g["irow"], g["jcol"])
        refused(s, NULL_E_MATRIX, "block-mg-a")
        _, it, _ = s.solve(g["b0"], g["xin0"], tol, itmax)
        assert it == int(g["iters"][0])
    with E.EC3DSolver() as s:                        # bands + tail
        _assemble(s, g8c)
        assert s.info.tail_rows > 0
        refused(s, NULL_E_MATRIX)
        _, it, _ = s.solve(g8c["b0"], g8c["xin0"], float(g8c["tol"]), int(g8c["itmax"]))
        assert it == int(g8c["iters"][0])
    with E.EC3DSolver() as s:                        # an unknown kind, a negative count
        _assemble(s, g)
        for args in ((3, 0, 0, 0), (-1, 0, 0, 0), (1, -1, 0, 0)):
            assert s.L.ec3d_set_null_precond(s.h, *args) == 2
        assert s.null_precond()[0] == "none"
        with pytest.raises(E.EC3DError) as e:         # nothing set: nothing to apply
            s.null_precond_apply(np.ones(s.n))
        assert e.value.status == 3
        _, it, _ = s.solve(g["b0"], g["xin0"], tol, itmax)
        assert it == int(g["iters"][0])


def test_what_the_block_hierarchy_refuses_comes_back_from_the_setter(E):
    """Five conducting domains have more A-row classes than the block smoothers' table holds: EC3D_PRECOND_E_MATRIX from
    ec3d_set_null_precond, the setting as it was, the handle usable -- with four the setter accepts."""
    import multidomain_numpy as MD
    from eddy_currents_3d_amd import vxc
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX
    for D in (4, 5):
        vox, names = MD.blocks_model(D)
        t = vxc.domain_tables(vxc.VxcModel(vox, names, 0.004, (1.0, 1.0, 1.0)))
        with E.EC3DSolver() as s:
            s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
            if D == 4:
                s.set_null_projection(True, precond="block-mg-a")
                assert s.null_precond()[0] == "block-mg-a"
                continue
            s.set_null_projection(True, precond="none", pre=1)      # a setting to keep
            for kind in ("block-mg", "block-mg-a"):
                with pytest.raises(E.EC3DError) as e:
                    s.set_null_projection(True, precond=kind)
                assert e.value.status == PRECOND_E_MATRIX and "ec3d_set_null_precond" in str(e.value) and "4" in str(e.value)
                assert s.null_precond()[0] == "none" and s.null_projection()["on"]
            s.set_null_projection(False)
            r = np.random.default_rng(7).standard_normal(s.n)
            _, it, _ = s.solve(r, np.zeros_like(r), 1e-6, 300)
            assert it >= 1


def test_the_setting_survives_an_assembly_and_changing_it_clears_the_vectors(E):
    g2, g3 = load_golden(G2), load_golden(G3)
    with E.EC3DSolver() as s:
        s.set_null_projection(True, precond="block-mg", pre=1, post=1)      # before any matrix
        assert s.null_precond()[0] == "block-mg"
        dims = _assemble(s, g2)
        s.left_null_vector(0)
        q = s.null_projection()
        assert q["built"] and s.null_precond()[1] == level_dims(*dims)
        it_11 = q["components"][0]["iterations"]
        dims = _assemble(s, g3)                                              # a new matrix: Q goes, the setting stays
        assert s.null_precond()[0] == "block-mg" and s.null_precond()[1] == [] and not s.null_projection()["built"]
        s.left_null_vector(0)
        assert s.null_projection()["built"] and s.null_precond()[1] == level_dims(*dims)
        s.set_null_projection(True, precond="block-mg", pre=1, post=1)      # the same setting: Q stays
        assert s.null_projection()["built"]
        s.set_null_projection(True, precond="block-mg")                     # other sweep counts: Q is made again
        assert not s.null_projection()["built"]
        s.left_null_vector(0)
        s.set_null_projection(True, precond="none")
        assert not s.null_projection()["built"] and s.null_precond() == ("none", [], 0.0)
        w = s.left_null_vector(0)
        assert s.null_precond()[1] == [] and abs(np.linalg.norm(w) - 1.0) <= 1e-12
        print(f"g2 with 1 + 1 sweeps: {it_11} adjoint iterations")


@pytest.mark.parametrize("pitched", [False, True], ids=["auto", "pitched"])
def test_guards_stay_clean(E, monkeypatch, pitched):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    g = load_golden(G2)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        z = Z.zones(s.vector_layout(), Z.pitch_info(s, 16 * 15))
        s.set_null_projection(True, precond="block-mg")
        _, it, _ = s.solve(g["b0"], g["xin0"], 1e-8, 2000)
        assert it <= 2000 and s.null_projection()["kept"] == 1
        Z.assert_clean(s, z, f"pitched={pitched}: after a preconditioned set-up and a projected solve")
        s.set_null_projection(True, 1e-30, precond="block-mg")      # no fp64 iteration gets there
        with pytest.raises(E.EC3DError) as e:
            s.solve(g["b0"], g["xin0"], 1e-8, 2000)
        assert e.value.status == NULL_E_SETUP and "component 0" in str(e.value)
        Z.assert_clean(s, z, f"pitched={pitched}: after a preconditioned set-up that failed")


def test_host_run_on_lim(E):
    """Either the set-up succeeds and every step's projected true residual is below the model's tol, or it fails with
    EC3D_NULL_E_SETUP naming the component; the unpreconditioned run of this call is known to fail."""
    from eddy_currents_3d_amd import host, vxc
    g = load_golden("g4_LIM")
    model = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    tol = float(g["tol"])
    seen, W = [], []

    def on_solved(k, s, info):
        if not W:
            W.extend(s.left_null_vector(i) for i in range(s.null_projection()["kept"]))
        b = s.download("B")
        r = NP.project(W, b - s.spmv(s.download("X")))[0]
        info["pres"] = float(np.linalg.norm(r) / np.linalg.norm(b))
        seen.append(info)

    with E.EC3DSolver() as s:
        try:
            host.run(model, s, steps=3, on_solved=on_solved, null_projection=True, null_tol=1e-8, null_precond="block-mg")
        except E.EC3DError as e:
            print(f"LIM, block-mg, null_tol 1e-8: {e}")
            assert e.status == NULL_E_SETUP and "component" in str(e)
            return
        q = s.null_projection()
        print(f"LIM, block-mg, null_tol 1e-8: adjoint iterations {[c['iterations'] for c in q['components']]}, "
              f"set-up {q['setup_ms']:.0f} ms, {s.null_precond()}")
    assert len(seen) == 3
    for k, info in enumerate(seen):
        print(f"LIM step {k}: {info['iter']} iterations, projected true residual {info['pres']:.3e}")
        assert info["pres"] < tol
