"""The left-null-vector projection of the A-V system on the device (ec3d_spmv_t, ec3d_set_null_projection;
csrc/ec3d_transpose.hip, csrc/ec3d_null.hip).

* ec3d_spmv_t == the twin's ordered transposed product (tests/null_projection_numpy.py) BIT FOR BIT on six fixtures,
  with and without padded planes (g8c is stored as bands + tail and is refused like any such matrix; g8d stands beside
  it), for a random x that is non-zero next to every box face; and == the transpose of
  ec3d_export_csr applied in numpy to 1e-13 * sum |terms|; ghosts, rows [n, n_pad) and the rows of no unknown stay zero;
* set-up: components kept 1, 1, 2, 1 on g2, g3, g8a, g9b, adjoint residuals below the CPU test's bound, iterations below
  the cap, ec3d_left_null_vector within 1e-6 of the twin's w up to the sign;
* THE TEST THAT FAILS WITHOUT THE FEATURE: tol = 1e-8, itmax = 2000 on every captured step -- with the projection
  iter <= 2000 and ||P (b - A x)|| / ||b|| <= 2e-8, without it iter = itmax + 1;
* ec3d_null_project == the twin's project_device BIT FOR BIT -- R, R0 and P of a solve with itmax = -1 (the residual launch,
  the projection and the set-up, no iteration) against the projection of the same call's R with the projection off -- on g2,
  pitched and not, and on a 96 x 96 x 64 box whose device rows exceed 1024 chunks: the second trip of the kernels' chunk loop;
* at the fixtures' own tolerance x is within 10 tol of the captured xout on the A blocks (U printed, not asserted);
* off is a fresh handle's bits; B keeps its bytes; guess history on top; refusals; host.run."""
import numpy as np
import pytest

import guard_zones as Z
import null_projection_numpy as NP
from conftest import load_golden
from eddy_currents_3d_amd.solver import NULL_E_MATRIX
from test_null_projection_host import BOUND, FOUR, KEPT

pytestmark = pytest.mark.gpu
SIX = ["g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14", "g3_moving_coil_18x16x12",
       "g8a_two_plates_18x16x16", "g8c_side_by_side_20x18x14", "g9b_L_hole_near_faces_17x16x16"]
# g8c numbers its U unknowns domain by domain, not in scan order, so ec3d_assemble stores it as bands + tail
# (tests/test_gpu_multidomain.py, STRUCTURED): there the transposed product is refused, as for every bands + tail matrix,
# and that is what its case asserts.  g8d -- two touching domains in the structured form -- stands beside it.
CASES = SIX + ["g8d_g3_split_18x16x12"]
BIG_NULL_TOL = 1e-10
BANDS_AND_TAIL = {"g8c_side_by_side_20x18x14"}


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _assemble(s, g):
    s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))


def _x_for(g, seed):
    """Random, and non-zero next to every face of the box in every block that has an unknown there."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(len(g["irow"]) - 1)
    x[x == 0.0] = 1.0
    return x


@pytest.mark.parametrize("pitched", [False, True], ids=["auto", "pitched"])
@pytest.mark.parametrize("name", CASES)
def test_spmv_t_equals_the_twin_bit_for_bit(E, monkeypatch, name, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    g = load_golden(name)
    sdz, sdy, sdx = g["geoPHYS"].shape
    with E.EC3DSolver() as s:
        _assemble(s, g)
        structured = s.info.tail_rows == 0 and s.info.dict_classes > 0
        assert structured == (name not in BANDS_AND_TAIL)
        if not structured:
            with pytest.raises(E.EC3DError) as err:
                s.spmv_t(_x_for(g, 1))
            assert err.value.status == NULL_E_MATRIX
            return
        rm = s.row_map()
        assert (rm[sdx * sdy] - rm[0] > sdx * sdy) == pitched
        valA, irow, jcol = s.export_csr()
        # the handle's matrix is the captured one, so the twin of either is the same
        assert np.array_equal(irow, g["irow"]) and np.array_equal(jcol, g["jcol"]) and np.array_equal(valA, g["valA"])
        At = NP.Ordered.of_csr_t(valA, irow, jcol)
        z = Z.zones(s.vector_layout(), Z.pitch_info(s, sdx * sdy))
        for seed in (1, 2):
            x = _x_for(g, seed)
            y = s.spmv_t(x)
            want = At(x)
            assert np.array_equal(y.view(np.uint64), want.view(np.uint64)), \
                f"{np.count_nonzero(y != want)} rows differ, max {np.abs(y - want).max():.3e}"
            row = np.repeat(np.arange(len(irow) - 1), np.diff(irow.astype(np.int64)))
            ref = np.zeros_like(x)
            np.add.at(ref, jcol.astype(np.int64) - 1, valA * x[row])
            assert np.all(np.abs(y - ref) <= 1e-13 * At.abs_sum(x))
            Z.assert_clean(s, z, f"{name} pitched={pitched}: after ec3d_spmv_t")
        e = np.zeros_like(x)        # a unit vector on a U row: one column of A^T, the adjoint solve's right-hand side
        e[NP.seed_rows(g["geoPHYS_C"])[0]] = 1.0
        assert np.array_equal(s.spmv_t(e), At(e))


@pytest.fixture(scope="module")
def setups(E, oracle):
    """Per fixture of FOUR: the twin's set-up, and what the device reported and returned for its own."""
    out = {}
    for name in FOUR:
        g = load_golden(name)
        with E.EC3DSolver() as s:
            _assemble(s, g)
            s.set_null_projection(True)
            assert not s.null_projection()["built"]
            W = [s.left_null_vector(0)]
            info = s.null_projection()
            W += [s.left_null_vector(i) for i in range(1, info["kept"])]
        out[name] = dict(g=g, twin=NP.setup_for(oracle, name, g), info=info, W=W)
    return out


@pytest.mark.parametrize("name", FOUR)
def test_setup(setups, name):
    c = setups[name]
    info, twin, g = c["info"], c["twin"], c["g"]
    n = len(g["irow"]) - 1
    print(name, info)
    assert info["on"] and info["built"] and info["null_tol"] == 1e-10
    assert (info["found"], info["kept"], info["dropped"]) == (KEPT[name], KEPT[name], 0)
    assert [r["seed_row"] for r in info["components"]] == twin["seeds"]
    for rec, trec in zip(info["components"], twin["info"]):
        assert rec["kept"]
        assert rec["residual"] <= BOUND
        assert 0 < rec["iterations"] <= NP.adjoint_cap(n)
        print(f"{name}: adjoint solve {rec['iterations']} iterations (twin {trec['iterations']}), "
              f"residual {rec['residual']:.3e} (twin {trec['residual']:.3e})")
    for w, q in zip(c["W"], twin["Q"]):
        sign = 1.0 if w @ q > 0 else -1.0
        d = np.linalg.norm(sign * w - q) / np.linalg.norm(q)
        print(f"{name}: |w - w_twin| / |w_twin| = {d:.3e}")
        assert abs(np.linalg.norm(w) - 1.0) <= 1e-12
        assert d <= 1e-6
    for i, u in enumerate(c["W"]):
        for v in c["W"][:i]:
            assert abs(u @ v) <= 1e-12


@pytest.mark.parametrize("name", FOUR)
def test_reaches_1e_8_on_every_captured_step(E, oracle, setups, name):
    """Fails without the feature: the unprojected solve runs into itmax on every one of these steps."""
    c = setups[name]
    g, W = c["g"], c["W"]
    A = c["twin"]["A"]
    tol, itmax = 1e-8, 2000
    with E.EC3DSolver() as s:
        _assemble(s, g)
        for k in range(len(g["iters"])):
            b, x0 = g[f"b{k}"], g[f"xin{k}"]
            s.set_null_projection(True)
            x, it, _ = s.solve(b, x0, tol, itmax)
            info = s.null_projection()
            res = np.linalg.norm(NP.project(W, b - A(x))[0]) / np.linalg.norm(b)
            s.set_null_projection(False)
            xo, ito, _ = s.solve(b, x0, tol, itmax)
            print(f"{name} step {k}: projection on {it} iterations, removed {info['removed']:.3e}, "
                  f"||P (b - A x)|| / ||b|| = {res:.3e}; off {ito} iterations")
            assert it <= itmax
            assert res <= 2e-8
            assert ito == itmax + 1
            wb = np.sqrt(sum((w @ (b - A(x0))) ** 2 for w in W)) / np.linalg.norm(b)
            assert abs(info["removed"] - wb) <= 1e-6 * wb + 1e-12


def _g2_args():
    g = load_golden("g2_conducting_hole_16x15x14")
    return (g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))


def _big_args():
    from test_gpu_field_integrals import big_box
    return big_box()


# null_tol of the big box: the bits of a projection do not depend on how accurate Q is (docs/rounds/r10.md has the adjoint
# solve's iterations at this value)
@pytest.mark.parametrize("args_of, pitched, null_tol", [(_g2_args, False, 1e-10), (_g2_args, True, 1e-10),
                                                        (_big_args, False, BIG_NULL_TOL)],
                         ids=["g2-auto", "g2-pitched", "big"])
def test_projection_equals_the_twin_bit_for_bit(E, monkeypatch, args_of, pitched, null_tol):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    args = args_of()
    n_ref = 3 * args[0].size + int(np.count_nonzero(args[1]))
    rng = np.random.default_rng(16)
    x, b = rng.standard_normal(n_ref), rng.standard_normal(n_ref)
    tol = 1e-8

    def set_up_only(s):
        s.upload("X", x)
        s.upload("B", b)
        it, _ = s.solve_resident(tol, -1)
        assert it == 0
        return [s.download(w) for w in ("R", "R0", "P")]

    with E.EC3DSolver() as s:
        s.assemble(*args)
        plain = set_up_only(s)
        assert all(np.array_equal(v.view(np.uint64), plain[0].view(np.uint64)) for v in plain)
        s.set_null_projection(True, null_tol)
        s.upload("B", b)
        s.upload("X", np.zeros(n_ref))
        s.solve_resident(tol, 0)                      # any solve: the vectors are built in front of it
        info = s.null_projection()
        print(f"null_tol {null_tol:g}: {info['kept']} kept, adjoint iterations "
              f"{[c['iterations'] for c in info['components']]}, set-up {info['setup_ms']:.0f} ms")
        assert info["built"] and info["kept"] >= 1
        W = [s.left_null_vector(i) for i in range(info["kept"])]
        got = set_up_only(s)
        removed = s.null_projection()["removed"]
        lay, rm = s.vector_layout(), s.row_map().astype(np.int64)
    n, n_pad = int(lay["n"]), int(lay["n_pad"])
    assert (n_pad // 512 > 1024) == (args_of is _big_args)      # the big box: workgroups 0 ... take a second chunk

    def to_dev(v):
        d = np.zeros(n_pad)
        d[rm] = v
        return d
    want, c, _ = NP.project_device([to_dev(w) for w in W], to_dev(plain[0]), n)
    want = want[rm]
    for name, v in zip(("R", "R0", "P"), got):
        assert np.array_equal(v.view(np.uint64), want.view(np.uint64)), \
            f"{name}: {np.count_nonzero(v != want)} rows differ, max {np.abs(v - want).max():.3e}"
    assert not np.array_equal(want, plain[0])         # (it did something)
    wb = float(np.sqrt(c @ c) / np.linalg.norm(b))
    print(f"removed {removed:.6e}, twin {wb:.6e}")
    assert abs(removed - wb) <= 1e-6 * wb + 1e-12


@pytest.mark.parametrize("name", FOUR)
def test_fixture_tolerance_lands_on_the_captured_solution(E, setups, name):
    g = setups[name]["g"]
    tol, itmax = float(g["tol"]), int(g["itmax"])
    nA = 3 * g["geoPHYS"].size
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.set_null_projection(True)
        for k in range(len(g["iters"])):
            x, it, _ = s.solve(g[f"b{k}"], g[f"xin{k}"], tol, itmax)
            xr = g[f"xout{k}"]
            dA = np.linalg.norm(x[:nA] - xr[:nA]) / np.linalg.norm(xr[:nA])
            dU = np.linalg.norm(x[nA:] - xr[nA:]) / max(np.linalg.norm(xr[nA:]), 1e-300)
            # U is fixed by the system only up to a constant per conducting component: printed, not asserted
            print(f"{name} step {k}: {it} iterations (reference {int(g['iters'][k])}), |x_A - x_A,ref| = {dA:.2e} "
                  f"({dA / tol:.2f} tol), |U - U_ref| = {dU:.2e}")
            assert it <= itmax
            assert dA <= 10 * tol


def test_off_is_a_fresh_handles_bits_and_b_keeps_its_bytes(E):
    g = load_golden("g3_moving_coil_18x16x12")
    tol, itmax = float(g["tol"]), int(g["itmax"])
    b, x0 = g["b1"], g["xin1"]
    with E.EC3DSolver() as fresh:
        _assemble(fresh, g)
        x_f, it_f, h_f = fresh.solve(b, x0, tol, itmax, hist_cap=64)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        assert not s.null_projection()["on"]
        x_a, it_a, h_a = s.solve(b, x0, tol, itmax, hist_cap=64)          # never switched on
        s.set_null_projection(True)
        s.upload("B", b)
        s.upload("X", x0)
        before = s.download("B")
        it_on, h_on = s.solve_resident(tol, itmax, hist_cap=64)
        assert np.array_equal(s.download("B").view(np.uint64), before.view(np.uint64))   # B is the caller's
        assert np.array_equal(before, b)
        assert s.null_projection()["built"] and s.null_projection()["removed"] > 0.0
        assert not np.array_equal(h_on, h_a, equal_nan=True)              # (it did something)
        x_on2, it_on2, h_on2 = s.solve(b, x0, tol, itmax, hist_cap=64)    # a solve is a pure function of its inputs
        assert it_on2 == it_on and np.array_equal(h_on2, h_on, equal_nan=True)
        s.set_null_projection(False)
        x_b, it_b, h_b = s.solve(b, x0, tol, itmax, hist_cap=64)          # switched off again
    for x, it, h in ((x_a, it_a, h_a), (x_b, it_b, h_b)):
        assert it == it_f == int(g["iters"][1])
        assert np.array_equal(x.view(np.uint64), x_f.view(np.uint64))
        assert np.array_equal(h, h_f, equal_nan=True)


def test_guess_history_on_top(E, oracle, setups):
    c = setups["g3_moving_coil_18x16x12"]
    g, W, A = c["g"], c["W"], c["twin"]["A"]
    with E.EC3DSolver() as s:
        s.set_guess_history(4)
        _assemble(s, g)
        s.set_null_projection(True)
        x = g["xin0"]
        for k in range(3):
            b = g[f"b{k}"]
            x, it, _ = s.solve(b, x, 1e-8, 2000)
            res = np.linalg.norm(NP.project(W, b - A(x))[0]) / np.linalg.norm(b)
            print(f"g3 step {k} with guess history 4: {it} iterations, projected true residual {res:.3e}, "
                  f"history {s.guess_history()['stored']} pairs")
            assert it <= 2000 and res <= 2e-8
        assert s.guess_history()["stored"] >= 1


def test_a_new_matrix_clears_the_vectors_and_keeps_the_setting(E, setups):
    g2, g8 = setups["g2_conducting_hole_16x15x14"]["g"], setups["g8a_two_plates_18x16x16"]["g"]
    with E.EC3DSolver() as s:
        _assemble(s, g2)
        s.set_null_projection(True)
        _, it, _ = s.solve(g2["b0"], g2["xin0"], 1e-8, 2000)
        assert it <= 2000 and s.null_projection()["kept"] == 1
        _assemble(s, g8)
        q = s.null_projection()
        assert q["on"] and not q["built"] and q["kept"] == 0
        _, it, _ = s.solve(g8["b0"], g8["xin0"], 1e-8, 2000)             # rebuilt by the first solve
        q = s.null_projection()
        assert it <= 2000 and q["built"] and q["kept"] == 2


def test_refusals_leave_the_setting_off(E, oracle):
    from eddy_currents_3d_amd.dist import HipAVSlabOps
    from eddy_currents_3d_amd.solver import NULL_E_MATRIX
    g = load_golden("g2_conducting_hole_16x15x14")
    tol, itmax = float(g["tol"]), int(g["itmax"])

    def refused(s, status):
        with pytest.raises(E.EC3DError) as e:
            s.set_null_projection(True)
        assert e.value.status == status
        assert not s.null_projection()["on"]

    with E.EC3DSolver() as s:                        # Poisson
        s.assemble_poisson(16, 16, 16)
        refused(s, NULL_E_MATRIX)
        with pytest.raises(E.EC3DError) as e:
            s.spmv_t(np.ones(s.n))
        assert e.value.status == NULL_E_MATRIX
    with E.EC3DSolver() as s:                        # CSR, also one the library recognises as an A-V system
        s.set_matrix_csr(g["valA"], g["irow"], g["jcol"])
        refused(s, NULL_E_MATRIX)
        x, it, _ = s.solve(g["b0"], g["xin0"], tol, itmax)
        assert it == int(g["iters"][0])
    with E.EC3DSolver(structured=False) as s:        # bands + tail (ec3d_set_structured(h, 0))
        _assemble(s, g)
        refused(s, NULL_E_MATRIX)
        x, it, _ = s.solve(g["b0"], g["xin0"], tol, itmax)
        assert it == int(g["iters"][0])
    sdz = g["geoPHYS"].shape[0]
    ops = HipAVSlabOps(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]), 0, sdz // 2, 2,
                       structured=True)              # a z-slab
    try:
        refused(ops.local, 4)
    finally:
        ops.close()
    with E.EC3DSolver() as s:                        # a setting made before an ineligible matrix: the solve says so
        s.set_null_projection(True)
        s.assemble_poisson(16, 16, 16)
        with pytest.raises(E.EC3DError) as e:
            s.solve(np.ones(s.n), np.zeros(s.n), 1e-8, 100)
        assert e.value.status == NULL_E_MATRIX
        s.set_null_projection(False)
        _, it, _ = s.solve(np.ones(s.n), np.zeros(s.n), 1e-8, 1000)
        assert it <= 1000


def test_host_run_two_steps(E):
    from eddy_currents_3d_amd import host
    from test_gpu_domain_integrals import g3_model
    g = load_golden("g3_moving_coil_18x16x12")
    model = g3_model()
    seen = []

    def on_solved(k, s, info):
        info["res"] = s.true_residual()[0]
        seen.append(info)

    with E.EC3DSolver() as s:
        log = host.run(model, s, steps=2, on_solved=on_solved, null_projection=True, tol=1e-7)
        assert s.null_projection()["on"]
    assert len(log) == 2
    for k, info in enumerate(seen):
        q = info["null"]
        print(f"g3 model step {k}: {info['iter']} iterations, true residual {info['res']:.2e}, removed {q['removed']:.2e}")
        assert q["built"] and q["kept"] == 1
        assert info["iter"] <= int(g["itmax"])


def test_a_vector_that_missed_null_tol_is_never_used(E):
    from eddy_currents_3d_amd.solver import NULL_E_SETUP
    g = load_golden("g2_conducting_hole_16x15x14")
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.set_null_projection(True, 1e-30)             # no fp64 iteration gets there
        with pytest.raises(E.EC3DError) as e:
            s.solve(g["b0"], g["xin0"], 1e-8, 2000)
        assert e.value.status == NULL_E_SETUP
        assert "component 0" in str(e.value) and "seed row 10242" in str(e.value)
        q = s.null_projection()
        assert q["on"] and not q["built"] and q["kept"] == 0
        z = Z.zones(s.vector_layout(), Z.pitch_info(s, 16 * 15))
        Z.assert_clean(s, z, "after a set-up that failed")       # whatever the adjoint iteration ended in
        s.set_null_projection(True)                    # the default accuracy: the same handle works
        _, it, _ = s.solve(g["b0"], g["xin0"], 1e-8, 2000)
        assert it <= 2000 and s.null_projection()["kept"] == 1
        Z.assert_clean(s, z, "after a set-up and a projected solve")
