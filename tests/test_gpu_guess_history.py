"""GPU: solves started from the projection onto earlier solutions (ec3d_set_guess_history, csrc/ec3d_guess.hip).

* bit for bit against tests/guess_history_numpy.py after each of five consecutive solves with depth 2 -- x, the iteration
  count, the ||S|| / ||R|| history, the projection's coefficients, stored and kept -- on Poisson boxes (padding rows, both
  formats), a bands + tail matrix, the structured A-V form (plane pitch auto and forced), the same system as bands + tail,
  two conducting domains, and under the multigrid preconditioner;
* right-hand sides from a two-dimensional space: the bounds of tests/test_guess_history_host.py, on the device;
* the contract: depth 0 is a fresh handle's bits and memory; a zero right-hand side leaves x and the history alone; a
  solve driven to NaN clears the history and the next clean solve is a fresh handle's; a new matrix and a new depth clear
  it; a handle on adopted vectors between canaries keeps every zone clean; slabs refuse with 4 and solve as before;
* the drop-in symbol with EC3D_GUESS_HISTORY=2, in a process of its own (the variable is read once): the handle's bits;
* host.run on the LIM input with guess_history=4: every step's true residual below the model's tolerance."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import csr_generate as G
import guard_zones as Z
import guess_history_numpy as GH
import mg_numpy as M
from conftest import load_golden
from test_guess_history_host import family_rhs

pytestmark = pytest.mark.gpu

AV = {"g2": "g2_conducting_hole_16x15x14", "g8a": "g8a_two_plates_18x16x16"}
SCALES = (1.0, -0.5, 2.0, 1.0, 0.25)
BIG_ITMAX = 12     # 97 x 81 x 77 needs 494 iterations to 1e-5, 23 ms each in the CPU twin: five solves of 13 iterations instead


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def bar_rhs_box(dims):
    """oracle.bar_rhs's bar on a box: mu0 * 1e6 on the cells i, k within [N/2 - 2, N/2 + 3], j within [N/4, 3 N/4] of
    their own axis (1-based, inclusive; clipped to the box)."""
    sdx, sdy, sdz = dims
    b = np.zeros((sdz, sdy, sdx))
    b[max(sdz // 2 - 3, 0):sdz // 2 + 3, max(sdy // 4 - 1, 0):3 * sdy // 4, max(sdx // 2 - 3, 0):sdx // 2 + 3] = \
        0.12566370964050292e-05 * 1e6
    return b.reshape(-1)


def info_line(i):
    return (f"used {i['used']} kept {i['kept']} stored {i['stored']} res {i['res_before']:.3e} -> {i['res_after']:.3e} "
            f"coef {np.array2string(i['coef'], precision=3)}")


def check_sequence(s, twin, rhs, x0, tol, itmax, cap, where):
    """Five solves in a row on the handle and on the twin, x carried on each side: everything equal after every solve."""
    x, xt = np.array(x0), np.array(x0)
    seen = []
    for t, b in enumerate(rhs):
        x, it, hist = s.solve(b, x, tol, itmax, hist_cap=cap)
        got = s.guess_history()
        xt, itt, hs, hr = twin.step(b, xt)[:4]
        want = twin.info
        print(f"{where} solve {t}: iter {it} (twin {itt}); {info_line(got)}")
        assert it == itt, (where, t)
        assert np.array_equal(hist[:, 0], hs, equal_nan=True) and np.array_equal(hist[:, 1], hr, equal_nan=True), (where, t)
        assert (got["used"], got["kept"], got["stored"]) == (want["used"], want["kept"], want["stored"]), (where, t, got, want)
        assert got["coef"].tobytes() == np.asarray(want["coef"], np.float64).tobytes(), (where, t, got["coef"], want["coef"])
        assert np.array_equal(x, xt), (where, t, np.abs(x - xt).max())
        assert got["res_before"] == pytest.approx(want["res_before"], rel=1e-9)
        assert got["res_after"] == pytest.approx(want["res_after"], rel=1e-9)
        seen.append(got)
    return seen


# ---- the twin, bit for bit ---------------------------------------------------------------------------------------------
# 97 x 81 x 77: 604 989 rows, an odd count (the last pair of rows is half masked) in 1182 chunks of 512 -- more than the 1024
# workgroups of a streaming launch, so workgroups 0 ... 157 take a second chunk.  Its itmax keeps the twin's CPU solves short;
# the comparison is the same.
PADDING = {(17, 9, 5): 259, (97, 81, 77): 195}


@pytest.mark.parametrize("dims, dictionary, itmax", [((17, 9, 5), True, 2000), ((16, 16, 16), True, 2000),
                                                     ((16, 16, 16), False, 2000), ((97, 81, 77), True, BIG_ITMAX)],
                         ids=["17x9x5", "16x16x16", "16x16x16-bands", "97x81x77"])
def test_poisson_equals_twin(E, oracle, dims, dictionary, itmax):
    valA, irow, jcol = oracle.poisson_csr(*dims)
    b0 = oracle.bar_rhs(dims[0]) if dims[0] == dims[1] == dims[2] else bar_rhs_box(dims)
    tol, cap = 1e-5, 48
    with E.EC3DSolver(dictionary=dictionary) as s:
        s.assemble_poisson(*dims)
        lay = s.vector_layout()
        assert lay["n_pad"] - lay["n"] == PADDING.get(dims, 0)
        assert (lay["n_pad"] // 512 > 1024) == (dims == (97, 81, 77))
        s.set_guess_history(2)
        twin = GH.for_handle(oracle, s, valA, irow, jcol, 2, tol, itmax, cap)
        seen = check_sequence(s, twin, [a * b0 for a in SCALES], np.zeros(len(b0)), tol, itmax, cap, f"poisson {dims}")
    assert seen[0]["used"] == 0 and seen[0]["kept"] == 1 and seen[1]["used"] == 1
    if itmax == 2000:                               # (a solve cut short leaves less than the whole direction)
        assert seen[1]["res_after"] <= 10 * tol     # the second right-hand side is a multiple of the first


def test_bands_and_tail_equals_twin(E, oracle):
    valA, irow, jcol = G.case("long_row")[:3]
    n = len(irow) - 1
    rng = np.random.default_rng(21)
    rhs = [rng.standard_normal(n) for _ in range(3)]
    rhs += [rhs[0] + rhs[2], rhs[1]]
    tol, itmax, cap = 1e-8, 5000, 64
    with E.EC3DSolver() as s:
        s.set_matrix_csr(valA, irow, jcol)
        assert s.info.tail_rows > 0
        s.set_guess_history(2)
        twin = GH.for_handle(oracle, s, valA, irow, jcol, 2, tol, itmax, cap)
        seen = check_sequence(s, twin, rhs, np.zeros(n), tol, itmax, cap, "long_row")
    assert [i["stored"] for i in seen[:2]] == [1, 2] and seen[2]["kept"] == 1      # the third solve evicts the first pair


@pytest.mark.parametrize("case, pitch, structured", [("g2", None, True), ("g2", "2", True), ("g2", None, False),
                                                     ("g8a", None, True)],
                         ids=["g2-auto", "g2-pitched", "g2-bands-tail", "g8a"])
def test_av_system_equals_twin(E, oracle, monkeypatch, case, pitch, structured):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    if pitch:
        monkeypatch.setenv("EC3D_PITCH", pitch)
    g = load_golden(AV[case])
    tol, itmax, cap = float(g["tol"]), int(g["itmax"]), 64
    rhs = [g["b0"], g["b1"], g["b2"], g["b0"] + g["b2"], g["b1"]]
    with E.EC3DSolver(structured=structured) as s:
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        lay = s.vector_layout()
        assert (lay["n"] != s.info.n) == structured          # the structured form embeds U in the grid
        s.set_guess_history(2)
        twin = GH.for_handle(oracle, s, g["valA"], g["irow"], g["jcol"], 2, tol, itmax, cap)
        seen = check_sequence(s, twin, rhs, np.array(g["xin0"]), tol, itmax, cap, f"{case} pitch {pitch} structured {structured}")
    assert [i["used"] for i in seen] == [0, 1, 2, 2, 2]


def test_preconditioned_solve_equals_twin(E, oracle):
    N = 16
    valA, irow, jcol = oracle.poisson_csr(N, N, N)
    b0 = oracle.bar_rhs(N)
    tol, itmax, cap = 1e-5, 100, 24
    mg = M.MG(N, N, N)
    with E.EC3DSolver() as s:
        s.assemble_poisson(N, N, N)
        s.set_guess_history(2)
        s.set_preconditioner("mg")
        assert s.guess_history()["depth"] == 2

        def solve(b, x0):
            return M.pbicgstab_gpuorder(mg, b, x0, tol, itmax, oracle.geoms_of(s)[1], hist_cap=cap)
        twin = GH.for_handle(oracle, s, valA, irow, jcol, 2, tol, itmax, cap, solve=solve)
        check_sequence(s, twin, [a * b0 for a in SCALES], np.zeros(N ** 3), tol, itmax, cap, "mg 16^3")


# ---- right-hand sides from a plane --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(16, 16, 16), (17, 9, 5)], ids=lambda d: "x".join(map(str, d)))
def test_right_hand_sides_from_a_plane(E, dims):
    tol, itmax = 1e-10, 5000
    n = int(np.prod(dims))
    with E.EC3DSolver() as s, E.EC3DSolver() as plain:
        s.assemble_poisson(*dims)
        plain.assemble_poisson(*dims)
        s.set_guess_history(2)
        x, xp = np.zeros(n), np.zeros(n)
        for t, b in enumerate(family_rhs(n), start=1):
            x, it, _ = s.solve(b, x, tol, itmax)
            xp, itp, _ = plain.solve(b, xp, tol, itmax)
            info = s.guess_history()
            print(f"{dims} step {t}: {it} iterations with the history, {itp} without; res_after / tol = "
                  f"{info['res_after'] / tol:.3g}, kept {info['kept']}")
            assert it <= itmax and itp <= itmax
            if t >= 3:
                assert info["res_after"] <= 100 * tol, t
                assert info["kept"] == 0 and info["stored"] == 2, t
                assert 5 * it <= itp, (t, it, itp)


# ---- the contract ------------------------------------------------------------------------------------------------------
def poisson_system(dims=(17, 9, 5)):
    n = int(np.prod(dims))
    rng = np.random.default_rng(77 + n)
    return dims, n, [rng.standard_normal(n) for _ in range(3)], rng.standard_normal(n)


def solves(s, rhs, x0, tol=1e-10, itmax=5000):
    out, x = [], x0
    for b in rhs:
        x, it, hist = s.solve(b, x, tol, itmax, hist_cap=32)
        out.append((x.tobytes(), it, hist.tobytes()))
    return out


def test_depth_zero_is_a_fresh_handle(E):
    dims, n, rhs, x0 = poisson_system()
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        nbytes = s.info.device_bytes
        want = solves(s, rhs, x0)
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_guess_history(0)
        assert solves(s, rhs, x0) == want and s.info.device_bytes == nbytes
        assert s.guess_history()["depth"] == 0 and s.guess_history()["stored"] == 0
        s.set_guess_history(3)
        assert solves(s, rhs, x0) != want and s.guess_history()["stored"] > 0      # (the history does change a solve)
        s.set_guess_history(0)                                                     # ... and is taken back
        assert solves(s, rhs, x0) == want and s.info.device_bytes == nbytes
        for bad in (-1, 9):
            with pytest.raises(E.EC3DError) as e:
                s.set_guess_history(bad)
            assert e.value.status == 2 and s.guess_history()["depth"] == 0


def test_zero_right_hand_side_leaves_everything_alone(E):
    dims, n, rhs, x0 = poisson_system()
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_guess_history(2)
        x = x0
        for b in rhs[:2]:
            x, _, _ = s.solve(b, x, 1e-8, 5000)
        before = s.guess_history()
        assert before["stored"] == 2
        x[5] = -0.0                                     # a bit pattern X + 0 * Q would not keep
        y, it, _ = s.solve(np.zeros(n), x, 1e-8, 5000)
        after = s.guess_history()
        assert it == 0 and y.tobytes() == x.tobytes()
        assert after["stored"] == 2 and after["kept"] == 0 and after["used"] == 2 and not after["coef"].any()
        # the pairs are the same pairs: the next solve is what it is on a handle that never saw the zero
        z, itz, _ = s.solve(rhs[2], x, 1e-8, 5000)
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_guess_history(2)
        x2 = x0
        for b in rhs[:2]:
            x2, _, _ = s.solve(b, x2, 1e-8, 5000)
        x2[5] = -0.0
        w, itw, _ = s.solve(rhs[2], x2, 1e-8, 5000)
    assert itz == itw and z.tobytes() == w.tobytes()


@pytest.mark.parametrize("bad", ["nan", "overflow"])
def test_a_nan_solve_clears_the_history(E, bad):
    dims, n, rhs, x0 = poisson_system()
    bb = np.array(rhs[0])
    if bad == "nan":
        bb[n // 3] = np.nan
    else:
        bb[:] = 0.0
        bb[n // 3] = 1e308
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_guess_history(2)
        want = solves(s, rhs, x0)
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_guess_history(2)
        z = Z.zones(s.vector_layout())
        solves(s, rhs[:2], x0)
        assert s.guess_history()["stored"] == 2
        x, _, _ = s.solve(bb, np.zeros(n), 1e-6, 7)
        assert not np.isfinite(x).all()
        info = s.guess_history()
        assert info["kept"] == -1 and info["stored"] == 0, info
        assert solves(s, rhs, x0) == want
        Z.assert_clean(s, z, f"after a {bad} solve and three clean ones")


def test_a_new_matrix_and_a_new_depth_clear_the_history(E):
    dims, n, rhs, x0 = poisson_system()
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        s.set_guess_history(2)
        want = solves(s, rhs, x0)
        assert s.guess_history()["stored"] == 2
        s.assemble_poisson(*dims)
        assert s.guess_history() ["stored"] == 0 and s.guess_history()["depth"] == 2    # the depth outlives the matrix
        assert solves(s, rhs, x0) == want
        s.set_guess_history(3)
        assert s.guess_history()["stored"] == 0
        got = solves(s, rhs, x0)
        assert got[:2] == want[:2] and s.guess_history()["stored"] == 3
        s.set_preconditioner("none")                      # ... and this does not
        assert s.guess_history()["stored"] == 3


@pytest.mark.parametrize("case", ["poisson-17x9x5", "g2-pitched"])
def test_adopted_vectors_between_canaries(E, monkeypatch, case):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    if case == "g2-pitched":
        monkeypatch.setenv("EC3D_PITCH", "2")
        g = load_golden(AV["g2"])
        plane = g["geoPHYS"].shape[1] * g["geoPHYS"].shape[2]

        def build(s):
            s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        rhs, x0, tol, itmax = [g["b0"], g["b1"], g["b2"]], np.array(g["xin0"]), float(g["tol"]), int(g["itmax"])
    else:
        dims, n, rhs, x0 = poisson_system()
        plane, tol, itmax = None, 1e-10, 5000

        def build(s):
            s.assemble_poisson(*dims)
    with E.EC3DSolver() as s:
        build(s)
        s.set_guess_history(2)
        want = solves(s, rhs, x0, tol, itmax)
    with Z.adopted(E, build) as a:
        a.s.set_guess_history(2)
        z = Z.zones(a.s.vector_layout(), Z.pitch_info(a.s, plane) if plane else None)
        x = x0
        for t, b in enumerate(rhs):
            x, it, hist = a.s.solve(b, x, tol, itmax, hist_cap=32)
            Z.assert_clean(a, z, f"{case}: after solve {t}")
            assert (x.tobytes(), it, hist.tobytes()) == want[t], (case, t)
        assert a.s.guess_history()["stored"] == 2


def test_slabs_refuse_and_solve_as_before(E):
    dims = (24, 24, 24)
    n = int(np.prod(dims))
    rng = np.random.default_rng(3)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims, slab=(8, 16))
        with pytest.raises(E.EC3DError) as e:
            s.set_guess_history(2)
        assert e.value.status == 4 and s.guess_history()["depth"] == 0
    with E.EC3DMulti(2, devices=[0, 0]) as m:
        m.assemble_poisson(*dims)
        want = m.solve(b, x0, 1e-8, 5000)
        for r in range(2):
            with pytest.raises(E.EC3DError) as e:
                m.slab(r)[0].set_guess_history(2)
            assert e.value.status == 4 and m.slab(r)[0].guess_history()["depth"] == 0
        got = m.solve(b, x0, 1e-8, 5000)
        assert got[1] == want[1] and np.array_equal(got[0], want[0])


def dropin_child(path):
    """What the child process of the test below runs: the F77 symbol, x carried from call to call."""
    import eddy_currents_3d_amd as E
    d = np.load(path)
    valA, irow, jcol = d["valA"], d["irow"], d["jcol"]
    x = np.zeros(len(irow) - 1)
    out = []
    for b in d["rhs"]:
        it = E.sprsBCGstabWR(valA, irow, jcol, len(irow) - 1, b, x, float(d["tol"]), int(d["itmax"]))
        out.append([it, hashlib.sha256(x.tobytes()).hexdigest()])
    print("RESULT " + json.dumps(out))


def test_drop_in_symbol_reads_the_depth_from_the_environment(E, oracle, tmp_path):
    dims, tol, itmax = (12, 10, 9), 1e-10, 5000
    valA, irow, jcol = oracle.poisson_csr(*dims)
    n = len(irow) - 1
    rhs = family_rhs(n)[:4]
    path = str(tmp_path / "system.npz")
    np.savez(path, valA=valA, irow=irow, jcol=jcol, rhs=np.array(rhs), tol=tol, itmax=itmax)
    want = {}
    for depth in (0, 2):
        with E.EC3DSolver() as s:
            s.set_matrix_csr(valA, irow, jcol)
            s.set_guess_history(depth)
            x, want[depth] = np.zeros(n), []
            for b in rhs:
                s.upload("B", b)
                s.upload("X", x)
                it, _ = s.solve_resident(tol, itmax)
                x = s.download("X")
                want[depth].append([it, hashlib.sha256(x.tobytes()).hexdigest()])
    assert want[0] != want[2] and 5 * want[2][3][0] <= want[0][3][0]
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, EC3D_GUESS_HISTORY="2", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env.pop("EC3D_NGPU", None)
    r = subprocess.run([sys.executable, "-c", f"import test_gpu_guess_history as T; T.dropin_child({path!r})"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("iterations through the symbol:", [g[0] for g in got], "on a handle without a history:", [w[0] for w in want[0]])
    assert got == want[2]


# ---- the time loop ------------------------------------------------------------------------------------------------------
def test_time_loop_with_a_history(E):
    from eddy_currents_3d_amd import host, vxc
    g = load_golden("g4_LIM")
    model = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                         tuple(float(x) for x in g["adj"]))
    tol = float(g["tol"])
    totals = {}
    for depth in (4, 0):
        res = []
        with E.EC3DSolver() as s:
            log = host.run(model, s, steps=30, guess_history=depth,
                           on_solved=lambda k, s, info: res.append(s.true_residual()[0]))
        assert len(log) == 30 and len(res) == 30
        assert ("guess" in log[0]) == (depth > 0)
        if depth:
            assert log[-1]["guess"]["depth"] == 4 and log[-1]["guess"]["used"] == 4
        assert max(res) < tol, (depth, max(res))
        totals[depth] = sum(i["iter"] for i in log)
        print(f"g4_LIM, 30 steps, depth {depth}: {totals[depth]} iterations ({[i['iter'] for i in log]}), "
              f"largest true residual {max(res):.3e} (tol {tol:g})")
