"""The left null vectors of the time-harmonic operator on the device (ec3d_harmonic_set_null_projection, k_hb_spmv_h and
the k_hbn_* kernels of csrc/ec3d_harmonic.hip) against the twin (tests/harmonic_null_numpy.py).
Every test here fails on a library without the entry points.

* harmonic_spmv_h == the twin's OperatorH BIT FOR BIT on g2, g2v, g8a, g9b, g3 with padded planes and the 96 x 96 x 64 box
  of tests/test_gpu_harmonic.py (4 608 chunks: the chunk loops make several trips), for random complex x and for a
  resident x^ with NaN in every row of no unknown;
* the set-up on g2, g8a, g9b: iterations, restarts and every kept vector equal left_null_vectors bit for bit, the
  report's residual to 1e-12 relative; X^ and B^ keep their bytes;
* the projection: R, R0, P behind harmonic_solve(tol, -1) == project_device of the device's own Q and of the same call's
  R with the projection off, bit for bit, on g2, g2 with padded planes and the box; ||R|| as k_hb_setup took it from the
  partials the subtraction left;
* whole solves: itmax = 1, 5, 20 on g2 and g8a equal bicgstab_projected bit for bit; tol 1e-6 on five fixtures and 1e-8
  on g3, g8a, g9b converge within 2000 iterations to a projected residual <= 10 tol that equals the twin's, where the
  same handle with the projection off runs into itmax at 1e-6.  (g2 and g2v at 1e-8 are left out: there the twin stalls
  near 1.2e-8 .. 4e-8, the accuracy of w at null_tol 1e-10; tests/test_harmonic_null_host.py.)
* the contract: on and off again gives a fresh handle's bits; the real vectors and rings keep their bytes; another omega
  or a new assembly clears Q, the same omega keeps it, the setting stays;
* a null_tol no solve reaches (1e-30: the recurrence's residual gets there after 1 129 iterations on g2, the true one
  stops at 1.5e-8 ||w||): EC3D_NULL_E_SETUP naming component and seed row, x^ untouched; refusals; host.run_harmonic."""
import numpy as np
import pytest

import device_sums_numpy as DS
import guard_zones as Z
import harmonic_null_numpy as HH
import harmonic_numpy as HN
import null_projection_numpy as NP
from conftest import load_golden
from eddy_currents_3d_amd.solver import NULL_E_MATRIX, NULL_E_SETUP
from test_gpu_harmonic import (G2, G2V, G3, G8A, G9B, OMEGA, SPMV_CASES, _assemble, _bits, _poison_rows_of_no_unknown,
                               _random_complex, _same, _sums, box)

pytestmark = pytest.mark.gpu
# the box's adjoint solve: at this null_tol it takes BOX_ADJOINT_ITERATIONS iterations on the device (found there:
# 1e-4 44, 1e-5 113, 1e-6 309, 1e-7 641, 1e-8 802 iterations)
BOX_NULL_TOL = 1e-6
BOX_ADJOINT_ITERATIONS = 309


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


_TWIN = {}


def twin(name, s):
    """dict(g, op, opH, sums, Q, info, b) of a fixture at 50 Hz, once per process (the handle gives the sums' layout,
    which is the same on every handle without padded planes)."""
    if name not in _TWIN:
        g = load_golden(name)
        op = HN.Operator(g, OMEGA)
        opH = HH.OperatorH(op)
        sums = _sums(s)
        Q, info = HH.left_null_vectors(op, opH, sums, NP.seed_rows(g["geoPHYS_C"]))
        _TWIN[name] = dict(g=g, op=op, opH=opH, sums=sums, Q=Q, info=info, b=g["b0"].astype(np.complex128))
    return _TWIN[name]


@pytest.mark.parametrize("name,pitched", SPMV_CASES, ids=[f"{n.split('_')[0]}{'-pitched' if p else ''}" for n, p in SPMV_CASES])
def test_spmv_h_equals_the_twin_bit_for_bit(E, monkeypatch, name, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    g = load_golden(name)
    op = HN.Operator(g, OMEGA)
    opH = HH.OperatorH(op)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        for seed in (1, 2):
            x = _random_complex(op.n, seed)
            _same(s.harmonic_spmv_h(x), opH(HN.split(x)), f"{name} seed {seed}")
        x = _random_complex(op.n, 3)
        assert _poison_rows_of_no_unknown(s, x) > 0
        y = s.harmonic_spmv_h(None)
        assert np.all(np.isfinite(y.real)) and np.all(np.isfinite(y.imag))
        _same(y, opH(HN.split(x)), f"{name} NaN in the rows of no unknown")
        _same(s.harmonic_download("X"), x, "X^ as uploaded")
        # <y, A x> = <A^H y, x> on the device's own two products
        y = _random_complex(op.n, 4)
        lhs, rhs = np.vdot(y, s.harmonic_spmv(x)), np.vdot(s.harmonic_spmv_h(y), x)
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_spmv_h_on_a_box_of_more_than_1024_chunks(E):
    g, op = box()
    opH = HH.OperatorH(op)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        assert s.vector_layout()["n_pad"] // 512 > 1024
        x = _random_complex(op.n, 5)
        _same(s.harmonic_spmv_h(x), opH(HN.split(x)), "box")
        _poison_rows_of_no_unknown(s, x)
        y = s.harmonic_spmv_h(None)
        assert np.all(np.isfinite(y.real)) and np.all(np.isfinite(y.imag))
        _same(y, opH(HN.split(x)), "box, NaN in the rows of no unknown")


@pytest.mark.parametrize("name", [G2, G8A, G9B])
def test_the_set_up_equals_the_twin_bit_for_bit(E, name):
    with E.EC3DSolver() as s:
        _assemble(s, load_golden(name))
        t = twin(name, s)
        x = _random_complex(t["op"].n, 9)
        s.harmonic_upload("X", x)
        s.harmonic_upload("B", t["b"])
        s.harmonic_set_null_projection(True)
        assert not s.harmonic_null_projection()["built"]
        bytes0 = s.harmonic_info()["device_bytes"]
        W = [s.harmonic_left_null_vector(0)]
        info = s.harmonic_null_projection()
        W += [s.harmonic_left_null_vector(i) for i in range(1, info["kept"])]
        _same(s.harmonic_download("X"), x, "X^ across the set-up")
        _same(s.harmonic_download("B"), t["b"], "B^ across the set-up")
        n_pad = s.vector_layout()["n_pad"]
        assert s.harmonic_info()["device_bytes"] - bytes0 >= info["kept"] * n_pad * 16
    print(f"{name}: device {[(c['iterations'], c['restarts'], c['residual']) for c in info['components']]}, "
          f"twin {[(c['iterations'], c['restarts'], c['residual']) for c in t['info']]}, set-up {info['setup_ms']:.0f} ms")
    assert info["built"] and info["on"] and info["found"] == len(t["info"]) and info["dropped"] == 0
    assert info["kept"] == len(t["Q"]) == (2 if name == G8A else 1)
    for c, w in zip(info["components"], t["info"]):
        assert (c["seed_row"], c["iterations"], c["restarts"], c["kept"]) == (w["seed"], w["iterations"], w["restarts"], w["kept"])
        assert c["iterations"] <= HH.adjoint_cap(t["op"].n)
        assert abs(c["residual"] - w["residual"]) <= 1e-12 * w["residual"]
    for i, (got, want) in enumerate(zip(W, t["Q"])):
        _same(got, want, f"{name} kept vector {i}")


def _box_rhs(op, g):
    rng = np.random.default_rng(11)
    b = np.zeros(op.n, np.complex128)
    coil = np.flatnonzero(np.asarray(g["geoPHYS_C"]).reshape(-1) == 0)[::97][:4000]
    b[coil] = rng.standard_normal(len(coil)) + 1j * rng.standard_normal(len(coil))
    b[op.nC + coil] = rng.standard_normal(len(coil))
    return b


@pytest.mark.parametrize("case", ["g2", "g2-pitched", "box"])
def test_the_projection_equals_the_twin_bit_for_bit(E, monkeypatch, case):
    if case == "g2-pitched":
        monkeypatch.setenv("EC3D_PITCH", "2")
    if case == "box":
        g, op = box()
        b, null_tol = _box_rhs(op, g), BOX_NULL_TOL
    else:
        g = load_golden(G2)
        op = HN.Operator(g, OMEGA)
        b, null_tol = g["b0"] + 1j * g["b1"], 1e-10
    x = 1e-3 * _random_complex(op.n, 7)
    tol = 1e-6

    def behind_begin(s):
        s.harmonic_upload("X", x)
        it, relres = s.harmonic_solve(tol, -1)
        assert it == 0
        s.synchronize()
        out = []
        for w in ("R", "R0", "P"):
            ptr, n_pad = s.harmonic_device_vector(w)
            out.append(Z.peek(ptr, 2 * n_pad).view(np.float64).reshape(n_pad, 2).copy().view(np.complex128).reshape(-1))
        return out, relres

    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.harmonic_upload("B", b)
        plain, _ = behind_begin(s)
        s.harmonic_set_null_projection(True, null_tol)
        got, relres = behind_begin(s)
        info = s.harmonic_null_projection()
        _, bnorm = s.harmonic_true_residual()
        W = [s.harmonic_left_null_vector(i) for i in range(info["kept"])]
        lay, rm = s.vector_layout(), s.row_map().astype(np.int64)
    n, n_pad = int(lay["n"]), int(lay["n_pad"])
    print(f"{case}: null_tol {null_tol:g}, adjoint iterations {[c['iterations'] for c in info['components']]}, "
          f"set-up {info['setup_ms']:.0f} ms, removed {info['removed']:.6e}")
    assert info["kept"] == 1 and (n_pad // 512 > 1024) == (case == "box")
    if case == "box":
        assert info["components"][0]["iterations"] == BOX_ADJOINT_ITERATIONS
    Qd = []
    for w in W:
        d = np.zeros(n_pad, np.complex128)
        d[rm] = w
        Qd.append(d)
    want, c, rr = HH.project_device(Qd, plain[0], n)
    for nm, v in zip(("R", "R0", "P"), got):
        assert np.array_equal(_bits(v[rm]), _bits(want[rm])), f"{nm}: {np.count_nonzero(v[rm] != want[rm])} rows differ"
    assert not np.array_equal(_bits(want[rm]), _bits(plain[0][rm]))        # (it did something)
    assert relres == np.sqrt(DS.strided(rr)) / bnorm                     # the HP_RR partials, as k_hb_setup read them
    wb = float(np.sqrt(np.sum(np.abs(c) ** 2)) / bnorm)
    assert abs(info["removed"] - wb) <= 1e-6 * wb


@pytest.mark.parametrize("name", [G2, G8A])
def test_whole_projected_iterations_equal_the_twin_bit_for_bit(E, name):
    with E.EC3DSolver() as s:
        _assemble(s, load_golden(name))
        t = twin(name, s)
        op, n = t["op"], t["op"].n
        b, x0 = t["g"]["b0"] + 1j * t["g"]["b1"], 1e-3 * _random_complex(n, 7)
        trace = []
        HH.bicgstab_projected(op, t["sums"], t["Q"], HN.split(b), HN.split(x0), 0.0, 20, trace=trace)
        s.harmonic_set_null_projection(True)
        s.harmonic_upload("B", b)
        for k in (1, 5, 20):
            s.harmonic_upload("X", x0)
            it, _ = s.harmonic_solve(0.0, k)
            info = s.harmonic_info()
            assert it == k + 1 == info["iter"]
            _same(s.harmonic_download("X"), trace[k][1], f"{name} itmax = {k}")
            assert info["restarts"] == trace[k][2]


CONVERGENCE = [(G2, 1e-6), (G2V, 1e-6), (G3, 1e-6), (G8A, 1e-6), (G9B, 1e-6), (G3, 1e-8), (G8A, 1e-8), (G9B, 1e-8)]


@pytest.mark.parametrize("name,tol", CONVERGENCE, ids=[f"{n.split('_')[0]}-{t:g}" for n, t in CONVERGENCE])
def test_convergence_below_the_floor(E, name, tol):
    g = load_golden(name)
    op = HN.Operator(g, OMEGA)
    b, zero = g["b0"].astype(np.complex128), np.zeros(op.n)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        s.harmonic_upload("B", b)
        if tol == 1e-6:
            s.harmonic_upload("X", zero)
            it_off, _ = s.harmonic_solve(tol, 2000)
            floor, _ = s.harmonic_true_residual()
            assert it_off == 2001, "the plain solve is expected to stall above 1e-6"
        s.harmonic_set_null_projection(True)
        s.harmonic_upload("X", zero)
        it, relres = s.harmonic_solve(tol, 2000)
        pres, removed = s.harmonic_projected_residual()
        true, _ = s.harmonic_true_residual()
        x = s.harmonic_download("X")
        info = s.harmonic_null_projection()
        Q = [HN.split(s.harmonic_left_null_vector(i)) for i in range(info["kept"])]
    twin_pres, twin_removed = HH.projected_residual(op, sums, Q, HN.split(b), HN.split(x))
    print(f"{name} tol {tol:g}: iter {it}, relres {relres:.3e}, projected residual {pres:.3e} (twin {twin_pres:.3e}), "
          f"true residual {true:.3e}, removed {removed:.3e}, adjoint {[c['iterations'] for c in info['components']]}")
    assert it <= 2000 and relres < tol
    assert abs(pres - twin_pres) <= 1e-12 and abs(removed - twin_removed) <= 1e-6 * twin_removed
    assert pres <= 10 * tol


def test_off_again_is_a_fresh_handle_and_q_follows_matrix_and_omega(E):
    g = load_golden(G2)
    tol, itmax = float(g["tol"]), int(g["itmax"])
    b = g["b0"] + 1j * g["b1"]

    def solve(s):
        s.harmonic_upload("B", b)
        s.harmonic_upload("X", np.zeros(s.n))
        it, relres = s.harmonic_solve(tol, itmax)
        return it, relres, s.harmonic_download("X"), s.harmonic_info()["restarts"]

    with E.EC3DSolver() as s:
        _assemble(s, g)
        fresh = solve(s)
        assert s.harmonic_null_projection() == dict(on=False, built=False, found=0, kept=0, dropped=0, null_tol=1e-10,
                                                    removed=0.0, setup_ms=0.0, components=[])
    with E.EC3DSolver() as s:
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        s.upload("B", g["b1"])
        s.upload("X", g["xin1"])
        s.solve_resident(tol, itmax)
        s.harmonic_setup(OMEGA)
        base, before = Z.owned_block(s)
        rings_before = Z.rings(s)
        s.harmonic_set_null_projection(True)
        on = solve(s)
        base2, after = Z.owned_block(s)
        assert base2 == base and np.array_equal(before, after), "a real vector changed under the set-up or the projected solve"
        for k, v in Z.rings(s).items():
            assert np.array_equal(v, rings_before[k]), k
        info = s.harmonic_null_projection()
        assert info["built"] and info["kept"] == 1 and info["removed"] > 0.0
        s.harmonic_set_null_projection(False)
        off = solve(s)
        assert off[:2] == fresh[:2] and off[3] == fresh[3]
        _same(off[2], fresh[2], "off again")
        assert not np.array_equal(_bits(on[2]), _bits(fresh[2]))
        assert s.harmonic_null_projection()["built"] and not s.harmonic_null_projection()["on"]     # Q stays
        s.harmonic_set_null_projection(True)
        s.harmonic_setup(OMEGA)
        assert s.harmonic_null_projection()["built"], "the same omega keeps Q"
        s.harmonic_setup(2.0 * OMEGA)
        q = s.harmonic_null_projection()
        assert not q["built"] and q["on"], "another omega clears Q, the setting stays"
        w2 = s.harmonic_left_null_vector(0)
        assert s.harmonic_null_projection()["built"]
        aw = s.harmonic_spmv_h(w2)
        assert np.linalg.norm(aw) <= 1e-2 and abs(np.linalg.norm(w2) - 1.0) <= 1e-12
        s.harmonic_set_null_projection(True, 1e-9)
        assert not s.harmonic_null_projection()["built"], "another null_tol makes the vectors again"
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        q = s.harmonic_null_projection()
        assert not q["built"] and q["on"] and q["null_tol"] == 1e-9, "a new assembly clears Q and keeps the setting"
        s.harmonic_setup(OMEGA)
        s.harmonic_set_null_projection(True, 1e-10)
        again = solve(s)
        assert again[:2] == on[:2]
        _same(again[2], on[2], "the rebuilt Q")


def test_a_vector_that_missed_null_tol_is_never_used(E):
    g = load_golden(G2)
    x = _random_complex(len(g["b0"]), 3)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.harmonic_upload("B", g["b0"])
        s.harmonic_upload("X", x)
        s.harmonic_set_null_projection(True, 1e-30)
        with pytest.raises(E.EC3DError, match=r"component 0 \(seed row 10242\)") as e:
            s.harmonic_solve(1e-6, 100)
        assert e.value.status == NULL_E_SETUP
        _same(s.harmonic_download("X"), x, "x^ after the refused solve")
        q = s.harmonic_null_projection()
        assert not q["built"] and q["on"] and q["kept"] == 0
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_left_null_vector(0)
        assert e.value.status == NULL_E_SETUP
        s.harmonic_set_null_projection(False)
        assert s.harmonic_solve(1e-3, 100)[0] <= 100


def test_refusals(E):
    g = load_golden(G2)

    def off(s):
        return not s.harmonic_null_projection()["on"]

    with E.EC3DSolver() as s:
        calls = (lambda: s.harmonic_set_null_projection(True), lambda: s.harmonic_left_null_vector(0),
                 lambda: s.harmonic_spmv_h(None), lambda: s.harmonic_projected_residual())
        for call in calls:                                                   # no matrix
            with pytest.raises(E.EC3DError) as e:
                call()
            assert e.value.status == 3 and off(s)
        s.assemble_poisson(8, 8, 8)
        for call in calls:
            with pytest.raises(E.EC3DError) as e:
                call()
            assert e.value.status == 3 and off(s)
        s.set_matrix_csr(g["valA"], g["irow"], g["jcol"])
        for call in calls:
            with pytest.raises(E.EC3DError) as e:
                call()
            assert e.value.status == 3 and off(s)
        c = load_golden("g8c_side_by_side_20x18x14")                          # bands + tail
        s.assemble(c["geoPHYS"], c["geoPHYS_C"], c["valPHYS"], c["BND"], c["delta"], float(c["dt"]))
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_set_null_projection(True)
        assert e.value.status == NULL_E_MATRIX and off(s)
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        for call in calls:                                                   # before harmonic_setup
            with pytest.raises(E.EC3DError, match="ec3d_harmonic_setup first") as e:
                call()
            assert e.value.status == 2 and off(s)
        s.harmonic_setup(OMEGA)
        with pytest.raises(E.EC3DError) as e:                                # the setting is off: no vectors, no residual
            s.harmonic_left_null_vector(0)
        assert e.value.status == 2
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_projected_residual()
        assert e.value.status == 2 and off(s)
        s.harmonic_set_null_projection(True)
        for bad in (-1, 1, 7):
            with pytest.raises(E.EC3DError) as e:
                s.harmonic_left_null_vector(bad)
            assert e.value.status == 2
        assert s.harmonic_null_projection()["on"] and s.harmonic_null_projection()["kept"] == 1
        assert s.L.ec3d_get_harmonic_null(s.h, None) == 2 and s.L.ec3d_harmonic_set_null_projection(None, 1, 0.0) == 2
        s.harmonic_set_null_projection(True, 0.0)                            # <= 0: the default
        assert s.harmonic_null_projection()["null_tol"] == 1e-10 and s.harmonic_null_projection()["built"]
    b = load_golden("g8b_stacked_moving_20x16x14")                            # a z-slab: planes [0, 9), owned [0, 7)
    geo = b["geoPHYS"][:9].copy()
    geoC = np.zeros(geo.shape, np.int32)
    q = np.concatenate([np.flatnonzero((geo.reshape(-1) == d) & (b["geoPHYS_C"][:9].reshape(-1) != 0)) for d in (1, 2)])
    geoC.reshape(-1)[q] = 3 * geo.size + 1 + np.arange(len(q))
    with E.EC3DSolver() as s:
        s.assemble_slab(b["geoPHYS"].shape[0], 0, 9, 0, 7, geo, geoC, b["valPHYS"], b["BND"], b["delta"], float(b["dt"]))
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_set_null_projection(True)
        assert e.value.status == 5 and off(s)


def test_run_harmonic_with_the_projection(E, capsys, tmp_path):
    """host.run_harmonic on two generated 4 x 4 x 4 blocks under a coil loop: tol 1e-6 is reached in the projected
    residual while the true residual shows the floor; the setting is left off; the command line reports it."""
    from eddy_currents_3d_amd import host, run, vxc
    from multidomain_numpy import blocks_model
    vox, names = blocks_model(2)
    model = vxc.VxcModel(vox, names, 0.004, (1.0, 1.0, 1.0))
    tol = 1e-6
    with E.EC3DSolver() as s:
        plain = host.run_harmonic(model, s, 50.0, tol=tol, itmax=2000)
        r = host.run_harmonic(model, s, 50.0, tol=tol, itmax=2000, null_projection=True)
        assert not s.harmonic_null_projection()["on"]
    print(f"two blocks at 50 Hz, tol {tol:g}: plain iter {plain['iter']} (true {plain['true_residual']:.3e}); projected iter "
          f"{r['iter']}, projected residual {r['projected_residual']:.3e}, true {r['true_residual']:.3e}, removed "
          f"{r['removed']:.3e}, adjoint {[c['iterations'] for c in r['null']['components']]}")
    assert "projected_residual" not in plain and plain["iter"] == 2001
    assert r["iter"] <= 2000 and r["relres"] < tol and r["projected_residual"] <= 10 * tol
    assert r["null"]["kept"] == 2 and r["null"]["built"]
    assert r["true_residual"] > 10 * tol and abs(r["true_residual"] - r["removed"]) <= 0.05 * r["removed"]
    path = str(tmp_path / "blocks.vxc")
    vxc.write_vxc(path, model)
    capsys.readouterr()
    assert run.main([path, "--harmonic", "50", "--tol", "1e-6", "--null-projection", "--no-output"]) == 0
    out = capsys.readouterr().out
    adjoint = "+".join(str(c["iterations"]) for c in r["null"]["components"])
    assert f"iter={r['iter']} " in out and f"projected residual={r['projected_residual']:.3e} adjoint iterations={adjoint} " in out
    import os
    from conftest import GOLDEN
    with pytest.raises(SystemExit):
        run.main([os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc"), "--harmonic", "50", "--null-projection", "--null-precond",
                  "block-mg", "--no-output"])
    assert "no preconditioner" in capsys.readouterr().err
