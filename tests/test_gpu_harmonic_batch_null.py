"""The left null vectors inside a batch of harmonic systems (ec3d_harmonic_batch_set_null_projection, k_hb_spmv_h, k_hb_xr_at
and the k_hbn_* kernels of csrc/ec3d_harmonic.hip).  Every system s of a batch gets the Q_s of its
own omega_s, found by adjoint solves that run in lock step, and is solved as the single projected solve solves it: the
twin of a system is tests/harmonic_null_numpy.py's left_null_vectors and bicgstab_projected at omega_s with the device's
row map, and a second reference is harmonic_setup + harmonic_set_null_projection + harmonic_solve on the same handle.
Every test here fails on a library without the entry points.

* the set-up on g2 at 5, 50, 500, 2000 Hz and g8a at 5, 50, 2000 Hz: iterations, restarts, kept and every kept vector
  equal the twin's and the single set-up's bit for bit, the systems stop in different polls, X^ and B^ keep their bytes;
* the projection: R, R0, P behind harmonic_batch_solve(tol, -1) == project_device of the system's own Q and of the same
  call's R with the setting off, bit for bit, on g2 and on g3 with padded planes;
* whole solves: itmax = 1, 5, 20 and tol 1e-6 on g2 and g8a, per system, against the twin and the single projected solve;
* systems with bit-equal omega share one set of vectors; no cross-talk from a zero and a NaN right-hand side;
* a batch of one system == the single set-up and the single projected solve, bit for bit, and three systems of one omega
  (one set for S = 3): device_bytes by the formula, so the single projection has no staging vector and the batch has one;
* a null_tol no solve reaches; the contract (off again is a fresh handle; what clears the vectors; the real vectors, the
  rings and the single solve's own Q and setting are untouched); refusals; host.run_harmonic_sweep and the command line."""
import ctypes as C

import numpy as np
import pytest

import device_sums_numpy as DS
import guard_zones as Z
import harmonic_null_numpy as HH
import harmonic_numpy as HN
import null_projection_numpy as NP
from conftest import load_golden
from eddy_currents_3d_amd.solver import NULL_E_MATRIX, NULL_E_SETUP, NullInfo
from test_gpu_harmonic_batch import G2, G3, G8A, _assemble, _bits, _random_complex, _report, _rhs, _same, _sums, _w

pytestmark = pytest.mark.gpu
FREQS = {G2: (5.0, 50.0, 500.0, 2000.0), G8A: (5.0, 50.0, 2000.0)}
NULL_TOL = 1e-10


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


_TWIN, _GOLDEN = {}, {}


def golden(name):
    if name not in _GOLDEN:
        _GOLDEN[name] = load_golden(name)
    return _GOLDEN[name]


def twin(name, f, sums):
    """dict(op, Q, info) of a fixture at f Hz, once per process: left_null_vectors at NULL_TOL with the device's row map
    (the same on every handle without padded planes)."""
    if (name, f) not in _TWIN:
        g = golden(name)
        op = HN.Operator(g, _w(f))
        Q, info = HH.left_null_vectors(op, HH.OperatorH(op), sums, NP.seed_rows(g["geoPHYS_C"]), NULL_TOL)
        _TWIN[(name, f)] = dict(op=op, Q=Q, info=info)
    return _TWIN[(name, f)]


def _batch(s, omegas, bs, xs):
    s.harmonic_batch_setup(omegas)
    for k in range(len(omegas)):
        s.harmonic_batch_upload(k, "B", bs[k])
        s.harmonic_batch_upload(k, "X", xs[k])


def _vectors(s, k):
    """the kept vectors of system k (every fixture here has a conductor: vector 0 exists, and asking for it builds them)"""
    v0 = s.harmonic_batch_left_null_vector(k, 0)
    return [v0] + [s.harmonic_batch_left_null_vector(k, i) for i in range(1, s.harmonic_batch_null_projection(k)["kept"])]


def _single_projected(s, omega, b, x0, tol, itmax):
    """the single projected solve on the same handle: (X^, (iter, restarts, stop_kind, relres), removed of the solve,
    harmonic_projected_residual() behind it); the single setting is left off"""
    s.harmonic_setup(omega)
    s.harmonic_set_null_projection(True, NULL_TOL)
    try:
        s.harmonic_upload("B", b)
        s.harmonic_upload("X", x0)
        s.harmonic_solve(tol, itmax)
        i = s.harmonic_info()
        removed = s.harmonic_null_projection()["removed"]
        return (s.harmonic_download("X"), (i["iter"], i["restarts"], i["stop_kind"], i["relres"]), removed,
                s.harmonic_projected_residual())
    finally:
        s.harmonic_set_null_projection(False)


def _peek(s, k, w):
    ptr, n_pad = s.harmonic_batch_device_vector(k, w)
    return Z.peek(ptr, 2 * n_pad).view(np.float64).reshape(n_pad, 2).copy().view(np.complex128).reshape(-1)


@pytest.mark.parametrize("name", [G2, G8A])
def test_the_set_up_equals_the_twin_and_the_single_set_up(E, name):
    g, freqs = golden(name), FREQS[name]
    b = _rhs(g)
    n, S = len(b), len(freqs)
    xs = [_random_complex(n, 50 + k) for k in range(S)]
    bs = [b * (1.0 + k) for k in range(S)]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        x1, b1 = _random_complex(n, 60), _random_complex(n, 61)
        s.harmonic_setup(_w(freqs[0]))
        s.harmonic_upload("X", x1)
        s.harmonic_upload("B", b1)
        _batch(s, [_w(f) for f in freqs], bs, xs)
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        assert not s.harmonic_batch_null_projection(0)["built"]
        bytes0 = s.harmonic_batch_info(0)["device_bytes"]
        W = [_vectors(s, k) for k in range(S)]
        info = [s.harmonic_batch_null_projection(k) for k in range(S)]
        n_pad = s.vector_layout()["n_pad"]
        assert s.harmonic_batch_info(0)["device_bytes"] - bytes0 >= S * (info[0]["kept"] + 1) * n_pad * 16
        for k in range(S):
            _same(s.harmonic_batch_download(k, "X"), xs[k], f"X^ of system {k} across the set-up")
            _same(s.harmonic_batch_download(k, "B"), bs[k], f"B^ of system {k} across the set-up")
        _same(s.harmonic_download("X"), x1, "the single X^ across the set-up")
        _same(s.harmonic_download("B"), b1, "the single B^ across the set-up")
        single = []
        for f in freqs:                                     # the single set-up at every omega, on the same handle
            s.harmonic_setup(_w(f))
            s.harmonic_set_null_projection(True, NULL_TOL)
            v0 = s.harmonic_left_null_vector(0)
            q = s.harmonic_null_projection()
            single.append((q, [v0] + [s.harmonic_left_null_vector(i) for i in range(1, q["kept"])]))
            s.harmonic_set_null_projection(False)
    ncomp = 2 if name == G8A else 1
    its = []
    for k, f in enumerate(freqs):
        t = twin(name, f, sums)
        q = info[k]
        print(f"{name} {f:g} Hz: batch {[(c['iterations'], c['restarts'], c['residual']) for c in q['components']]}, twin "
              f"{[(c['iterations'], c['restarts'], c['residual']) for c in t['info']]}, set-up {q['setup_ms']:.0f} ms")
        assert q["built"] and q["on"] and q["found"] == len(t["info"]) == ncomp and q["dropped"] == 0 and q["shares_with"] == k
        assert q["kept"] == len(t["Q"]) == len(W[k]) == ncomp and q["null_tol"] == NULL_TOL
        q1, V1 = single[k]
        assert q1["kept"] == q["kept"]
        for c, w, c1 in zip(q["components"], t["info"], q1["components"]):
            assert (c["seed_row"], c["iterations"], c["restarts"], c["kept"]) == (w["seed"], w["iterations"], w["restarts"], w["kept"])
            assert (c["seed_row"], c["iterations"], c["restarts"], c["kept"]) == (c1["seed_row"], c1["iterations"], c1["restarts"],
                                                                                c1["kept"])
            assert c["iterations"] <= HH.adjoint_cap(t["op"].n)
            assert abs(c["residual"] - w["residual"]) <= 1e-12 * w["residual"] and c["residual"] == c1["residual"]
            its.append(c["iterations"])
        for i in range(ncomp):
            _same(W[k][i], t["Q"][i], f"{name} {f:g} Hz kept vector {i} against the twin")
            _same(W[k][i], V1[i], f"{name} {f:g} Hz kept vector {i} against the single set-up")
    # the premise: the systems stop in different polls of the lock-step adjoint iteration
    per_comp = [[q["components"][i]["iterations"] for q in info] for i in range(ncomp)]
    assert min(its) > 16 and all(len({(it + 15) // 16 for it in row}) > 1 for row in per_comp), "not the case it is meant to be"


@pytest.mark.parametrize("case", ["g2", "g3-pitched"])
def test_the_projection_equals_the_twin_bit_for_bit(E, monkeypatch, case):
    if case == "g3-pitched":
        monkeypatch.setenv("EC3D_PITCH", "2")
    g = load_golden(G2 if case == "g2" else G3)
    b = _rhs(g)
    n_ref = len(b)
    freqs = (50.0, 500.0, 50.0)
    xs = [1e-3 * _random_complex(n_ref, 70 + k) for k in range(3)]
    bs = [b, b, 2.0 * b]
    tol = 1e-6
    with E.EC3DSolver() as s:
        _assemble(s, g)
        lay, rm = s.vector_layout(), s.row_map().astype(np.int64)
        if case == "g3-pitched":
            sdz, sdy, sdx = g["geoPHYS"].shape
            assert rm[sdx * sdy] - rm[0] > sdx * sdy, "not the case it is meant to be"
        sums = _sums(s)
        _batch(s, [_w(f) for f in freqs], bs, xs)
        assert [it for it, _ in s.harmonic_batch_solve(tol, -1)] == [0, 0, 0]
        s.synchronize()
        plain = [_peek(s, k, "R") for k in range(3)]
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        solved = s.harmonic_batch_solve(tol, -1)
        s.synchronize()
        got = [[_peek(s, k, w) for w in ("R", "R0", "P")] for k in range(3)]
        info = [s.harmonic_batch_null_projection(k) for k in range(3)]
        W = [_vectors(s, k) for k in range(3)]
        for k in range(3):
            _same(s.harmonic_batch_download(k, "X"), xs[k], f"X^ of system {k}")
    n, n_pad = int(lay["n"]), int(lay["n_pad"])
    for k in range(3):
        assert info[k]["kept"] == len(W[k]) >= 1 and solved[k][0] == 0
        Qd = []
        for w in W[k]:
            d = np.zeros(n_pad, np.complex128)
            d[rm] = w
            Qd.append(d)
        want, c, rr = HH.project_device(Qd, plain[k], n)
        for nm, v in zip(("R", "R0", "P"), got[k]):
            assert np.array_equal(_bits(v[rm]), _bits(want[rm])), f"system {k} {nm}: {np.count_nonzero(v[rm] != want[rm])} rows differ"
        assert not np.array_equal(_bits(want[rm]), _bits(plain[k][rm]))             # (it did something)
        bk = HN.split(bs[k])
        bnorm = np.sqrt(sums(bk[0] * bk[0] + bk[1] * bk[1]))
        assert solved[k][1] == np.sqrt(DS.strided(rr)) / bnorm                  # the HP_RR partials, as k_hb_setup read them
        wb = float(np.sqrt(np.sum(np.abs(c) ** 2)) / bnorm)
        assert abs(info[k]["removed"] - wb) <= 1e-6 * wb
        print(f"{case} system {k}: adjoint {[q['iterations'] for q in info[k]['components']]}, removed {info[k]['removed']:.6e}")


@pytest.mark.parametrize("name", [G2, G8A])
def test_whole_projected_iterations_equal_the_twin_bit_for_bit(E, name):
    g, freqs = golden(name), FREQS[name]
    b = _rhs(g)
    n, S = len(b), len(freqs)
    xs = [1e-3 * _random_complex(n, 80 + k) for k in range(S)]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        _batch(s, [_w(f) for f in freqs], [b] * S, xs)
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        got = {}
        for itmax in (1, 5, 20):
            for k in range(S):
                s.harmonic_batch_upload(k, "X", xs[k])
            solved = s.harmonic_batch_solve(0.0, itmax)
            assert [it for it, _ in solved] == [itmax + 1] * S
            got[itmax] = [(s.harmonic_batch_download(k, "X"), _report(s, k), s.harmonic_batch_null_projection(k)["removed"])
                          for k in range(S)]
    for k, f in enumerate(freqs):
        t = twin(name, f, sums)
        trace = []
        *_, rel_t, kind_t, removed_t = HH.bicgstab_projected(t["op"], sums, t["Q"], HN.split(b), HN.split(xs[k]), 0.0, 20, trace=trace)
        for itmax in (1, 5, 20):
            x, rep, removed = got[itmax][k]
            _same(x, trace[itmax][1], f"{name} {f:g} Hz itmax = {itmax}")
            assert rep[:3] == (itmax + 1, trace[itmax][2], 0) and removed == removed_t
        assert got[20][k][1][3] == rel_t and kind_t == 0


@pytest.mark.parametrize("name", [G2, G8A])
def test_convergence_below_the_floor_in_every_system(E, name):
    g, freqs = golden(name), FREQS[name]
    b = _rhs(g)
    n, S = len(b), len(freqs)
    zero = np.zeros(n)
    tol, itmax = 1e-6, 2000
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        _batch(s, [_w(f) for f in freqs], [b] * S, [zero] * S)
        off = s.harmonic_batch_solve(tol, itmax)
        off_kinds = [_report(s, k)[2] for k in range(S)]
        for k in range(S):
            s.harmonic_batch_upload(k, "X", zero)
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        solved = s.harmonic_batch_solve(tol, itmax)
        rep = [_report(s, k) for k in range(S)]
        x = [s.harmonic_batch_download(k, "X") for k in range(S)]
        removed = [s.harmonic_batch_null_projection(k)["removed"] for k in range(S)]      # of the solve's projection ...
        pres = s.harmonic_batch_projected_residual()
        removed_after = [s.harmonic_batch_null_projection(k)["removed"] for k in range(S)]  # ... and of the last one
        for k in range(S):
            _same(s.harmonic_batch_download(k, "X"), x[k], f"X^ of system {k} across the projected residual")
            _same(s.harmonic_batch_download(k, "B"), b, f"B^ of system {k} across the projected residual")
        single = [_single_projected(s, _w(f), b, zero, tol, itmax) for f in freqs]
    assert [it for it, _ in off] == [itmax + 1] * S and off_kinds == [0] * S, "the plain batch is expected to stall above 1e-6"
    for k, f in enumerate(freqs):
        t = twin(name, f, sums)
        xt, it_t, rs_t, rel_t, kind_t, removed_t = HH.bicgstab_projected(t["op"], sums, t["Q"], HN.split(b), HN.split(zero), tol, itmax)
        twin_pres, twin_removed = HH.projected_residual(t["op"], sums, t["Q"], HN.split(b), xt)
        x1, rep1, removed1, pres1 = single[k]
        print(f"{name} {f:g} Hz: batch {rep[k]}, twin {(it_t, rs_t, kind_t, rel_t)}, single {rep1}; projected residual {pres[k]!r}, "
              f"twin {(twin_pres, twin_removed)!r}, single {pres1!r}; removed {removed[k]!r}, twin {removed_t!r}, single {removed1!r}")
        assert rep[k][0] <= itmax and rep[k][2] in (1, 2) and rep[k][3] < tol, "every system exits"
        assert rep[k] == (it_t, rs_t, kind_t, rel_t) and solved[k] == (it_t, rel_t)
        _same(x[k], xt, f"{name} {f:g} Hz against the twin")
        assert removed[k] == removed_t
        assert pres[k][0] <= 10 * tol and pres[k] == (twin_pres, twin_removed) and removed_after[k] == pres[k][1]
        assert rep1 == rep[k] and removed1 == removed[k] and pres1 == pres[k]
        _same(x[k], x1, f"{name} {f:g} Hz against the single projected solve")


def test_systems_with_equal_omega_share_one_set_of_vectors(E):
    g = golden(G2)
    b = _rhs(g)
    n = len(b)
    freqs = (50.0, 500.0, 50.0)
    bs = [b, g["b1"] + 1j * g["b0"], g["b0"].astype(np.complex128)]
    zero = np.zeros(n)
    tol, itmax = 1e-6, 2000
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        n_pad = s.vector_layout()["n_pad"]
        _batch(s, [_w(f) for f in freqs], bs, [zero] * 3)
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        bytes0 = s.harmonic_batch_info(0)["device_bytes"]
        solved = s.harmonic_batch_solve(tol, itmax)
        grew = s.harmonic_batch_info(0)["device_bytes"] - bytes0
        info = [s.harmonic_batch_null_projection(k) for k in range(3)]
        W = [_vectors(s, k) for k in range(3)]
        rep = [_report(s, k) for k in range(3)]
        x = [s.harmonic_batch_download(k, "X") for k in range(3)]
    assert [q["shares_with"] for q in info] == [0, 1, 0]
    assert info[2]["components"] == info[0]["components"] != info[1]["components"]
    for a, c in zip(W[2], W[0]):
        _same(a, c, "system 2's vector against system 0's")
    # two sets, each one vector of Q and one staging vector of n_pad pairs (a third set would be two vectors more)
    assert 4 * 16 * n_pad <= grew < 6 * 16 * n_pad, f"device_bytes grew by {grew}"
    for k, f in enumerate(freqs):
        t = twin(G2, f, sums)
        xt, it_t, rs_t, rel_t, kind_t, removed_t = HH.bicgstab_projected(t["op"], sums, t["Q"], HN.split(bs[k]), HN.split(zero), tol,
                                                                         itmax)
        print(f"system {k} at {f:g} Hz: batch {rep[k]}, twin {(it_t, rs_t, kind_t, rel_t)}")
        assert rep[k] == (it_t, rs_t, kind_t, rel_t) and solved[k] == (it_t, rel_t) and kind_t != 0
        assert info[k]["removed"] == removed_t
        _same(x[k], xt, f"system {k} against its twin")


def _stream_wgs(n_pad):
    return min(n_pad // DS.TILE, DS.WGS)        # ec3d_stream_wgs


def test_a_batch_of_one_is_the_single_projected_solve(E):
    """The single solve and the batch are one code path at S = 1 and S > 1: a batch of one system with the projection on
    against the single set-up and the single projected solve on the same handle, bit for bit; the single projection's
    memory is Q, its partials and its coefficients, with no staging vector and no table of its own."""
    g = golden(G8A)
    b = _rhs(g)
    n, w = len(b), _w(50.0)
    x0 = 1e-3 * _random_complex(n, 95)
    runs = ((0.0, 5, x0), (1e-6, 2000, np.zeros(n)))      # (from zero every g8a system exits below 1e-6)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        n_pad = s.vector_layout()["n_pad"]
        _batch(s, [w], [b], [x0])
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        W = _vectors(s, 0)
        info = s.harmonic_batch_null_projection(0)
        got = []
        for tol, itmax, xin in runs:
            s.harmonic_batch_upload(0, "X", xin)
            solved = s.harmonic_batch_solve(tol, itmax)
            got.append((s.harmonic_batch_download(0, "X"), _report(s, 0), s.harmonic_batch_null_projection(0)["removed"], solved))
        s.harmonic_setup(w)
        base = s.harmonic_info()["device_bytes"]
        s.harmonic_set_null_projection(True, NULL_TOL)
        V = [s.harmonic_left_null_vector(0)]
        info1 = s.harmonic_null_projection()
        V += [s.harmonic_left_null_vector(i) for i in range(1, info1["kept"])]
        grew = s.harmonic_info()["device_bytes"] - base
        s.harmonic_set_null_projection(False)
        single = [_single_projected(s, w, b, xin, tol, itmax) for tol, itmax, xin in runs]
    ncomp = 2
    print(f"batch of one {info['components']}, single {info1['components']}; reports {[q[1] for q in got]}, single "
          f"{[q[1] for q in single]}; device_bytes of the single projection {grew}")
    assert info["built"] and info1["built"] and info["shares_with"] == 0
    assert info["found"] == info1["found"] == info["kept"] == info1["kept"] == len(W) == len(V) == ncomp
    assert info["components"] == info1["components"]          # seed_row, iterations, residual, kept, restarts
    for i in range(ncomp):
        _same(W[i], V[i], f"kept vector {i}: the batch of one against the single set-up")
    for (tol, itmax, _), (x, rep, removed, solved), (x1, rep1, removed1, _) in zip(runs, got, single):
        assert rep == rep1 and removed == removed1 and solved == [(rep1[0], rep1[3])]
        _same(x, x1, f"X^ behind tol = {tol:g}, itmax = {itmax}: the batch of one against the single projected solve")
    assert got[0][1][0] == 6 and got[0][1][2] == 0 and got[1][1][2] in (1, 2) and got[1][1][3] < 1e-6
    assert grew == (ncomp * 2 * n_pad + 2 * ncomp * _stream_wgs(n_pad) + 2 * ncomp) * 8


def test_three_systems_of_one_omega_share_one_set(E):
    """D = 1 < S: one set of vectors, one staging vector and one table for three systems, partials and coefficients per
    system; equal right-hand sides give equal bits."""
    g = golden(G2)
    b = _rhs(g)
    n, w, S = len(b), _w(50.0), 3
    x0 = 1e-3 * _random_complex(n, 96)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        n_pad = s.vector_layout()["n_pad"]
        _batch(s, [w] * S, [b] * S, [x0] * S)
        base = s.harmonic_batch_info(0)["device_bytes"]
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        solved = s.harmonic_batch_solve(0.0, 5)
        grew = s.harmonic_batch_info(0)["device_bytes"] - base
        info = [s.harmonic_batch_null_projection(k) for k in range(S)]
        rep = [_report(s, k) for k in range(S)]
        x = [s.harmonic_batch_download(k, "X") for k in range(S)]
    assert [q["shares_with"] for q in info] == [0] * S and info[0]["built"]
    D, ncomp, G = 1, info[0]["found"], _stream_wgs(n_pad)
    assert ncomp == info[0]["kept"] == 1
    # the batch itself: S * (8 vectors of 2 n_pad + a table of 2 nt + 10 * G partials) + 2 n_pad of staging doubles and S
    # states of 112 bytes; nt = 16 pairs per class, which no report shows, from there
    words, odd = divmod(base - 112 * S, 8)
    per_system, odd2 = divmod(words - 2 * n_pad, S)
    two_nt = per_system - 16 * n_pad - 10 * G
    assert odd == 0 and odd2 == 0 and two_nt > 0 and two_nt % 32 == 0
    print(f"device_bytes: batch {base}, its projection {grew}; n_pad {n_pad}, G {G}, classes {two_nt // 32}")
    assert grew == (D * ncomp * 2 * n_pad + D * 2 * n_pad + D * two_nt + S * 2 * ncomp * G + S * 2 * ncomp) * 8
    assert [it for it, _ in solved] == [6] * S and rep[1] == rep[0] and rep[2] == rep[0]
    assert info[1]["removed"] == info[0]["removed"] == info[2]["removed"] > 0.0
    for k in (1, 2):
        _same(x[k], x[0], f"X^ of system {k} against system 0's")


def test_no_cross_talk(E):
    g = golden(G2)
    b = _rhs(g)
    n = len(b)
    tol, itmax = 1e-6, 300
    x0 = [1e-6 * _random_complex(n, 30 + k) for k in range(3)]
    x0.append(x0[0])
    bs = [b, np.zeros(n, np.complex128), b.copy(), b]
    bs[2][np.flatnonzero(b)[3]] = complex(np.nan, 1.0)
    freqs = (50.0, 200.0, 500.0, 50.0)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        _batch(s, [_w(f) for f in freqs], bs, x0)
        s.harmonic_batch_set_null_projection(True, NULL_TOL)
        solved = s.harmonic_batch_solve(tol, itmax)                     # (ends without an error)
        x = [s.harmonic_batch_download(k, "X") for k in range(4)]
        rep = [_report(s, k) for k in range(4)]
        removed = [s.harmonic_batch_null_projection(k)["removed"] for k in range(4)]
    t = twin(G2, 50.0, sums)
    xt, it_t, rs_t, rel_t, kind_t, removed_t = HH.bicgstab_projected(t["op"], sums, t["Q"], HN.split(b), HN.split(x0[0]), tol, itmax)
    print(f"reports {rep}, twin {(it_t, rs_t, kind_t, rel_t)}")
    assert 16 < it_t <= itmax and kind_t != 0, "not the case it is meant to be"
    assert rep[0] == rep[3] == (it_t, rs_t, kind_t, rel_t) and removed[0] == removed[3] == removed_t
    _same(x[0], xt, "system 0 against the twin")
    _same(x[3], xt, "system 3 against the twin")
    assert rep[1][0] == 0 and rep[1][2] == 0 and solved[1][0] == 0 and removed[1] == 0.0
    _same(x[1], x0[1], "b^ = 0: X^ as uploaded")
    assert rep[2][0] == itmax + 1 and rep[2][2] == 0


def test_a_null_tol_no_solve_reaches(E):
    g = golden(G2)
    b = _rhs(g)
    n = len(b)
    freqs = (50.0, 500.0)
    xs = [_random_complex(n, 90 + k) for k in range(2)]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        _batch(s, [_w(f) for f in freqs], [b, b], xs)
        bytes0 = s.harmonic_batch_info(0)["device_bytes"]
        s.harmonic_batch_set_null_projection(True, 1e-30)
        with pytest.raises(E.EC3DError, match=r"system [01] .*component 0 \(seed row 10242\)") as e:
            s.harmonic_batch_solve(1e-6, 100)
        assert e.value.status == NULL_E_SETUP
        for k in range(2):
            _same(s.harmonic_batch_download(k, "X"), xs[k], f"x^ of system {k} after the refused solve")
            _same(s.harmonic_batch_download(k, "B"), b, f"b^ of system {k} after the refused solve")
            q = s.harmonic_batch_null_projection(k)
            assert not q["built"] and q["on"] and q["kept"] == 0 and q["null_tol"] == 1e-30 and q["components"] == []
        assert s.harmonic_batch_info(0)["device_bytes"] == bytes0, "no vector is kept"
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_batch_left_null_vector(0, 0)
        assert e.value.status == NULL_E_SETUP
        s.harmonic_batch_set_null_projection(False)
        solved = s.harmonic_batch_solve(0.0, 5)
        for k, f in enumerate(freqs):
            xt, it_t, rs_t, rel_t, kind_t = HN.bicgstab(HN.Operator(g, _w(f)), sums, HN.split(b), HN.split(xs[k]), 0.0, 5)
            assert _report(s, k) == (it_t, rs_t, kind_t, rel_t) and solved[k] == (6, rel_t)
            _same(s.harmonic_batch_download(k, "X"), xt, f"the unprojected solve behind the refusal, {f:g} Hz")


def test_the_contract(E):
    g = golden(G2)
    tol, itmax = 0.02, 40
    b = _rhs(g)
    ws = [_w(50.0), _w(500.0)]

    def solve(s):
        for k in range(2):
            s.harmonic_batch_upload(k, "B", b)
            s.harmonic_batch_upload(k, "X", np.zeros(s.n))
        solved = s.harmonic_batch_solve(tol, itmax)
        return solved, [_report(s, k) for k in range(2)], [s.harmonic_batch_download(k, "X") for k in range(2)]

    def same_solve(a, c, what):
        assert a[:2] == c[:2], what
        for k in range(2):
            _same(a[2][k], c[2][k], f"{what}, system {k}")

    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.harmonic_batch_setup(ws)
        fresh = solve(s)
        assert s.harmonic_batch_null_projection(1) == dict(on=False, built=False, found=0, kept=0, dropped=0, null_tol=1e-10,
                                                           removed=0.0, setup_ms=0.0, components=[], shares_with=1)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.upload("B", g["b1"])
        s.upload("X", g["xin1"])
        s.solve_resident(float(g["tol"]), int(g["itmax"]))          # the real work vectors hold a solve's leftovers
        s.harmonic_setup(ws[1])                                     # the single solve's own Q, at ANOTHER omega than system 0's
        s.harmonic_upload("B", _random_complex(s.n, 1))
        s.harmonic_upload("X", _random_complex(s.n, 2))
        s.harmonic_set_null_projection(True, 1e-9)
        q_single = s.harmonic_left_null_vector(0)
        s.harmonic_set_null_projection(False)
        single_before = s.harmonic_null_projection()
        assert single_before["built"] and single_before["null_tol"] == 1e-9
        hx, n_pad = s.harmonic_device_vector("X")
        hb, _ = s.harmonic_device_vector("B")
        s.harmonic_batch_setup(ws)
        s.synchronize()
        xb_before = Z.peek(hx, 2 * n_pad), Z.peek(hb, 2 * n_pad)
        base, before = Z.owned_block(s)
        rings_before = Z.rings(s)
        s.harmonic_batch_set_null_projection(True)
        on = solve(s)
        s.harmonic_batch_projected_residual()
        s.synchronize()
        assert np.array_equal(Z.peek(hx, 2 * n_pad), xb_before[0]) and np.array_equal(Z.peek(hb, 2 * n_pad), xb_before[1])
        base2, after = Z.owned_block(s)
        assert base2 == base and np.array_equal(before, after), "a real vector changed under the set-up or the projected batch"
        for k, v in Z.rings(s).items():
            assert np.array_equal(v, rings_before[k]), k
        assert s.harmonic_null_projection() == single_before, "the single solve's setting or report changed"
        _same(s.harmonic_left_null_vector(0), q_single, "the single solve's own Q")
        info = s.harmonic_batch_null_projection(0)
        assert info["built"] and info["on"] and info["kept"] == 1 and info["removed"] > 0.0 and info["null_tol"] == 1e-10
        s.harmonic_batch_set_null_projection(False)
        same_solve(solve(s), fresh, "off again")
        assert not np.array_equal(_bits(on[2][0]), _bits(fresh[2][0]))
        q = s.harmonic_batch_null_projection(0)
        assert q["built"] and not q["on"]                               # the vectors stay
        s.harmonic_batch_set_null_projection(True)
        assert s.harmonic_batch_null_projection(0)["built"], "the same null_tol keeps the vectors"
        s.harmonic_batch_set_null_projection(True, 1e-9)
        q = s.harmonic_batch_null_projection(0)
        assert not q["built"] and q["on"] and q["null_tol"] == 1e-9, "another null_tol makes the vectors again"
        s.harmonic_batch_left_null_vector(1, 0)
        assert s.harmonic_batch_null_projection(0)["built"]
        s.harmonic_batch_setup(ws)
        q = s.harmonic_batch_null_projection(0)
        assert not q["built"] and q["on"] and q["null_tol"] == 1e-9, "a new batch set-up clears the vectors and keeps the setting"
        s.harmonic_batch_left_null_vector(0, 0)
        assert s.harmonic_batch_null_projection(1)["built"]
        _assemble(s, g)
        with pytest.raises(E.EC3DError, match="ec3d_harmonic_batch_setup first") as e:
            s.harmonic_batch_null_projection(0)
        assert e.value.status == 2
        s.harmonic_batch_setup(ws)
        q = s.harmonic_batch_null_projection(0)
        assert not q["built"] and q["on"] and q["null_tol"] == 1e-9, "a new assembly clears the vectors and keeps the setting"
        s.harmonic_batch_set_null_projection(True, 0.0)                 # <= 0: the default
        assert s.harmonic_batch_null_projection(0)["null_tol"] == 1e-10
        same_solve(solve(s), on, "the rebuilt vectors")


def _null_calls(s):
    """Every entry point of the batch's null projection on system 0 through the C interface: [(name, status)]"""
    v = np.zeros(1 << 16)           # (longer than any matrix here)
    info, sw, rs, rel = NullInfo(), C.c_int32(0), np.zeros(32, np.int32), np.zeros(16)
    L = s.L
    return [("set", L.ec3d_harmonic_batch_set_null_projection(s.h, 1, 0.0)),
            ("get", L.ec3d_get_harmonic_batch_null(s.h, 0, C.byref(info), C.byref(sw))),
            ("vector", L.ec3d_harmonic_batch_left_null_vector(s.h, 0, 0, v.ctypes.data, v.ctypes.data)),
            ("restarts", L.ec3d_harmonic_batch_null_restarts(s.h, 0, rs.ctypes.data)),
            ("residual", L.ec3d_harmonic_batch_projected_residual(s.h, rel.ctypes.data, None)),
            ("off", L.ec3d_harmonic_batch_set_null_projection(s.h, 0, 0.0))]


def test_refusals(E):
    g = golden(G2)
    with E.EC3DSolver() as s:
        assert [rc for _, rc in _null_calls(s)] == [3] * 6                       # before ec3d_assemble
        s.assemble_poisson(8, 8, 8)
        assert [rc for _, rc in _null_calls(s)] == [3] * 6
        s.set_matrix_csr(g["valA"], g["irow"], g["jcol"])
        assert [rc for _, rc in _null_calls(s)] == [3] * 6                       # a CSR handle
        c = load_golden("g8c_side_by_side_20x18x14")                              # bands + tail
        s.assemble(c["geoPHYS"], c["geoPHYS_C"], c["valPHYS"], c["BND"], c["delta"], float(c["dt"]))
        assert s.info.tail_rows > 0
        assert [rc for _, rc in _null_calls(s)] == [NULL_E_MATRIX] * 6
        _assemble(s, g)
        assert [rc for _, rc in _null_calls(s)] == [2] * 5 + [0]                 # before a batch set-up: only "off" needs none
        with pytest.raises(E.EC3DError, match="ec3d_harmonic_batch_setup first"):
            s.harmonic_batch_set_null_projection(True)
        s.harmonic_batch_set_null_projection(False)                              # switching off needs no batch
        assert s.L.ec3d_harmonic_batch_set_null_projection(None, 0, 0.0) == 2
        b = _rhs(g)
        s.harmonic_batch_setup([_w(50.0), _w(500.0)])
        s.harmonic_batch_upload(0, "B", b)
        s.harmonic_batch_upload(1, "B", b)
        assert not s.harmonic_batch_null_projection(0)["on"], "a refusal leaves the setting as it was"
        v = np.zeros(s.n)
        info, sw, rs, rel = NullInfo(), C.c_int32(7), np.zeros(32, np.int32), np.zeros(16)
        L, p = s.L, v.ctypes.data
        assert L.ec3d_harmonic_batch_left_null_vector(s.h, 0, 0, p, p) == 2       # the setting is off: no vectors ...
        assert L.ec3d_harmonic_batch_projected_residual(s.h, rel.ctypes.data, None) == 2     # ... and no residual
        assert not s.harmonic_batch_null_projection(0)["built"]
        for sys in (-1, 2, 16):
            assert L.ec3d_get_harmonic_batch_null(s.h, sys, C.byref(info), C.byref(sw)) == 2
            assert L.ec3d_harmonic_batch_left_null_vector(s.h, sys, 0, p, p) == 2
            assert L.ec3d_harmonic_batch_null_restarts(s.h, sys, rs.ctypes.data) == 2
        assert sw.value == 7
        s.harmonic_batch_set_null_projection(True)
        for bad in (-1, 1, 7):
            with pytest.raises(E.EC3DError) as e:
                s.harmonic_batch_left_null_vector(1, bad)
            assert e.value.status == 2
        q = s.harmonic_batch_null_projection(1)
        assert q["on"] and q["built"] and q["kept"] == 1
        assert L.ec3d_get_harmonic_batch_null(s.h, 0, None, C.byref(sw)) == 2
        assert L.ec3d_get_harmonic_batch_null(s.h, 1, C.byref(info), None) == 0 and info.kept == 1
        assert L.ec3d_harmonic_batch_left_null_vector(s.h, 0, 0, None, p) == 2
        assert L.ec3d_harmonic_batch_left_null_vector(s.h, 0, 0, p, None) == 2
        assert L.ec3d_harmonic_batch_null_restarts(s.h, 0, None) == 2
        assert L.ec3d_harmonic_batch_projected_residual(s.h, None, None) == 2
        assert L.ec3d_harmonic_batch_projected_residual(s.h, rel.ctypes.data, None) == 0 and 0.0 < rel[0] <= 1.0
        # the single setting is refused by the batch solve exactly as before, whatever the batch's own setting is
        s.harmonic_setup(_w(50.0))
        s.harmonic_set_null_projection(True)
        with pytest.raises(E.EC3DError, match="ec3d_harmonic_set_null_projection is on, and its vectors belong to one omega") as e:
            s.harmonic_batch_solve(1e-3, 10)
        assert e.value.status == 2
        s.harmonic_set_null_projection(False)
        assert len(s.harmonic_batch_solve(1e-3, 3)) == 2
        assert s.harmonic_batch_null_projection(0)["on"] and not s.harmonic_null_projection()["on"]
    z = load_golden("g8b_stacked_moving_20x16x14")                        # a z-slab: planes [0, 9), owned [0, 7)
    geo = z["geoPHYS"][:9].copy()
    geoC = np.zeros(geo.shape, np.int32)
    q = np.concatenate([np.flatnonzero((geo.reshape(-1) == d) & (z["geoPHYS_C"][:9].reshape(-1) != 0)) for d in (1, 2)])
    geoC.reshape(-1)[q] = 3 * geo.size + 1 + np.arange(len(q))
    with E.EC3DSolver() as s:
        s.assemble_slab(z["geoPHYS"].shape[0], 0, 9, 0, 7, geo, geoC, z["valPHYS"], z["BND"], z["delta"], float(z["dt"]))
        assert [rc for _, rc in _null_calls(s)] == [5] * 6


def test_run_harmonic_sweep_with_the_projection_and_the_command_line(E, tmp_path, capsys):
    """host.run_harmonic_sweep(..., null_projection=True) on the shipped compare_to_Elmer model at two frequencies and the
    same through --harmonic F0 --sweep ... --sweep-null-projection."""
    import os
    from conftest import GOLDEN
    from eddy_currents_3d_amd import host, run, vxc
    path = os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc")
    model = vxc.read_vxc(path)
    tol, itmax = 1e-6, int(vxc.domain_tables(model)["itmax"])     # (the command line has the model's iteration limit)
    freqs = [25.0, 50.0]
    with E.EC3DSolver() as s:
        rs = host.run_harmonic_sweep(model, s, 50.0, freqs, tol=tol, itmax=itmax, null_projection=True)
        assert not s.harmonic_null_projection()["on"]
        s.harmonic_batch_setup([_w(50.0)])
        assert not s.harmonic_batch_null_projection(0)["on"], "the setting is put back as it was found"
    with E.EC3DSolver() as s2:
        r = host.run_harmonic(model, s2, 50.0, tol=tol, itmax=itmax, null_projection=True)
    assert [q["freq"] for q in rs] == freqs
    for q in rs:
        print(f"{q['freq']:g} Hz: iter {q['iter']}, relres {q['relres']:.3e}, projected residual {q['projected_residual']:.3e}, true "
              f"residual {q['true_residual']:.3e}, removed {q['removed']:.3e}, adjoint "
              f"{[c['iterations'] for c in q['null']['components']]}, set-up {q['null']['setup_ms']:.0f} ms")
        assert q["iter"] <= itmax and q["relres"] < tol and q["projected_residual"] <= 10 * tol
        assert q["null"]["built"] and q["null"]["kept"] >= 1
    at50 = rs[1]
    assert at50["iter"] == r["iter"] and at50["relres"] == r["relres"]
    assert at50["projected_residual"] == r["projected_residual"] and at50["removed"] == r["removed"]
    _same(at50["x"], r["x"], "x^ at 50 Hz: the projected sweep against run_harmonic")
    capsys.readouterr()
    assert run.main([path, "--harmonic", "50", "--sweep", "25,50", "--tol", "1e-6", "--sweep-null-projection", "--no-output"]) == 0
    text = capsys.readouterr().out
    adjoint = "+".join(str(c["iterations"]) for c in at50["null"]["components"])
    assert text.count("harmonic sweep ") == 2
    assert f"iter={at50['iter']} " in text
    assert f"projected residual={at50['projected_residual']:.3e} adjoint iterations={adjoint} " in text
