"""A batch of time-harmonic systems solved in lock step (ec3d_harmonic_batch_*; csrc/ec3d_harmonic.hip; DESIGN.md section
18b): up to 16 systems (omega_s, b^_s, x^_s) on one matrix ride in the five launches of an iteration, on a grid of
(workgroups, systems), and every system keeps the bits of its own single solve.  The twin of a batch is therefore
tests/harmonic_numpy.py's bicgstab run once per system, and a second reference is harmonic_setup + harmonic_solve on the
same handle.

* mixed exits on g2 and g8a: systems that take the ||S|| exit, the ||R|| exit and (g2) none, on both sides of the
  16-iteration poll: (iter, restarts, stop_kind, relres) and X^ equal the twin's and the single solve's bit for bit;
* pitched planes (g3, EC3D_PITCH=2) from a non-zero x0; the 96 x 96 x 64 box, whose 4608 chunks make the workgroups stride;
* no cross-talk: a system with b^ = 0 and one with a NaN in b^ beside two equal healthy ones;
* capacity (16 systems; 17 refused; nsys = 0 frees); NaN in the rows of no unknown; the memory contract; select; refusals;
  host.run_harmonic_sweep and --harmonic F0 --sweep on the shipped compare_to_Elmer model."""
import ctypes as C

import numpy as np
import pytest

import av_generate as AG
import guard_zones as Z
import harmonic_numpy as HN
from conftest import load_golden
from eddy_currents_3d_amd.solver import NULL_E_MATRIX, HarmonicInfo

pytestmark = pytest.mark.gpu
G2, G3, G8A = "g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12", "g8a_two_plates_18x16x16"
# name: (tol, itmax, frequencies [Hz], a system without an exit is part of the case)
MIXED = {G2: (0.02, 40, (5.0, 50.0, 200.0, 500.0, 2000.0), True),
         G8A: (0.05, 40, (5.0, 50.0, 200.0, 500.0, 2000.0, 10000.0), False)}


def _w(f):
    return 2.0 * np.pi * float(f)


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _assemble(s, g):
    s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))


def _sums(s):
    return HN.DeviceSums(s.row_map(), s.vector_layout()["n_pad"])


def _bits(z):
    z = np.asarray(z, np.complex128)
    return np.stack([z.real, z.imag]).view(np.uint64)


def _same(got, want, what):
    g = _bits(got)
    w = np.stack([want[0], want[1]]).view(np.uint64) if isinstance(want, tuple) else _bits(want)
    assert np.array_equal(g, w), f"{what}: {np.count_nonzero((g != w).any(axis=0))} of {g.shape[1]} rows differ"


def _random_complex(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _rhs(g):
    return g["b0"] + 1j * g["b1"]


def _report(s, k):
    i = s.harmonic_batch_info(k)
    return i["iter"], i["restarts"], i["stop_kind"], i["relres"]


def _single(s, omega, b, x0, tol, itmax):
    """harmonic_setup + upload + harmonic_solve on the same handle: (X^, (iter, restarts, stop_kind, relres))"""
    s.harmonic_setup(omega)
    s.harmonic_upload("B", b)
    s.harmonic_upload("X", x0)
    s.harmonic_solve(tol, itmax)
    i = s.harmonic_info()
    return s.harmonic_download("X"), (i["iter"], i["restarts"], i["stop_kind"], i["relres"])


@pytest.fixture(scope="module")
def mixed(E):
    """Per fixture of MIXED: an open handle whose batch has been solved, the twin's results with the device's row map,
    and what the batch reported."""
    out, open_ = {}, []
    try:
        for name, (tol, itmax, freqs, _) in MIXED.items():
            g = load_golden(name)
            s = E.EC3DSolver()
            open_.append(s)
            _assemble(s, g)
            sums = _sums(s)
            b = _rhs(g)
            n = len(b)
            zero = np.zeros(n)
            twin = [HN.bicgstab(HN.Operator(g, _w(f)), sums, HN.split(b), HN.split(zero), tol, itmax) for f in freqs]
            s.harmonic_batch_setup([_w(f) for f in freqs])
            for k in range(len(freqs)):
                s.harmonic_batch_upload(k, "B", b)
                s.harmonic_batch_upload(k, "X", zero)
            solved = s.harmonic_batch_solve(tol, itmax)
            out[name] = dict(g=g, s=s, b=b, twin=twin, solved=solved, x=[s.harmonic_batch_download(k, "X") for k in range(len(freqs))])
        yield out
    finally:
        for s in open_:
            s.close()


@pytest.mark.parametrize("name", [G2, G8A])
def test_mixed_exits_equal_the_twin_and_the_single_solve(mixed, name):
    c = mixed[name]
    tol, itmax, freqs, with_none = MIXED[name]
    s, b, twin = c["s"], c["b"], c["twin"]
    kinds = [t[4] for t in twin]
    exits = {t[1] for t in twin if t[4] != 0}
    print(f"{name}: twin (iter, restarts, exit) per frequency: {[(t[1], t[2], t[4]) for t in twin]}")
    assert 1 in kinds and 2 in kinds and (0 in kinds or not with_none) and len(exits) >= 2, "not the case it is meant to be"
    assert min(exits) <= 16 < max(t[1] for t in twin), "not the case it is meant to be"     # both sides of the poll
    assert len(c["solved"]) == len(freqs)
    zero = np.zeros(len(b))
    for k, f in enumerate(freqs):
        xt, it_t, rs_t, rel_t, kind_t = twin[k]
        got = _report(s, k)
        print(f"{name}: {f:g} Hz: batch {got}, twin {(it_t, rs_t, kind_t, rel_t)}")
        assert got == (it_t, rs_t, kind_t, rel_t), f"{f:g} Hz"
        assert c["solved"][k] == (it_t, rel_t)
        assert s.harmonic_batch_info(k)["omega"] == _w(f)
        _same(c["x"][k], xt, f"{name} {f:g} Hz against the twin")
        x1, rep1 = _single(s, _w(f), b, zero, tol, itmax)
        assert rep1 == got
        _same(c["x"][k], x1, f"{name} {f:g} Hz against the single solve")


def test_pitched_planes_from_a_nonzero_start(E, monkeypatch):
    monkeypatch.setenv("EC3D_PITCH", "2")
    g = load_golden(G3)
    sdz, sdy, sdx = g["geoPHYS"].shape
    b = _rhs(g)
    n = len(b)
    freqs = (5.0, 50.0, 500.0)
    x0 = [1e-3 * _random_complex(n, 20 + k) for k in range(3)]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        rm = s.row_map()
        assert rm[sdx * sdy] - rm[0] > sdx * sdy, "not the case it is meant to be"
        sums = _sums(s)
        s.harmonic_batch_setup([_w(f) for f in freqs])
        for k in range(3):
            s.harmonic_batch_upload(k, "B", b)
            s.harmonic_batch_upload(k, "X", x0[k])
        solved = s.harmonic_batch_solve(0.0, 5)
        for k, f in enumerate(freqs):
            xt, it_t, rs_t, rel_t, kind_t = HN.bicgstab(HN.Operator(g, _w(f)), sums, HN.split(b), HN.split(x0[k]), 0.0, 5)
            assert (it_t, kind_t) == (6, 0)
            assert _report(s, k) == (it_t, rs_t, kind_t, rel_t) and solved[k] == (6, rel_t)
            _same(s.harmonic_batch_download(k, "X"), xt, f"g3 pitched, {f:g} Hz")


def test_three_iterations_on_the_box(E):
    """96 x 96 x 64 cells with a conducting plate: 4608 chunks against 1024 workgroups, the grid-stride path."""
    geo, geoC, val, bnd, delta, dt = AG.from_boxes(
        (96, 96, 64), [dict(boxes=[((30, 66), (28, 70), (29, 35))], C=44.3, vel=(0.0, 0.0, 0.0))],
        [[-0.95, -0.95], [-0.95, -0.95], [-0.95, -0.95]], (0.004, 0.005, 0.003), 1e-3)
    g = dict(geoPHYS=geo, geoPHYS_C=geoC, valPHYS=val, BND=bnd, delta=delta, dt=dt)
    freqs = (50.0, 500.0)
    ops = [HN.Operator(g, _w(f)) for f in freqs]
    n, nC = ops[0].n, ops[0].nC
    rng = np.random.default_rng(11)
    b = np.zeros(n, np.complex128)
    coil = np.flatnonzero(np.asarray(geoC).reshape(-1) == 0)[::97][:4000]
    b[coil] = rng.standard_normal(len(coil)) + 1j * rng.standard_normal(len(coil))
    b[nC + coil] = rng.standard_normal(len(coil))
    zero = np.zeros(n)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        assert s.vector_layout()["n_pad"] // 512 > 1024
        sums = _sums(s)
        s.harmonic_batch_setup([_w(f) for f in freqs])
        for k in range(2):
            s.harmonic_batch_upload(k, "B", b)
            s.harmonic_batch_upload(k, "X", zero)
        solved = s.harmonic_batch_solve(0.0, 2)
        for k, f in enumerate(freqs):
            xt, it_t, rs_t, rel_t, kind_t = HN.bicgstab(ops[k], sums, HN.split(b), HN.split(zero), 0.0, 2)
            assert _report(s, k) == (3, rs_t, 0, rel_t) == (it_t, rs_t, kind_t, rel_t) and solved[k][0] == 3
            _same(s.harmonic_batch_download(k, "X"), xt, f"box, {f:g} Hz")


def test_no_cross_talk(E):
    g = load_golden(G2)
    b = _rhs(g)
    n = len(b)
    tol, itmax = 0.02, 40           # (from 1e-6 x random the twin takes the ||R|| exit of 50 Hz after 17 iterations)
    x0 = [1e-6 * _random_complex(n, 30 + k) for k in range(3)]
    x0.append(x0[0])
    bs = [b, np.zeros(n, np.complex128), b.copy(), b]
    bs[2][np.flatnonzero(b)[3]] = complex(np.nan, 1.0)
    omegas = [_w(50.0), _w(200.0), _w(500.0), _w(50.0)]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.harmonic_batch_setup(omegas)
        for k in range(4):
            s.harmonic_batch_upload(k, "B", bs[k])
            s.harmonic_batch_upload(k, "X", x0[k])
        solved = s.harmonic_batch_solve(tol, itmax)                     # (ends without an error)
        x = [s.harmonic_batch_download(k, "X") for k in range(4)]
        rep = [_report(s, k) for k in range(4)]
        x1, rep1 = _single(s, omegas[0], b, x0[0], tol, itmax)
        print(f"reports {rep}, single {rep1}")
        assert 0 < rep1[0] <= itmax, "not the case it is meant to be"
        assert rep[0] == rep[3] == rep1
        _same(x[0], x1, "system 0 against the single solve")
        _same(x[3], x1, "system 3 against the single solve")
        assert rep[1][0] == 0 and rep[1][2] == 0 and solved[1][0] == 0
        _same(x[1], x0[1], "b^ = 0: X^ as uploaded")
        assert rep[2][0] == itmax + 1 and rep[2][2] == 0


def test_capacity(E):
    g = load_golden(G2)
    b = _rhs(g)
    zero = np.zeros(len(b))
    tol, itmax = 0.02, 40
    info = HarmonicInfo()
    with E.EC3DSolver() as s:
        _assemble(s, g)
        x1, rep1 = _single(s, _w(50.0), b, zero, tol, itmax)
        bytes_single = s.harmonic_info()["device_bytes"]
        s.harmonic_batch_setup([_w(50.0)] * 16)
        for k in range(16):
            s.harmonic_batch_upload(k, "B", b)
            s.harmonic_batch_upload(k, "X", zero)
        assert len(s.harmonic_batch_solve(tol, itmax)) == 16
        for k in range(16):
            assert _report(s, k) == rep1
            _same(s.harmonic_batch_download(k, "X"), x1, f"system {k} of 16")
        n_pad = s.vector_layout()["n_pad"]
        got = s.harmonic_batch_info(0)["device_bytes"]
        assert 16 * 128 * n_pad <= got <= 16 * 144 * n_pad + (1 << 20)
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_batch_setup([_w(50.0)] * 17)
        assert e.value.status == 2
        _same(s.harmonic_batch_download(15, "X"), x1, "the batch after a refused set-up")
        s.harmonic_batch_upload(15, "X", zero)
        s.harmonic_batch_solve(tol, itmax)
        _same(s.harmonic_batch_download(15, "X"), x1, "the batch solved again after a refused set-up")
        s.harmonic_batch_setup([])
        v = np.zeros(s.n)
        p, m = C.c_void_p(), C.c_int64(0)
        for rc in (s.L.ec3d_harmonic_batch_upload(s.h, 0, 0, v.ctypes.data, v.ctypes.data),
                   s.L.ec3d_harmonic_batch_download(s.h, 0, 0, v, v),
                   s.L.ec3d_harmonic_batch_solve(s.h, tol, itmax, None),
                   s.L.ec3d_get_harmonic_batch(s.h, 0, C.byref(info)),
                   s.L.ec3d_harmonic_batch_select(s.h, 0),
                   s.L.ec3d_harmonic_batch_device_vector(s.h, 0, 0, C.byref(p), C.byref(m))):
            assert rc == 2
        assert s.harmonic_info()["device_bytes"] == bytes_single
        _same(s.harmonic_download("X"), x1, "the single solve's X^ through all of it")


def test_nan_in_the_rows_of_no_unknown(E):
    g = load_golden(G2)
    b = _rhs(g)
    n = len(b)
    freqs = (50.0, 500.0)
    x0 = [1e-3 * _random_complex(n, 40 + k) for k in range(2)]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        s.harmonic_batch_setup([_w(f) for f in freqs])
        for k in range(2):
            s.harmonic_batch_upload(k, "B", b)
            s.harmonic_batch_upload(k, "X", x0[k])
            ptr, n_pad = s.harmonic_batch_device_vector(k, "X")
            s.synchronize()
            v = Z.peek(ptr, 2 * n_pad).view(np.float64).reshape(n_pad, 2).copy()
            hidden = np.setdiff1d(np.arange(n_pad), s.row_map())
            assert len(hidden) > 0 and not v[hidden].any()
            v[hidden] = np.nan
            Z.poke(ptr, v.reshape(-1))
        s.harmonic_batch_solve(0.0, 5)
        for k, f in enumerate(freqs):
            xt, it_t, rs_t, rel_t, kind_t = HN.bicgstab(HN.Operator(g, _w(f)), sums, HN.split(b), HN.split(x0[k]), 0.0, 5)
            assert _report(s, k) == (6, rs_t, 0, rel_t) == (it_t, rs_t, kind_t, rel_t)
            _same(s.harmonic_batch_download(k, "X"), xt, f"NaN in the rows of no unknown, {f:g} Hz")


def test_memory_contract_and_the_transient_solve_afterwards(E):
    g = load_golden(G2)
    tol, itmax = float(g["tol"]), int(g["itmax"])
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.upload("B", g["b1"])
        s.upload("X", g["xin1"])
        it0, _ = s.solve_resident(tol, itmax)           # the work vectors hold a solve's leftovers
        x_first = s.download("X")
        s.upload("X", g["xin1"])
        s.harmonic_setup(_w(50.0))
        s.harmonic_upload("B", _random_complex(s.n, 1))
        s.harmonic_upload("X", _random_complex(s.n, 2))
        hx, n_pad = s.harmonic_device_vector("X")
        hb, _ = s.harmonic_device_vector("B")
        s.synchronize()
        single_before = Z.peek(hx, 2 * n_pad), Z.peek(hb, 2 * n_pad)
        base, before = Z.owned_block(s)
        rings_before = Z.rings(s)
        s.harmonic_batch_setup([_w(50.0), _w(500.0)])
        for k in range(2):
            s.harmonic_batch_upload(k, "B", g["b0"] + 1j * g["b1"])
            s.harmonic_batch_upload(k, "X", np.zeros(s.n))
        solved = s.harmonic_batch_solve(tol, itmax)
        assert all(0 < it <= itmax for it, _ in solved)
        s.harmonic_batch_download(1, "X")
        s.synchronize()
        assert np.array_equal(Z.peek(hx, 2 * n_pad), single_before[0]), "the single X^ changed under the batch"
        assert np.array_equal(Z.peek(hb, 2 * n_pad), single_before[1]), "the single B^ changed under the batch"
        base2, after = Z.owned_block(s)
        assert base2 == base and np.array_equal(before, after), "a real vector changed under the batch"
        for k, v in Z.rings(s).items():
            assert np.array_equal(v, rings_before[k]), k
        it1, _ = s.solve_resident(tol, itmax)
        x_after = s.download("X")
        assert it1 == it0 and 0 < it0 <= itmax
        assert np.array_equal(x_after.view(np.uint64), x_first.view(np.uint64))
        _assemble(s, g)                                 # a new matrix clears the batch
        with pytest.raises(E.EC3DError, match="ec3d_harmonic_batch_setup first") as e:
            s.harmonic_batch_download(0, "X")
        assert e.value.status == 2


def test_select(mixed):
    c = mixed[G2]
    tol, itmax, freqs, _ = MIXED[G2]
    s, g, b = c["s"], c["g"], c["b"]
    for k in (1, 4):
        s.harmonic_batch_select(k)
        x = s.harmonic_download("X")
        _same(x, c["x"][k], f"X^ of system {k} selected")
        _same(s.harmonic_download("B"), s.harmonic_batch_download(k, "B"), f"B^ of system {k} selected")
        _same(s.harmonic_download("B"), b, f"B^ of system {k} as uploaded")
        assert s.harmonic_info()["omega"] == _w(freqs[k])
        ax = HN.Operator(g, _w(freqs[k]))(HN.split(x))
        r = b.real - ax[0], b.imag - ax[1]
        twin_true = np.sqrt(np.sum(r[0] * r[0] + r[1] * r[1])) / np.linalg.norm(b)
        true, bnorm = s.harmonic_true_residual()
        print(f"system {k}: true residual {true:.6e}, twin {twin_true:.6e}")
        assert abs(true - twin_true) <= 1e-12 * twin_true
        for part in (0, 1):
            s.harmonic_load(part)
            X = s.download("X")
            assert np.any(X != 0.0) and np.all(np.isfinite(X))
        for j in range(len(freqs)):
            _same(s.harmonic_batch_download(j, "X"), c["x"][j], f"system {j} of the batch after select({k})")


def _batch_calls(s):
    """Every batch entry point on system 0 through the C interface: [(name, status)]"""
    v = np.zeros(1 << 16)           # (longer than any matrix here: no call gets as far as reading it)
    w = np.array([_w(50.0)])
    info, p, m = HarmonicInfo(), C.c_void_p(), C.c_int64(0)
    L = s.L
    return [("setup", L.ec3d_harmonic_batch_setup(s.h, 1, w.ctypes.data)),
            ("upload", L.ec3d_harmonic_batch_upload(s.h, 0, 0, v.ctypes.data, v.ctypes.data)),
            ("download", L.ec3d_harmonic_batch_download(s.h, 0, 0, v, v)),
            ("solve", L.ec3d_harmonic_batch_solve(s.h, 1e-3, 10, None)),
            ("get", L.ec3d_get_harmonic_batch(s.h, 0, C.byref(info))),
            ("select", L.ec3d_harmonic_batch_select(s.h, 0)),
            ("device_vector", L.ec3d_harmonic_batch_device_vector(s.h, 0, 0, C.byref(p), C.byref(m)))]


def test_refusals(E):
    g = load_golden(G2)
    with E.EC3DSolver() as s:
        assert [rc for _, rc in _batch_calls(s)] == [3] * 7                      # before ec3d_assemble
        s.assemble_poisson(8, 8, 8)
        assert [rc for _, rc in _batch_calls(s)] == [3] * 7
        s.set_matrix_csr(g["valA"], g["irow"], g["jcol"])
        assert [rc for _, rc in _batch_calls(s)] == [3] * 7                      # a CSR handle
        c = load_golden("g8c_side_by_side_20x18x14")                              # bands + tail
        s.assemble(c["geoPHYS"], c["geoPHYS_C"], c["valPHYS"], c["BND"], c["delta"], float(c["dt"]))
        assert s.info.tail_rows > 0
        assert [rc for _, rc in _batch_calls(s)] == [NULL_E_MATRIX] * 7
        _assemble(s, g)
        v = np.zeros(s.n)
        info, p, m = HarmonicInfo(), C.c_void_p(), C.c_int64(0)
        for name, rc in (("upload", s.L.ec3d_harmonic_batch_upload(s.h, 0, 0, v.ctypes.data, v.ctypes.data)),
                         ("download", s.L.ec3d_harmonic_batch_download(s.h, 0, 0, v, v)),
                         ("solve", s.L.ec3d_harmonic_batch_solve(s.h, 1e-3, 10, None)),
                         ("get", s.L.ec3d_get_harmonic_batch(s.h, 0, C.byref(info))),
                         ("select", s.L.ec3d_harmonic_batch_select(s.h, 0)),
                         ("device_vector", s.L.ec3d_harmonic_batch_device_vector(s.h, 0, 0, C.byref(p), C.byref(m)))):
            assert rc == 2, f"{name} before a batch set-up"
        with pytest.raises(E.EC3DError, match="ec3d_harmonic_batch_setup first"):
            s.harmonic_batch_solve(1e-3, 10)
        # a batch of two that every refusal below has to leave as it was
        b = _rhs(g)
        s.harmonic_batch_setup([_w(50.0), _w(500.0)])
        s.harmonic_batch_upload(0, "B", b)
        s.harmonic_batch_upload(1, "X", b)
        two = np.array([_w(50.0), _w(60.0)])
        assert s.L.ec3d_harmonic_batch_setup(s.h, 17, two.ctypes.data) == 2
        assert s.L.ec3d_harmonic_batch_setup(s.h, -1, two.ctypes.data) == 2
        assert s.L.ec3d_harmonic_batch_setup(s.h, 2, None) == 2
        for bad in (float("nan"), float("inf"), -1.0):
            w = np.array([_w(50.0), bad])
            assert s.L.ec3d_harmonic_batch_setup(s.h, 2, w.ctypes.data) == 2
            with pytest.raises(E.EC3DError) as e:
                s.harmonic_batch_setup([bad])
            assert e.value.status == 2
        for sys in (-1, 2, 16):
            assert s.L.ec3d_harmonic_batch_upload(s.h, sys, 0, v.ctypes.data, v.ctypes.data) == 2
            assert s.L.ec3d_harmonic_batch_download(s.h, sys, 0, v, v) == 2
            assert s.L.ec3d_get_harmonic_batch(s.h, sys, C.byref(info)) == 2
            assert s.L.ec3d_harmonic_batch_select(s.h, sys) == 2
            assert s.L.ec3d_harmonic_batch_device_vector(s.h, sys, 0, C.byref(p), C.byref(m)) == 2
        assert s.L.ec3d_harmonic_batch_upload(s.h, 0, 0, None, None) == 2
        assert s.L.ec3d_harmonic_batch_upload(s.h, 0, 2, v.ctypes.data, None) == 2          # R is no argument
        assert s.L.ec3d_harmonic_batch_device_vector(s.h, 0, 8, C.byref(p), C.byref(m)) == 2
        assert s.L.ec3d_get_harmonic_batch(s.h, 0, None) == 2 and s.L.ec3d_harmonic_batch_setup(None, 1, two.ctypes.data) == 2
        # the null projection belongs to one omega: refused, never ignored
        s.harmonic_setup(_w(50.0))
        s.harmonic_set_null_projection(True)
        with pytest.raises(E.EC3DError, match="ec3d_harmonic_set_null_projection is on") as e:
            s.harmonic_batch_solve(1e-3, 10)
        assert e.value.status == 2
        s.harmonic_set_null_projection(False)
        assert [s.harmonic_batch_info(k)["omega"] for k in (0, 1)] == [_w(50.0), _w(500.0)]
        _same(s.harmonic_batch_download(0, "B"), b, "B^ of system 0 through the refusals")
        _same(s.harmonic_batch_download(1, "X"), b, "X^ of system 1 through the refusals")
        assert not s.harmonic_batch_download(0, "X").any()
        assert len(s.harmonic_batch_solve(1e-3, 3)) == 2
    z = load_golden("g8b_stacked_moving_20x16x14")                        # a z-slab: planes [0, 9), owned [0, 7)
    geo = z["geoPHYS"][:9].copy()
    geoC = np.zeros(geo.shape, np.int32)
    q = np.concatenate([np.flatnonzero((geo.reshape(-1) == d) & (z["geoPHYS_C"][:9].reshape(-1) != 0)) for d in (1, 2)])
    geoC.reshape(-1)[q] = 3 * geo.size + 1 + np.arange(len(q))
    with E.EC3DSolver() as s:
        s.assemble_slab(z["geoPHYS"].shape[0], 0, 9, 0, 7, geo, geoC, z["valPHYS"], z["BND"], z["delta"], float(z["dt"]))
        assert [rc for _, rc in _batch_calls(s)] == [5] * 7


def test_run_harmonic_sweep_and_the_command_line(E, tmp_path, capsys):
    """host.run_harmonic_sweep on the shipped compare_to_Elmer model and the same through --harmonic F0 --sweep."""
    import os
    from conftest import GOLDEN
    from eddy_currents_3d_amd import host, run, vxc
    path = os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc")
    model = vxc.read_vxc(path)
    t = vxc.domain_tables(model)
    freqs = [25.0, 50.0, 100.0]
    with E.EC3DSolver() as s:
        rs = host.run_harmonic_sweep(model, s, 50.0, freqs, integrals=True)
    with E.EC3DSolver() as s2:
        r = host.run_harmonic(model, s2, 50.0, integrals=True)
    assert [q["freq"] for q in rs] == freqs and set(r) - {"info"} <= set(rs[1])
    for q in rs:
        print(f"{q['freq']:g} Hz: iter {q['iter']}, relres {q['relres']:.3e}, true residual {q['true_residual']:.3e}, joule [W] "
              f"{[d['joule_w'] for d in q['integrals']]}")
        assert q["iter"] <= t["itmax"] and q["relres"] < t["tol"] and q["true_residual"] <= 10 * t["tol"]
    at50 = rs[1]
    assert at50["iter"] == r["iter"] and at50["relres"] == r["relres"]
    _same(at50["x"], r["x"], "x^ at 50 Hz: the sweep against run_harmonic")
    assert len(at50["integrals"]) == len(r["integrals"]) > 0
    for a, c in zip(at50["integrals"], r["integrals"]):
        assert a["domain"] == c["domain"] and a["joule_w"] == c["joule_w"] > 0.0 and np.array_equal(a["force_n"], c["force_n"])
    assert rs[0]["integrals"][0]["joule_w"] != rs[2]["integrals"][0]["joule_w"]
    capsys.readouterr()
    csv = tmp_path / "sweep.csv"
    out = tmp_path / "cli"
    assert run.main([path, "--harmonic", "50", "--sweep", "25,50,100", "--sweep-batch", "2", "--out", str(out),
                     "--integrals", str(csv)]) == 0
    text = capsys.readouterr().out
    assert text.count("harmonic sweep ") == 3 and f"iter={r['iter']} " in text
    lines = csv.read_text().splitlines()
    assert lines[0] == run.HARMONIC_INTEGRALS_HEADER and len(lines) == 1 + 3 * len(r["integrals"])
    assert [float(l.split(",")[0]) for l in lines[1:]] == [f for f in freqs for _ in r["integrals"]]
    nd = len(r["integrals"])
    assert float(lines[1 + nd].split(",")[3]) == r["integrals"][0]["joule_w"]
    assert sorted(os.listdir(out)) == sorted(f"harmonic_{k}_{p}.vtk" for k in range(3) for p in ("re", "im"))
