"""The time-harmonic A-V solve on the device (ec3d_harmonic_*; csrc/ec3d_harmonic.hip) against
its numpy twin (tests/harmonic_numpy.py).

* harmonic_spmv == the twin's ordered complex row product BIT FOR BIT on g2, g2v (advection in re), g8a (two domains, 73
  classes), g9b (every one-sided U pattern), g3 with padded planes and a generated 96 x 96 x 64 box with a plate (more than
  1024 chunks: the kernels' stride loops make several trips), for random complex x and for a resident x^ whose rows of
  no unknown hold NaN;
* whole iterations: harmonic_solve(tol = 0, itmax = k), k = 1, 2, 5, 20 on g2 and g8a and k = 3 on the box: X^, iter and
  the restart count equal the twin's bit for bit; the same with a tol at which the twin restarts within 20 iterations;
* convergence on g2, g8a, g9b at the fixture's own tol with b^ = the fixture's first right-hand side (Jaf of the step from
  x = 0: the sources alone, a real phasor) at 50 Hz: relres < tol, harmonic_true_residual == the twin's residual of the
  downloaded x^ to 1e-12 ||b^||, and <= 10 tol;
* g1 (no conductor): the solve of (1 + 2j) b is (1 + 2j) times the real solve within 2 cond(A) tol;
* harmonic_load: X and B of either part equal the twin's, their float32 fields are ec3d_vtk_fields bit for bit, and
  domain_integrals of the part equals the twin's;
* refusals; the memory contract: the real vectors keep their bytes through a harmonic solve, and the transient solve that
  follows gives the bits it gives on a handle that never ran one."""
import numpy as np
import pytest

import av_generate as AG
import domain_integrals_numpy as DI
import fields_numpy as FN
import guard_zones as Z
import harmonic_numpy as HN
from conftest import load_golden
from eddy_currents_3d_amd.solver import NULL_E_MATRIX

pytestmark = pytest.mark.gpu
OMEGA = 2.0 * np.pi * 50.0
G2, G2V, G3 = "g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14", "g3_moving_coil_18x16x12"
G8A, G9B = "g8a_two_plates_18x16x16", "g9b_L_hole_near_faces_17x16x16"
S_EXIT_TOL = {G2: 0.02, G8A: 0.2}
SPMV_CASES = [(G2, False), (G2V, False), (G8A, False), (G9B, False), (G3, True)]


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _assemble(s, g, omega=OMEGA):
    s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
    s.harmonic_setup(omega)


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


_BOX = {}


def box():
    """96 x 96 x 64 cells with a conducting plate in the middle: 4 * 64 * 9216 device rows = 4608 chunks."""
    if not _BOX:
        geo, geoC, val, bnd, delta, dt = AG.from_boxes(
            (96, 96, 64), [dict(boxes=[((30, 66), (28, 70), (29, 35))], C=44.3, vel=(0.0, 0.0, 0.0))],
            [[-0.95, -0.95], [-0.95, -0.95], [-0.95, -0.95]], (0.004, 0.005, 0.003), 1e-3)
        g = dict(geoPHYS=geo, geoPHYS_C=geoC, valPHYS=val, BND=bnd, delta=delta, dt=dt)
        _BOX.update(g=g, op=HN.Operator(g, OMEGA))
    return _BOX["g"], _BOX["op"]


def _poison_rows_of_no_unknown(s, x):
    """Upload x as X^ and put NaN into every pair of the device vector that holds no unknown (the padding between planes,
    the empty U slots, the rows [n, n_pad)); returns how many."""
    s.harmonic_upload("X", x)
    ptr, n_pad = s.harmonic_device_vector("X")
    s.synchronize()
    v = Z.peek(ptr, 2 * n_pad).view(np.float64).reshape(n_pad, 2).copy()
    hidden = np.setdiff1d(np.arange(n_pad), s.row_map())
    assert not v[hidden].any()
    v[hidden] = np.nan
    Z.poke(ptr, v.reshape(-1))
    return len(hidden)


@pytest.mark.parametrize("name,pitched", SPMV_CASES, ids=[f"{n.split('_')[0]}{'-pitched' if p else ''}" for n, p in SPMV_CASES])
def test_spmv_equals_the_twin_bit_for_bit(E, monkeypatch, name, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    g = load_golden(name)
    op = HN.Operator(g, OMEGA)
    sdz, sdy, sdx = g["geoPHYS"].shape
    with E.EC3DSolver() as s:
        _assemble(s, g)
        assert s.info.tail_rows == 0 and s.info.dict_classes == op.ids["ncls"]
        rm = s.row_map()
        assert (rm[sdx * sdy] - rm[0] > sdx * sdy) == pitched
        for seed in (1, 2):
            x = _random_complex(op.n, seed)
            _same(s.harmonic_spmv(x), op(HN.split(x)), f"{name} seed {seed}")
        x = _random_complex(op.n, 3)
        assert _poison_rows_of_no_unknown(s, x) > 0
        y = s.harmonic_spmv(None)
        assert np.all(np.isfinite(y.real)) and np.all(np.isfinite(y.imag))
        _same(y, op(HN.split(x)), f"{name} NaN in the rows of no unknown")
        _same(s.harmonic_download("X"), x, "X^ as uploaded")
        # a real x and omega = 0: the imaginary table is zero, the product is real
        s.harmonic_setup(0.0)
        y0 = s.harmonic_spmv(x.real)
        assert not y0.imag.any()
        _same(y0, HN.Operator(g, 0.0)(HN.split(x.real)), f"{name} omega = 0")


def test_spmv_on_a_box_of_more_than_1024_chunks(E):
    g, op = box()
    with E.EC3DSolver() as s:
        _assemble(s, g)
        assert s.vector_layout()["n_pad"] // 512 > 1024
        x = _random_complex(op.n, 5)
        _same(s.harmonic_spmv(x), op(HN.split(x)), "box")
        _poison_rows_of_no_unknown(s, x)
        _same(s.harmonic_spmv(None), op(HN.split(x)), "box, NaN in the rows of no unknown")


def _rhs(g, n):
    """a complex right-hand side with both parts alive: two captured steps' Jaf"""
    return g["b0"] + 1j * g["b1"]


@pytest.mark.parametrize("name", [G2, G8A])
def test_whole_iterations_equal_the_twin_bit_for_bit(E, name):
    g = load_golden(name)
    op = HN.Operator(g, OMEGA)
    n = op.n
    b, x0 = _rhs(g, n), 1e-3 * _random_complex(n, 7)
    with E.EC3DSolver() as s:
        _assemble(s, g)
        sums = _sums(s)
        trace = []
        HN.bicgstab(op, sums, HN.split(b), HN.split(x0), 0.0, 20, trace=trace)
        assert [t[0] for t in trace] == list(range(1, 22))
        s.harmonic_upload("B", b)
        for k in (1, 2, 5, 20):
            s.harmonic_upload("X", x0)
            it, relres = s.harmonic_solve(0.0, k)
            info = s.harmonic_info()
            assert it == k + 1 == info["iter"] and info["stop_kind"] == 0
            _same(s.harmonic_download("X"), trace[k][1], f"{name} itmax = {k}")
            assert info["restarts"] == trace[k][2]
        # tolerances at which the twin, from x^ = 0, restarts within 20 iterations and takes no exit (1e-3), restarts and
        # takes the ||R|| exit (1e-2), and takes the ||S|| exit (S_EXIT_TOL): found with the twin, asserted of the twin
        zero = np.zeros(n)
        for tol, kind in ((1e-3, 0), (1e-2, 2), (S_EXIT_TOL[name], 1)):
            xt, it_t, rs_t, rel_t, kind_t = HN.bicgstab(op, sums, HN.split(b), HN.split(zero), tol, 20)
            assert kind_t == kind and (rs_t >= 1 or kind == 1) and (it_t <= 20) == (kind != 0), "not the case it is meant to be"
            s.harmonic_upload("X", zero)
            it, relres = s.harmonic_solve(tol, 20)
            info = s.harmonic_info()
            print(f"{name}: tol {tol}: iter {it}, restarts {info['restarts']}, exit {info['stop_kind']} (twin {it_t}, {rs_t}, {kind_t})")
            assert (it, info["restarts"], info["stop_kind"]) == (it_t, rs_t, kind_t)
            _same(s.harmonic_download("X"), xt, f"{name} with restarts, tol {tol}")
            assert relres == rel_t


def test_three_iterations_on_the_box(E):
    g, op = box()
    rng = np.random.default_rng(11)
    b = np.zeros(op.n, np.complex128)
    coil = np.flatnonzero(np.asarray(g["geoPHYS_C"]).reshape(-1) == 0)[::97][:4000]     # a scattered source on Ax, Ay
    b[coil] = rng.standard_normal(len(coil)) + 1j * rng.standard_normal(len(coil))
    b[op.nC + coil] = rng.standard_normal(len(coil))
    with E.EC3DSolver() as s:
        _assemble(s, g)
        xt, it_t, rs_t, _, _ = HN.bicgstab(op, _sums(s), HN.split(b), HN.split(np.zeros(op.n)), 0.0, 3)
        s.harmonic_upload("B", b)
        s.harmonic_upload("X", np.zeros(op.n))
        it, _ = s.harmonic_solve(0.0, 3)
        assert (it, s.harmonic_info()["restarts"]) == (it_t, rs_t) == (4, rs_t)
        _same(s.harmonic_download("X"), xt, "box, itmax = 3")


@pytest.fixture(scope="module")
def converged(E):
    """Per fixture: the solve at the fixture's own tolerance, what it reported, x^ and b^, and the loaded parts."""
    out = {}
    for name in (G2, G8A, G9B):
        g = load_golden(name)
        op = HN.Operator(g, OMEGA)
        tol, itmax = float(g["tol"]), int(g["itmax"])
        b = g["b0"].astype(np.complex128)
        with E.EC3DSolver() as s:
            _assemble(s, g)
            s.harmonic_upload("B", b)
            s.harmonic_upload("X", np.zeros(op.n))
            it, relres = s.harmonic_solve(tol, itmax)
            true, bnorm = s.harmonic_true_residual()
            x = s.harmonic_download("X")
            parts = []
            for part in (0, 1):
                s.harmonic_load(part)
                parts.append(dict(X=s.download("X"), B=s.download("B"),
                                  vtk=s.vtk_fields(g["delta"], g["geoPHYS"].size, True),
                                  integrals=s.domain_integrals(g["delta"])))
            out[name] = dict(g=g, op=op, tol=tol, itmax=itmax, b=b, it=it, relres=relres, true=true, bnorm=bnorm, x=x,
                             parts=parts, cel_bnd=s.cel_bnd(), info=s.harmonic_info())
    return out


@pytest.mark.parametrize("name", [G2, G8A, G9B])
def test_convergence_at_the_fixtures_tolerance(converged, name):
    c = converged[name]
    op, b, x, tol = c["op"], c["b"], c["x"], c["tol"]
    ax = op(HN.split(x))
    r = b.real - ax[0], b.imag - ax[1]
    twin_true = np.sqrt(np.sum(r[0] * r[0] + r[1] * r[1])) / np.linalg.norm(b)
    print(f"{name}: iter {c['it']} (itmax {c['itmax']}), restarts {c['info']['restarts']}, relres {c['relres']:.3e}, true residual "
          f"{c['true']:.3e} (twin {twin_true:.3e}), tol {tol:g}, {c['info']['ms']:.1f} ms")
    assert c["it"] <= c["itmax"] and c["relres"] < tol
    assert abs(c["bnorm"] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    assert abs(c["true"] - twin_true) <= 1e-12
    assert c["true"] <= 10 * tol


def test_g1_on_the_device(E, oracle):
    g = load_golden("g1_nonconducting_8x7x6")
    op = HN.Operator(g, OMEGA)
    n, tol, itmax = op.n, float(g["tol"]), int(g["itmax"])
    A = op.dense()
    assert not A.imag.any()
    cond = np.linalg.cond(A.real)
    z, b = 1.0 + 2.0j, g["b0"]
    xre, it_re = oracle.bicgstab_wr(g["valA"], g["irow"], g["jcol"], b, np.zeros(n), tol, itmax)[:2]
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.harmonic_upload("B", z * b)
        s.harmonic_upload("X", np.zeros(n))
        it, relres = s.harmonic_solve(tol, itmax)
        x = s.harmonic_download("X")
        xt, it_t, _, _, _ = HN.bicgstab(op, _sums(s), HN.split(z * b), HN.split(np.zeros(n)), tol, itmax)
    err = np.linalg.norm(x - z * xre) / np.linalg.norm(z * xre)
    print(f"g1: cond(A) = {cond:.3e}, iter {it} (real solve {it_re}), |x^ - (1 + 2j) x| / |x| = {err:.3e}, bar {2 * cond * tol:.3e}")
    assert it <= itmax and it_re <= itmax and relres < tol
    assert err <= 2.0 * cond * tol
    assert it == it_t
    _same(x, xt, "g1")


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("name", [G2, G8A])
def test_harmonic_load(converged, name, part):
    c = converged[name]
    g, op, got = c["g"], c["op"], c["parts"][part]
    X, B = HN.load_part(op, g, c["cel_bnd"], HN.split(c["x"]), HN.split(c["b"]), part)
    assert np.array_equal(got["X"].view(np.uint64), X.view(np.uint64))
    assert np.array_equal(got["B"].view(np.uint64), B.view(np.uint64))
    nC = op.nC
    cond = np.flatnonzero(np.asarray(g["geoPHYS_C"]).reshape(-1) != 0)
    if part == 1:
        assert np.any(B[cond] != 0.0)                  # omega C Re A^ in the conductor: the eddy current's Im part
    want = FN.fields(g["geoPHYS_C"], g["delta"], got["X"], got["B"])
    for k in ("A", "eddy", "source", "B"):
        assert np.array_equal(got["vtk"][k], want[k]), k
    twin = DI.integrals(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["delta"], X, B)
    assert [r["domain"] for r in got["integrals"]] == [w["domain"] for w in twin]
    for r, w in zip(got["integrals"], twin):
        g4 = np.concatenate([[r["joule_w"]], r["force_n"]])
        w4 = np.concatenate([[w["joule_w"]], w["force_n"]])
        assert np.all(np.abs(g4 - w4) <= 1e-12 * w["abs"]), (name, part, r["domain"])
    if part == 0 and name == G2:
        # the real right-hand side drives Im A^ < Re A^ but both are alive at 50 Hz in copper
        assert np.linalg.norm(c["x"].imag) > 1e-3 * np.linalg.norm(c["x"].real)


def test_refusals(E):
    g = load_golden(G2)
    with E.EC3DSolver() as s:
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_setup(OMEGA)                                       # no matrix
        assert e.value.status == 3
        s.assemble_poisson(8, 8, 8)
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_setup(OMEGA)
        assert e.value.status == 3
        s.set_matrix_csr(g["valA"], g["irow"], g["jcol"])
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_setup(OMEGA)
        assert e.value.status == 3
        c = load_golden("g8c_side_by_side_20x18x14")                      # bands + tail
        s.assemble(c["geoPHYS"], c["geoPHYS_C"], c["valPHYS"], c["BND"], c["delta"], float(c["dt"]))
        assert s.info.tail_rows > 0
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_setup(OMEGA)
        assert e.value.status == NULL_E_MATRIX
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        for call in (lambda: s.harmonic_solve(1e-3, 10), lambda: s.harmonic_upload("X", np.zeros(s.n)),
                     lambda: s.harmonic_load(0), lambda: s.harmonic_true_residual(), lambda: s.harmonic_spmv(np.zeros(s.n))):
            with pytest.raises(E.EC3DError, match="ec3d_harmonic_setup first") as e:
                call()
            assert e.value.status == 2
        for bad in (float("nan"), float("inf"), -1.0):
            with pytest.raises(E.EC3DError) as e:
                s.harmonic_setup(bad)
            assert e.value.status == 2
        assert not s.harmonic_info()["ready"]
        s.harmonic_setup(OMEGA)
        assert s.harmonic_info()["ready"] and s.harmonic_info()["omega"] == OMEGA
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_load(2)
        assert e.value.status == 2
        assert s.L.ec3d_harmonic_download(s.h, 0, np.zeros(s.n), np.zeros(s.n)) == 0
        assert s.L.ec3d_harmonic_upload(s.h, 0, None, None) == 2
        assert s.L.ec3d_harmonic_upload(s.h, 2, np.zeros(s.n).ctypes.data, None) == 2      # R is no argument
        assert s.L.ec3d_get_harmonic(s.h, None) == 2 and s.L.ec3d_harmonic_setup(None, OMEGA) == 2
        # a new assembly clears the set-up
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        assert not s.harmonic_info()["ready"]
    b = load_golden("g8b_stacked_moving_20x16x14")                        # a z-slab: planes [0, 9), owned [0, 7)
    geo = b["geoPHYS"][:9].copy()
    geoC = np.zeros(geo.shape, np.int32)
    q = np.concatenate([np.flatnonzero((geo.reshape(-1) == d) & (b["geoPHYS_C"][:9].reshape(-1) != 0)) for d in (1, 2)])
    geoC.reshape(-1)[q] = 3 * geo.size + 1 + np.arange(len(q))
    with E.EC3DSolver() as s:
        s.assemble_slab(b["geoPHYS"].shape[0], 0, 9, 0, 7, geo, geoC, b["valPHYS"], b["BND"], b["delta"], float(b["dt"]))
        with pytest.raises(E.EC3DError) as e:
            s.harmonic_setup(OMEGA)
        assert e.value.status == 5


def test_memory_contract_and_the_transient_solve_afterwards(E):
    g = load_golden(G2)
    tol, itmax = float(g["tol"]), int(g["itmax"])
    with E.EC3DSolver() as s:
        s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        s.upload("B", g["b1"])
        s.upload("X", g["xin1"])
        it0, _ = s.solve_resident(tol, itmax)           # the work vectors hold a solve's leftovers
        x_first = s.download("X")
        s.upload("X", g["xin1"])
        base, before = Z.owned_block(s)
        rings_before = Z.rings(s)
        s.harmonic_setup(OMEGA)
        s.harmonic_upload("B", g["b0"] + 1j * g["b1"])
        s.harmonic_upload("X", np.zeros(s.n))
        it_h, _ = s.harmonic_solve(tol, itmax)
        s.harmonic_true_residual()
        s.harmonic_spmv(_random_complex(s.n, 1))
        assert 0 < it_h <= itmax
        base2, after = Z.owned_block(s)
        assert base2 == base and np.array_equal(before, after), "a real vector changed under the harmonic solve"
        for k, v in Z.rings(s).items():
            assert np.array_equal(v, rings_before[k]), k
        it1, _ = s.solve_resident(tol, itmax)
        x_after = s.download("X")
        # harmonic_load is the one call that writes X and B
        s.harmonic_load(0)
        assert not np.array_equal(s.download("B"), g["b1"])
    assert it1 == it0 and 0 < it0 <= itmax
    assert np.array_equal(x_after.view(np.uint64), x_first.view(np.uint64))


def test_run_harmonic_and_the_command_line(E, tmp_path, capsys):
    """host.run_harmonic on the shipped compare_to_Elmer model (TEAM 7 at 50 Hz) and the same through --harmonic."""
    import os
    from conftest import GOLDEN
    from eddy_currents_3d_amd import host, probes as P, run, vxc
    from test_vtk_output import parse_vectors
    path = os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc")
    model = vxc.read_vxc(path)
    t = vxc.domain_tables(model)
    sdz, sdy, sdx = model.vox.shape
    cells = P.probe_line((10, 51, 12), (90, 51, 12), (sdx, sdy, sdz))
    with E.EC3DSolver() as s:
        r = host.run_harmonic(model, s, 50.0, out_dir=str(tmp_path / "h"), integrals=True, probes=cells)
        print(f"compare_to_Elmer at 50 Hz: iter {r['iter']}, relres {r['relres']:.3e}, true residual {r['true_residual']:.3e}, "
              f"{r['info']['ms']:.1f} ms; joule [W] {[q['joule_w'] for q in r['integrals']]}")
        assert r["iter"] <= t["itmax"] and r["relres"] < t["tol"] and r["true_residual"] <= 10 * t["tol"]
        assert r["x"].shape == (3 * model.vox.size + t["ncells0"],) and np.any(r["x"].imag != 0.0)
        # part 1 is still loaded: the resident real X is Im x^ but for the cel_bnd zeros
        X = s.download("X")
        keep = np.ones(len(X), bool)
        for lst in s.cel_bnd()[:3]:
            keep[np.asarray(lst, np.int64) - 1] = False
        assert np.array_equal(X[keep], r["x"].imag[keep])
    assert r["probes"].shape == (len(cells), 13) and r["probes"].dtype == np.complex128
    assert np.array_equal(r["probes"].real, r["parts"][0]["probes"]) and np.array_equal(r["probes"].imag, r["parts"][1]["probes"])
    for q, a, c in zip(r["integrals"], r["parts"][0]["integrals"], r["parts"][1]["integrals"]):
        assert q["joule_w"] == 0.5 * (a["joule_w"] + c["joule_w"]) > 0.0
        assert np.array_equal(q["force_n"], 0.5 * (a["force_n"] + c["force_n"]))
    # the files hold the float32 fields of the two parts: A of harmonic_re.vtk is float32(Re A^) where nothing was zeroed
    nC = model.vox.size
    for part, name in enumerate(("re", "im")):
        f = parse_vectors((tmp_path / "h" / f"harmonic_{name}.vtk").read_bytes(), nC)
        A = np.stack([(r["x"].real, r["x"].imag)[part][d * nC:(d + 1) * nC] for d in range(3)], axis=1).astype(np.float32)
        same = f["Field_A"] == A            # (cel_bndX/Y/Z zeroes single components)
        assert same.mean() > 0.9 and np.all(f["Field_A"][~same] == 0.0)
        assert set(f) == {"_points", "Field_A", "Vector_field_eddy", "Vector_field_SOURCE", "Vector_field_B"}
    capsys.readouterr()
    csv = tmp_path / "avg.csv"
    assert run.main([path, "--harmonic", "50", "--out", str(tmp_path / "cli"), "--integrals", str(csv)]) == 0
    out = capsys.readouterr().out
    assert f"iter={r['iter']} " in out and "harmonic_re.vtk" in out
    assert (tmp_path / "cli" / "harmonic_re.vtk").read_bytes() == (tmp_path / "h" / "harmonic_re.vtk").read_bytes()
    assert (tmp_path / "cli" / "harmonic_im.vtk").read_bytes() == (tmp_path / "h" / "harmonic_im.vtk").read_bytes()
    lines = csv.read_text().splitlines()
    assert lines[0] == run.HARMONIC_INTEGRALS_HEADER and len(lines) == 1 + len(r["integrals"])
    assert float(lines[1].split(",")[3]) == r["integrals"][0]["joule_w"]
    with pytest.raises(SystemExit):
        run.main([os.path.join(GOLDEN, "g4_ec_src_move_hole.vxc"), "--harmonic", "50", "--no-output"])
