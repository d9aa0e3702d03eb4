"""ec3d_set_probes .. ec3d_get_probes on the device: the resident fields at chosen cells -- bit for bit against the twin
(tests/probes_numpy.py: the expressions of the float32 field twin without the rounding) in both storage forms and with
pitched planes, against the float32 field output of the same state, the record that stays on the device, what the calls
leave alone, what they refuse, more probes than one launch has threads, and in the time loop.

The twin reads X and B as EC3DSolver.download returns them (the reference's numbering), so a state reached by a solve is
downloaded from the structured handle and uploaded to the bands + tail handle: both then hold the same X and B and have
to return the same bits."""
import numpy as np
import pytest

import guard_zones as Z
import probes_numpy as PN
from conftest import load_golden
from test_gpu_domain_integrals import g3_model
from test_gpu_field_integrals import CAPTURED, args_of, case, status_of
from test_gpu_timeloop import coil_sources

pytestmark = pytest.mark.gpu

KEYS = ["g1", "g2", "g3", "g8a", "S3"]
PITCHED = {"g1": (False, True), "g2": (False, True), "g3": (False, True), "g8a": (False, True), "S3": (True,)}
REPEATS = 37
MAX_WGS = 1024      # EC3D_PROBE_MAX_WGS of csrc/ec3d_probes.hip: a launch has min(ceil(nprobes / 256), 1024) workgroups


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def shuffled_box(ncells, seed):
    """Every cell of the box in a fixed shuffled order, followed by 37 repeats: every face, edge and corner goes through
    the clamping, duplicates are present, and the length is no multiple of 256."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cells = np.concatenate([rng.permutation(ncells), rng.integers(0, ncells, REPEATS)]).astype(np.int64)
    assert len(cells) % 256 != 0
    return cells


def flat(d):
    """probe_sample's dict as the (nprobes, 13) array of the twin."""
    from eddy_currents_3d_amd.probes import stack
    return stack(d)


def set_pitch(monkeypatch, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    else:
        monkeypatch.delenv("EC3D_PITCH", raising=False)


# --------------------------------------------------------------------------------------------- 1. the twin, both forms
@pytest.mark.parametrize("key,pitched", [(k, p) for k in KEYS for p in PITCHED[k]])
def test_bits_equal_the_twin_in_both_forms(E, monkeypatch, key, pitched):
    set_pitch(monkeypatch, pitched)
    args, prepare = case(key)
    geo, geoC, delta = args[0], args[1], args[4]
    plane = geo.shape[1] * geo.shape[2]
    cells = shuffled_box(geo.size, 60 + KEYS.index(key))
    if key == "g2":
        assert len(cells) == 3397 and (len(cells) + 255) // 256 == 14
    with E.EC3DSolver(structured=True) as s:
        s.assemble(*args)
        assert s.info.tail_rows == 0
        if np.count_nonzero(geoC):
            pi = Z.pitch_info(s, plane)
            assert pi["pitch"] == ((plane + 511) // 512 * 512 if pitched else plane)
            if key == "S3":
                assert pi["pitch"] == 1536 and pi["plane"] == 1200
        prepare(s)
        x, b = s.download("X"), s.download("B")
        s.set_probes(cells)
        assert s.probes() == dict(nprobes=len(cells), capacity=0, recorded=0, device_bytes=(8 + 104) * len(cells))
        d = s.probe_sample(delta)
        assert [(k, v.shape, v.dtype) for k, v in d.items()] == \
            [(k, (len(cells), 3), np.float64) for k in ("a", "eddy", "source", "b")] + [("u", (len(cells),), np.float64)]
        got = flat(d)
        assert flat(s.probe_sample(delta)).tobytes() == got.tobytes()
    want = PN.sample(geoC, delta, x, b, cells)
    diff = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    print(f"{key} pitched={pitched}: {len(cells)} probes, {len(diff)} differ from the twin"
          + (f", first probe {diff[0]} (cell {cells[diff[0]]}): {got[diff[0]]!r} / {want[diff[0]]!r}" if len(diff) else ""))
    assert np.isfinite(got).all() and got[:, 9:12].any()
    assert got.tobytes() == want.tobytes()
    if key == "g1":
        assert not np.count_nonzero(geoC) and got[:, 3:6].tobytes() == bytes(24 * len(cells)) and not got[:, 12].any()
    else:
        assert got[:, 12].any() and got[:, 3:6].any()
    with E.EC3DSolver(structured=False) as s:
        s.assemble(*args)
        assert s.info.tail_rows > 0 or not np.count_nonzero(geoC)
        s.upload("X", x)
        s.upload("B", b)
        s.set_probes(cells)
        assert flat(s.probe_sample(delta)).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ 2. against the fields
@pytest.mark.parametrize("key", KEYS)
def test_float32_of_the_sample_is_the_field_output(E, monkeypatch, key):
    set_pitch(monkeypatch, PITCHED[key][-1])
    args, prepare = case(key)
    geoC, delta = args[1], args[4]
    N = geoC.size
    conducting = bool(np.count_nonzero(geoC))
    cells = shuffled_box(N, 80 + KEYS.index(key))
    with E.EC3DSolver() as s:
        s.assemble(*args)
        prepare(s)
        s.set_probes(cells)
        got = flat(s.probe_sample(delta))
        f = s.vtk_fields(delta, N, conducting)        # g1: field_eddy is NULL
        x = s.download("X")
    assert (f["eddy"] is None) == (key == "g1")
    for name, at in (("A", 0), ("eddy", 3), ("source", 6), ("B", 9)):
        want = f[name][cells] if f[name] is not None else np.zeros((len(cells), 3), np.float32)
        assert got[:, at:at + 3].astype(np.float32).tobytes() == want.tobytes(), name
    uid = geoC.reshape(-1)[cells].astype(np.int64)       # the reference's 1-based U number of a conductor cell
    want_u = np.where(uid != 0, x[np.maximum(uid, 1) - 1], 0.0)
    assert got[:, 12].tobytes() == want_u.tobytes()


# ------------------------------------------------------------------------------------------------------- 3. the record
def test_the_record_keeps_every_step_and_refuses_when_full(E):
    g = load_golden(CAPTURED["g3"][0])
    args = args_of(g)
    delta = args[4]
    n = len(g["irow"]) - 1
    cells = shuffled_box(g["geoPHYS"].size, 7)[:700]
    T = [0.0, 0.001, 0.002, 0.003]
    with E.EC3DSolver() as s:
        s.assemble(*args)
        s.upload("X", np.zeros(n))
        s.upload("B", np.zeros(n))
        s.set_probes(cells, capacity=3)
        assert s.probes() == dict(nprobes=700, capacity=3, recorded=0, device_bytes=700 * (8 + 104 * 4))
        direct = []
        for k in range(4):
            idx, val = coil_sources(g, k, True)
            s.rhs_step(idx, val, moving=True)
            s.solve_resident(float(g["tol"]), int(g["itmax"]))
            s.post_update()
            if k < 3:
                s.probe_record(delta, T[k])
                assert s.probes()["recorded"] == k + 1
            else:
                assert status_of(E, lambda: s.probe_record(delta, T[k])) == E.solver.PROBE_E_FULL == 24
                assert s.probes()["recorded"] == 3
            direct.append(flat(s.probe_sample(delta)))
        assert direct[0].tobytes() != direct[1].tobytes() != direct[2].tobytes()       # the coil moves
        Tr, rec = s.probe_read()
        assert Tr.tobytes() == np.array(T[:3]).tobytes()
        assert rec["a"].shape == (3, 700, 3) and rec["u"].shape == (3, 700)
        assert flat(rec).tobytes() == np.stack(direct[:3]).tobytes()          # the refused fourth changed no byte
        Tm, mid = s.probe_read(1, 2)
        assert Tm.tolist() == T[1:3] and flat(mid).tobytes() == np.stack(direct[1:3]).tobytes()
        T0, none = s.probe_read(3)
        assert len(T0) == 0 and none["a"].shape == (0, 700, 3)
        assert status_of(E, lambda: s.probe_read(2, 2)) == 2 and status_of(E, lambda: s.probe_read(4, 0)) == 2
        assert status_of(E, lambda: s.probe_read(-1, 1)) == 2
        s.probe_reset()
        assert s.probes()["recorded"] == 0 and status_of(E, lambda: s.probe_read(0, 1)) == 2
        s.probe_record(delta, 7.5)                                           # number 0 again: the state of step 3
        T1, one = s.probe_read()
        assert T1.tolist() == [7.5] and flat(one).tobytes() == direct[3][None].tobytes()
        s.set_probes(cells[:5])                                              # capacity 0: sampling only
        assert s.probes() == dict(nprobes=5, capacity=0, recorded=0, device_bytes=5 * (8 + 104))
        assert status_of(E, lambda: s.probe_record(delta, 0.0)) == 24
        assert flat(s.probe_sample(delta)).tobytes() == direct[3][:5].tobytes()
        s.set_probes([])
        assert s.probes() == dict(nprobes=0, capacity=0, recorded=0, device_bytes=0)
        assert status_of(E, lambda: s.probe_sample(delta)) == 2


# ------------------------------------------------------------------------------------- 4. what the calls leave alone
@pytest.mark.parametrize("pitched", [False, True])
def test_the_calls_change_no_vector_and_no_canary(E, monkeypatch, pitched):
    set_pitch(monkeypatch, pitched)
    g = load_golden(CAPTURED["g3"][0])
    args = args_of(g)
    delta = args[4]
    sdz, sdy, sdx = g["geoPHYS"].shape
    cells = shuffled_box(g["geoPHYS"].size, 11)
    want = PN.sample(args[1], delta, g["xout0"], g["b0"], cells)
    with Z.adopted(E, lambda s: s.assemble(*args)) as a:
        s = a.s
        z = Z.zones(s.vector_layout(), Z.pitch_info(s, sdx * sdy))
        s.upload("B", g["b0"])
        s.upload("X", g["xout0"])
        _, before, _ = a.read()
        before = before.copy()
        assert s.download("X").tobytes() == g["xout0"].tobytes()
        s.set_probes(cells, capacity=2)
        for k in range(2):
            got = flat(s.probe_sample(delta))
            s.probe_record(delta, float(k))
            assert got.tobytes() == want.tobytes()
            _, after, _ = a.read()
            assert after.tobytes() == before.tobytes()       # X, B and the six other work vectors, ghosts and padding
            Z.assert_clean(a, z, "after probe_sample and probe_record")
        assert flat(s.probe_read()[1]).tobytes() == np.stack([want, want]).tobytes()


@pytest.mark.parametrize("pitched", [False, True])
def test_a_nan_solve_shows_in_the_sample_and_is_forgotten(E, monkeypatch, pitched):
    set_pitch(monkeypatch, pitched)
    args, prepare = case("g2")
    geo, geoC, delta = args[0], args[1], args[4]
    n = 3 * geo.size + int(np.count_nonzero(geoC))
    bb = np.random.Generator(np.random.PCG64(9)).standard_normal(n)
    bb[n // 3] = np.nan
    cells = shuffled_box(geo.size, 13)
    with E.EC3DSolver() as s:
        s.assemble(*args)
        s.set_probes(cells, capacity=1)
        assert not flat(s.probe_sample(delta)).any()               # the buffers exist before the bad solve
        x, _, _ = s.solve(bb, np.zeros(n), 1e-6, 7)
        assert not np.isfinite(x).all()
        s.probe_record(delta, 0.0)
        bad = flat(s.probe_sample(delta))                           # status 0: no exception
        assert np.isnan(bad[:, 0:3]).any() and np.isnan(bad[:, 9:12]).any()
        assert np.isnan(flat(s.probe_read()[1])).any()
        prepare(s)
        x, b = s.download("X"), s.download("B")
        assert np.isfinite(x).all() and np.isfinite(b).all()
        assert flat(s.probe_sample(delta)).tobytes() == PN.sample(geoC, delta, x, b, cells).tobytes()


# --------------------------------------------------------------------------------------------------------- 5. refusals
def test_poisson_csr_and_empty_handles_are_refused(E):
    import csr_generate as G
    delta = (0.004, 0.004, 0.004)
    calls = (lambda s: s.set_probes([0]), lambda s: s.probe_sample(delta), lambda s: s.probe_record(delta, 0.0),
             lambda s: s.probe_read(0, 0), lambda s: s.probe_reset())
    with E.EC3DSolver() as s:
        assert [status_of(E, lambda: f(s)) for f in calls] == [3] * 5          # nothing assembled
        assert s.probes()["nprobes"] == 0
        s.assemble_poisson(16, 8, 8)
        assert [status_of(E, lambda: f(s)) for f in calls] == [3] * 5
    with E.EC3DSolver() as s:
        s.set_matrix_csr(*G.case("nb3")[:3])
        assert [status_of(E, lambda: f(s)) for f in calls] == [3] * 5


def test_z_slab_is_refused(E):
    from eddy_currents_3d_amd.dist import HipAVSlabOps, slab_bounds
    g = load_golden(CAPTURED["g3"][0])
    k0, k1 = slab_bounds(g["geoPHYS"].shape[0], 0, 2)
    o = HipAVSlabOps(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]), k0, k1, 2)
    try:
        assert status_of(E, lambda: o.local.set_probes([0])) == 5
        assert status_of(E, lambda: o.local.probe_sample(g["delta"])) == 5
    finally:
        o.close()


def test_cells_outside_the_box_keep_the_earlier_set_and_an_assembly_clears_it(E):
    import ctypes as C
    args, prepare = case("g2")
    geoC, delta = args[1], args[4]
    N = geoC.size
    cells = np.array([3, N - 1, 0, 3], np.int64)
    with E.EC3DSolver() as s:
        s.assemble(*args)
        prepare(s)
        s.set_probes(cells, capacity=2)
        s.probe_record(delta, 1.0)
        first = flat(s.probe_sample(delta))
        for bad, at in (([5, 6, -1, N], 2), ([N, -1], 0), ([0] * 300 + [N], 300)):
            with pytest.raises(E.EC3DError) as err:
                s.set_probes(bad, capacity=4)
            assert err.value.status == 2 and f"cells[{at}]" in str(err.value)
            assert s.probes() == dict(nprobes=4, capacity=2, recorded=1, device_bytes=4 * (8 + 104 * 3))
            assert flat(s.probe_sample(delta)).tobytes() == first.tobytes()
        assert s.L.ec3d_set_probes(s.h, 2, None, 0) == 2 and s.L.ec3d_set_probes(s.h, -1, cells.ctypes.data, 0) == 2
        assert s.L.ec3d_set_probes(s.h, 4, cells.ctypes.data, -1) == 2
        assert s.L.ec3d_probe_sample(s.h, np.ascontiguousarray(delta, np.float64), None) == 2
        assert s.L.ec3d_probe_read(s.h, 0, 1, None, None) == 2 and s.L.ec3d_get_probes(s.h, None) == 2
        assert s.probes()["nprobes"] == 4
        s.assemble(*args)                                                  # a new assembly: the set is gone
        assert s.probes() == dict(nprobes=0, capacity=0, recorded=0, device_bytes=0)
        assert status_of(E, lambda: s.probe_sample(delta)) == 2


def test_multi_handle_and_slabs_are_refused_before_assembling(E):
    from eddy_currents_3d_amd import host
    with E.EC3DMulti(2, devices=[0, 0]) as mu:
        mu.assemble = lambda *a, **k: pytest.fail("assembled before refusing")
        with pytest.raises(ValueError, match="probes"):
            host.run(g3_model(), mu, steps=1, probes=[0])
    with pytest.raises(ValueError, match="probes"):
        host.run_slabs(g3_model(), 0, 1, probes=[0])


# ------------------------------------------------------------------------------ 6. more than one trip through the loop
def test_the_whole_big_box_and_one_plane_of_it(E):
    """A launch has min(ceil(nprobes / 256), 1024) workgroups of 256 threads, each thread taking the probes t, t + 256 *
    workgroups, ...: the 589 824 probes of the whole box would fill 2304 workgroups, so the 1024 launched go through the
    loop twice, the first 256 of them a third time.  The plane's 9216 probes are 36 workgroups, one trip."""
    from eddy_currents_3d_amd.probes import probe_box
    args, prepare = case("big")
    geo, geoC, delta = args[0], args[1], args[4]
    sdz, sdy, sdx = geo.shape
    assert (sdx, sdy, sdz) == (96, 96, 64) and (geo.size + 255) // 256 == 2304 > 2 * MAX_WGS
    whole = probe_box((0, 0, 0), (sdx - 1, sdy - 1, sdz - 1), (sdx, sdy, sdz))
    plane = probe_box((0, 0, 20), (sdx - 1, sdy - 1, 20), (sdx, sdy, sdz))
    assert len(whole) == 589824 and len(plane) == 9216 and np.count_nonzero(geoC.reshape(-1)[plane])
    with E.EC3DSolver() as s:
        s.assemble(*args)
        prepare(s)
        x, b = s.download("X"), s.download("B")
        s.set_probes(whole)
        got = flat(s.probe_sample(delta))
        s.set_probes(plane)
        got_plane = flat(s.probe_sample(delta))
    want = PN.whole_box(geoC, delta, x, b)
    diff = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    print(f"whole box: {len(diff)} of {len(whole)} probes differ from the twin" + (f", first {diff[0]}" if len(diff) else ""))
    assert got.tobytes() == want.tobytes()
    assert got_plane.tobytes() == want[plane].tobytes()


# ------------------------------------------------------------------------------------------------------------- 7. loop
def test_the_time_loop_records_every_step_and_changes_nothing(E, tmp_path, capsys):
    from eddy_currents_3d_amd import host, run, vxc
    from eddy_currents_3d_amd.probes import CSV_HEADER, probe_line, read_csv
    import dataclasses
    model = g3_model()
    names = [n.replace("stop=4m", "stop=5m") for n in model.names]       # g3 stops after four steps: one more
    assert names != model.names
    model = dataclasses.replace(model, names=names)
    t = vxc.domain_tables(model)
    geoC, delta = t["geoPHYS_C"], t["delta"]
    sdz, sdy, sdx = model.vox.shape
    cells = probe_line((0, 0, 0), (sdx - 1, sdy - 1, sdz - 1), (sdx, sdy, sdz))
    assert len(cells) == 18 and np.count_nonzero(np.asarray(geoC).reshape(-1)[cells])
    twin, seen, runs = [], [], {}

    def on_step(k, s, info):
        seen.append("probes" in info)
        twin.append(PN.sample(geoC, delta, s.download("X"), s.download("B"), cells))

    for flag in (False, True):
        with E.EC3DSolver() as s:
            log = host.run(model, s, steps=5, on_step=on_step if flag else None,
                           **(dict(probes=cells, probe_capacity=2) if flag else {}))   # drained after steps 2 and 4, and at the end
            runs[flag] = ([i["iter"] for i in log], s.download("X"))
            assert len(log) == 5 and all(("probes" in i) == flag for i in log)
            if flag:
                assert s.probes()["capacity"] == 2 and s.probes()["recorded"] == 0
    assert seen == [False] * 5                                # the hooks run before the record is read
    assert runs[True][0] == runs[False][0] and runs[True][1].tobytes() == runs[False][1].tobytes()
    for k, info in enumerate(log):
        assert info["probes"].shape == (18, 13) and info["probes"].dtype == np.float64
        assert info["probes"].tobytes() == twin[k].tobytes(), k
    assert log[0]["probes"].tobytes() != log[4]["probes"].tobytes() and any(i["probes"][:, 12].any() for i in log)

    path, csv = str(tmp_path / "model.vxc"), str(tmp_path / "probes.csv")
    vxc.write_vxc(path, model, compression="ZLIB")
    assert run.main([path, "--steps", "3", "--no-output", "--probes", csv, "--probe-line",
                     f"0,0,0:{sdx - 1},{sdy - 1},{sdz - 1}"]) == 0
    capsys.readouterr()
    lines = open(csv).read().splitlines()
    assert lines[0] == CSV_HEADER and len(lines) == 1 + 3 * 18
    back = read_csv(csv)
    assert back["values"].tobytes() == np.concatenate([i["probes"] for i in log[:3]]).tobytes()
    assert back["T"].tobytes() == np.repeat(np.array([i["T"] for i in log[:3]]), 18).tobytes()
    assert back["step"].tolist() == [k for k in range(3) for _ in range(18)] and back["probe"].tolist() == list(range(18)) * 3
