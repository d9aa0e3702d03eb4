"""ec3d_field_energy and ec3d_domain_linkage on the device: the magnetic energy of the box, the integral of A.J and the
flux linkage of every non-conducting domain from the resident X and B -- bit for bit against the twin
(tests/field_integrals_numpy.py: the same terms, the same order), in both storage forms and with pitched planes, against
the float32 field output of the same state, for what the calls leave alone, what they refuse, and in the time loop.

The twin reads X and B as EC3DSolver.download returns them (the reference's numbering), so a state reached by a solve is
downloaded from the structured handle and uploaded to the bands + tail handle: both then hold the same X and B and have
to return the same bits."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import av_generate as AG
import av_grids as AGR
import field_integrals_numpy as FI
import guard_zones as Z
from conftest import load_golden
from test_field_integrals_host import mirrored_vectors, two_coil_model
from test_gpu_domain_integrals import g3_model
from test_gpu_timeloop import coil_sources

pytestmark = pytest.mark.gpu

CAPTURED = {"g1": ("g1_nonconducting_8x7x6", False), "g2": ("g2_conducting_hole_16x15x14", False),
            "g2v": ("g2v_conducting_moving_16x15x14", False), "g3": ("g3_moving_coil_18x16x12", True)}
G8A = "g8a_two_plates_18x16x16"
KEYS = ["g1", "g2", "g2v", "g3", "g8a", "S3", "big"]
PITCHED = {"g1": (False, True), "g2": (False, True), "g2v": (False,), "g3": (False, True), "g8a": (False, True),
           "S3": (True,), "big": (False,)}     # S3's planes need the pitch; big's are whole tiles either way
VTK_BOUND = 1e-6
ORDER_BOUND = 1e-12


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def args_of(g):
    return g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"])


def big_box():
    """96 x 96 x 64 cells, a 56 x 56 x 20 plate: planes of 18 chunks, 1152 chunks in all -- the workgroup-strided loop of
    the streaming pass runs twice in 128 workgroups -- and an air list of 516 chunks, more than one round of k_dom_final."""
    return AG.from_boxes((96, 96, 64), [dict(boxes=[((20, 76), (20, 76), (20, 40))], C=AG.MU0 * 35.26e6, vel=(0.0, 0.0, 0.0))],
                         (1.5, 0.0, -0.25, -0.95, 0.5, -1.0), (0.005, 0.003, 0.004), 1e-3)


def case(key):
    """(assembly arguments, prepare(s): puts the state into a structured handle's X and B)."""
    if key in CAPTURED:
        name, moving = CAPTURED[key]
        g = dict(load_golden(name))
        if key == "g1":
            g["vox"] = np.where(g["vox"] > 0, g["vox"] + 1, 0)      # as tests/test_gpu_timeloop.py: g1's palette starts with the coils
        n = len(g["irow"]) - 1

        def prepare(s):                                          # one captured step
            s.upload("X", np.zeros(n))
            s.upload("B", np.zeros(n))
            idx, val = coil_sources(g, 0, moving)
            s.rhs_step(idx, val, moving=moving)
            s.solve_resident(float(g["tol"]), int(g["itmax"]))
            s.post_update()
        return args_of(g), prepare
    if key == "g8a":
        g = load_golden(G8A)

        def prepare(s):                                          # the captured solution of step 0, post-updated
            s.upload("B", g["b0"])
            s.upload("X", g["xout0"])
            s.post_update()
        return args_of(g), prepare
    args = AGR.system("S3") if key == "S3" else big_box()
    n = 3 * args[0].size + int(np.count_nonzero(args[1]))
    rng = np.random.Generator(np.random.PCG64(40 + KEYS.index(key)))
    x, b = rng.standard_normal(n), rng.standard_normal(n)

    def prepare(s):
        s.upload("X", x)
        s.upload("B", b)
    return args, prepare


def ebits(r):
    return (r["cells"], struct.pack("<4d", r["energy_b"], r["aj_source"], r["aj_eddy"], 0.0), r["energy_axis"].tobytes())


def lbits(recs):
    return [(r["domain"], r["cells"], struct.pack("<d", r["linkage"]), r["jsum"].tobytes()) for r in recs]


def show(what, got, want):
    print(f"{what}: energy_b {got['energy_b']!r} / twin {want['energy_b']!r}; aj_source {got['aj_source']!r} / "
          f"{want['aj_source']!r}; aj_eddy {got['aj_eddy']!r} / {want['aj_eddy']!r}")


# --------------------------------------------------------------------------------------------- 1. the twin, both forms
@pytest.mark.parametrize("key,pitched", [(k, p) for k in KEYS for p in PITCHED[k]])
def test_bits_equal_the_twin_in_both_forms(E, monkeypatch, key, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    else:
        monkeypatch.delenv("EC3D_PITCH", raising=False)
    args, prepare = case(key)
    geo, geoC, delta = args[0], args[1], args[4]
    plane = geo.shape[1] * geo.shape[2]
    with E.EC3DSolver(structured=True) as s:
        s.assemble(*args)
        assert s.info.tail_rows == 0
        if np.count_nonzero(geoC):
            pi = Z.pitch_info(s, plane)
            assert pi["pitch"] == ((plane + 511) // 512 * 512 if pitched else plane)
        prepare(s)
        x, b = s.download("X"), s.download("B")
        got_e, got_l = s.field_energy(delta), s.domain_linkage(delta)
        assert ebits(s.field_energy(delta)) == ebits(got_e) and lbits(s.domain_linkage(delta)) == lbits(got_l)
        ncond = s.domain_integrals(delta)
    terms = FI.cell_terms(geoC, delta, x, b)
    want_e = FI.field_energy(geoC, delta, x, b, terms)
    want_l = FI.domain_linkage(geo, geoC, delta, x, b, terms)
    show(f"{key} pitched={pitched}", got_e, want_e)
    assert np.isfinite(got_e["energy_b"]) and got_e["energy_b"] > 0
    assert ebits(got_e) == ebits(want_e)
    assert lbits(got_l) == lbits(want_l)
    assert [(r["domain"], r["cells"]) for r in got_l] == FI.linkage_lists(geo, geoC)
    assert not {r["domain"] for r in ncond} & {r["domain"] for r in got_l}
    if key == "g1":
        assert ncond == [] and struct.pack("<d", got_e["aj_eddy"]) == struct.pack("<d", 0.0)
    if key == "S3":
        assert pi["pitch"] == 1536 and pi["plane"] == 1200
    with E.EC3DSolver(structured=False) as s:
        s.assemble(*args)
        assert s.info.tail_rows > 0 or not np.count_nonzero(geoC)
        s.upload("X", x)
        s.upload("B", b)
        assert ebits(s.field_energy(delta)) == ebits(got_e)
        assert lbits(s.domain_linkage(delta)) == lbits(got_l)


# ------------------------------------------------------------------------------------------------ 2. against the fields
def test_sums_agree_with_the_field_output(E):
    """energy_b against the float64 sum of squares of ec3d_vtk_fields' float32 field_B: every component carries at most
    2^-24 of rounding, its square 2^-23 + 2^-48, and the terms are non-negative, so the sum errs by less than 2.4e-7 of
    itself; 1e-6 holds that and the summation.  A.J changes sign: its bound is 1e-6 of dV * sum|A.J| of the same fields
    (two rounded factors per product).  J = s * Jaf: field_eddy holds it, field_source holds Jaf itself."""
    args, prepare = case("g3")
    geoC, delta = args[1], args[4]
    N = geoC.size
    with E.EC3DSolver() as s:
        s.assemble(*args)
        prepare(s)
        e = s.field_energy(delta)
        link = s.domain_linkage(delta)
        f = s.vtk_fields(delta, N, True)
    vol = float(np.prod(delta))
    b2 = (f["B"].astype(np.float64) ** 2).sum()
    want = vol * 0.5 * FI.INV_MU0 * b2
    print(f"energy_b {e['energy_b']!r}, from the float32 fields {want!r}: relative difference {abs(e['energy_b'] - want) / want:.2e}")
    assert abs(e["energy_b"] - want) <= VTK_BOUND * want
    A = f["A"].astype(np.float64)
    J = fields_j(f)
    a = (A * J).sum(axis=1)
    scale = vol * np.abs(a).sum()
    print(f"aj_source + aj_eddy {e['aj_source'] + e['aj_eddy']!r}, from the fields {vol * a.sum()!r}, dV sum|A.J| {scale!r}")
    assert scale > 0 and abs(e["aj_source"] + e["aj_eddy"] - vol * a.sum()) <= VTK_BOUND * scale
    cond = np.asarray(geoC).reshape(-1) != 0
    assert abs(e["aj_eddy"] - vol * a[cond].sum()) <= VTK_BOUND * scale
    assert abs(sum(r["linkage"] for r in link) - vol * a[~cond].sum()) <= VTK_BOUND * scale


def fields_j(f):
    from fields_numpy import EDDY_SCALE
    return f["eddy"].astype(np.float64) + EDDY_SCALE * f["source"].astype(np.float64)      # one of the two is zero per cell


# ---------------------------------------------------------------------------------------------------------- 3. linkage
@pytest.mark.parametrize("key", ["g3", "g8a", "big"])
def test_linkages_and_eddy_part_make_up_the_whole(E, key):
    """The listed domains and the conductor cells are the box: from the twin's ordered sums the total is the twin's, and
    the streaming pass -- another order over the same terms -- agrees to 1e-12 of dV * sum|A.J| (the longest chain of
    either order is below 4096 additions: 4.5e-13)."""
    args, prepare = case(key)
    geo, geoC, delta = args[0], args[1], args[4]
    with E.EC3DSolver() as s:
        s.assemble(*args)
        prepare(s)
        x, b = s.download("X"), s.download("B")
        e, link = s.field_energy(delta), s.domain_linkage(delta)
    t = FI.cell_terms(geoC, delta, x, b)
    vol = float(np.prod(delta))
    scale = vol * np.abs(t["a"]).sum()
    want_l = FI.domain_linkage(geo, geoC, delta, x, b, t)
    want_e = FI.field_energy(geoC, delta, x, b, t)
    total = sum(r["linkage"] for r in link) + e["aj_eddy"]
    assert total == sum(r["linkage"] for r in want_l) + want_e["aj_eddy"]
    print(f"{key}: lists + aj_eddy {total!r}, streaming total {e['aj_source'] + e['aj_eddy']!r}, dV sum|A.J| {scale!r}")
    assert abs(total - (e["aj_source"] + e["aj_eddy"])) <= ORDER_BOUND * scale
    assert abs(total - vol * math.fsum(t["a"].tolist())) <= ORDER_BOUND * scale


@pytest.mark.parametrize("structured", [True, False])
def test_mirrored_coils_return_equal_linkages(E, structured):
    args = two_coil_model()
    geo, geoC, delta = args[0], args[1], args[4]
    x, b = mirrored_vectors(geo, geoC)
    with E.EC3DSolver(structured=structured) as s:
        s.assemble(*args)
        s.upload("X", x)
        s.upload("B", b)
        r = {q["domain"]: q for q in s.domain_linkage(delta)}
    assert sorted(r) == [1, 3, 4] and r[1]["cells"] == r[3]["cells"] == 72
    assert r[1]["linkage"] != 0.0 and struct.pack("<d", r[1]["linkage"]) == struct.pack("<d", r[3]["linkage"])
    assert struct.pack("<d", r[1]["jsum"][1]) == struct.pack("<d", -r[3]["jsum"][1]) and r[1]["jsum"][1] != 0.0
    assert not r[1]["jsum"][[0, 2]].any() and not r[3]["jsum"][[0, 2]].any()
    assert r[4]["linkage"] == 0.0 and not r[4]["jsum"].any()
    assert lbits(list(r.values())) == lbits(FI.domain_linkage(geo, geoC, delta, x, b))


# ------------------------------------------------------------------------------------- 4. what the calls leave alone
@pytest.mark.parametrize("pitched", [False, True])
def test_the_calls_change_no_vector_and_no_canary(E, monkeypatch, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    else:
        monkeypatch.delenv("EC3D_PITCH", raising=False)
    g = load_golden(CAPTURED["g3"][0])
    args = args_of(g)
    delta = args[4]
    sdz, sdy, sdx = g["geoPHYS"].shape
    with E.EC3DSolver() as plain:
        plain.assemble(*args)
        plain.upload("B", g["b0"])
        plain.upload("X", g["xout0"])
        plain.post_update()
        want = ebits(plain.field_energy(delta)), lbits(plain.domain_linkage(delta))
    with Z.adopted(E, lambda s: s.assemble(*args)) as a:
        s = a.s
        z = Z.zones(s.vector_layout(), Z.pitch_info(s, sdx * sdy))
        s.upload("B", g["b0"])
        s.upload("X", g["xout0"])
        s.post_update()
        _, before, _ = a.read()
        before = before.copy()
        for _ in range(2):                                   # the first call allocates and uploads, the second does not
            got = ebits(s.field_energy(delta)), lbits(s.domain_linkage(delta))
            assert got == want
            _, after, _ = a.read()
            assert after.tobytes() == before.tobytes()       # X, B and the six other work vectors, ghosts and padding
            Z.assert_clean(a, z, "after field_energy and domain_linkage")


@pytest.mark.parametrize("pitched", [False, True])
def test_a_nan_solve_gives_nan_sums_and_is_forgotten(E, monkeypatch, pitched):
    if pitched:
        monkeypatch.setenv("EC3D_PITCH", "2")
    else:
        monkeypatch.delenv("EC3D_PITCH", raising=False)
    args, prepare = case("g2")
    geo, geoC, delta = args[0], args[1], args[4]
    n = 3 * geo.size + int(np.count_nonzero(geoC))
    bb = np.random.Generator(np.random.PCG64(9)).standard_normal(n)
    bb[n // 3] = np.nan
    with E.EC3DSolver() as s:
        s.assemble(*args)
        first = s.field_energy(delta), s.domain_linkage(delta)     # the buffers exist before the bad solve
        assert first[0]["energy_b"] == 0.0
        x, _, _ = s.solve(bb, np.zeros(n), 1e-6, 7)
        assert not np.isfinite(x).all()
        e, link = s.field_energy(delta), s.domain_linkage(delta)   # status 0: no exception
        assert np.isnan(e["energy_b"]) and np.isnan(e["aj_source"] + e["aj_eddy"])
        assert any(np.isnan(r["linkage"]) for r in link)
        prepare(s)
        x, b = s.download("X"), s.download("B")
        assert np.isfinite(x).all() and np.isfinite(b).all()
        assert ebits(s.field_energy(delta)) == ebits(FI.field_energy(geoC, delta, x, b))
        assert lbits(s.domain_linkage(delta)) == lbits(FI.domain_linkage(geo, geoC, delta, x, b))


# --------------------------------------------------------------------------------------------------------- 5. refusals
def status_of(E, f):
    with pytest.raises(E.EC3DError) as err:
        f()
    return err.value.status


def test_poisson_and_csr_handles_are_refused(E):
    import csr_generate as G
    delta = (0.004, 0.004, 0.004)
    with E.EC3DSolver() as s:
        s.assemble_poisson(16, 8, 8)
        assert status_of(E, lambda: s.field_energy(delta)) == 3 and status_of(E, lambda: s.domain_linkage(delta)) == 3
    with E.EC3DSolver() as s:
        s.set_matrix_csr(*G.case("nb3")[:3])
        assert status_of(E, lambda: s.field_energy(delta)) == 3 and status_of(E, lambda: s.domain_linkage(delta)) == 3


def test_z_slab_is_refused(E):
    from eddy_currents_3d_amd.dist import HipAVSlabOps, slab_bounds
    g = load_golden(CAPTURED["g3"][0])
    k0, k1 = slab_bounds(g["geoPHYS"].shape[0], 0, 2)
    o = HipAVSlabOps(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]), k0, k1, 2)
    try:
        assert status_of(E, lambda: o.local.field_energy(g["delta"])) == 5
        assert status_of(E, lambda: o.local.domain_linkage(g["delta"])) == 5
    finally:
        o.close()


def test_null_arguments_and_small_capacity(E):
    args = two_coil_model()
    delta = np.ascontiguousarray(args[4], np.float64)
    with E.EC3DSolver() as s:
        s.assemble(*args)
        n = C.c_int32(0)
        out = (E.solver.DomainLink * 3)()
        assert s.L.ec3d_domain_linkage(s.h, delta, 2, C.byref(n), out) == 2 and n.value == 3
        n = C.c_int32(0)
        assert s.L.ec3d_domain_linkage(s.h, delta, 0, C.byref(n), None) == 0 and n.value == 3
        assert s.L.ec3d_domain_linkage(s.h, delta, 3, C.byref(n), out) == 0 and n.value == 3
        assert [(r.domain, r.cells) for r in out] == [(1, 72), (3, 72), (4, 22 * 12 * 10 - 288)]
        assert s.L.ec3d_domain_linkage(s.h, delta, 3, None, out) == 2
        assert s.L.ec3d_field_energy(s.h, delta, None) == 2


def test_multi_handle_is_refused_before_assembling(E):
    from eddy_currents_3d_amd import host
    with E.EC3DMulti(2, devices=[0, 0]) as mu:
        mu.assemble = lambda *a, **k: pytest.fail("assembled before refusing")
        with pytest.raises(ValueError, match="energy"):
            host.run(g3_model(), mu, steps=1, energy=True)


# ------------------------------------------------------------------------------------------------------------- 6. loop
def test_the_time_loop_carries_both_and_changes_nothing(E):
    from eddy_currents_3d_amd import host, vxc
    model = g3_model()
    delta = vxc.domain_tables(model)["delta"]
    direct, runs = [], {}

    def on_step(k, s, info):
        direct.append((ebits(s.field_energy(delta)), lbits(s.domain_linkage(delta))))

    for flag in (False, True):
        with E.EC3DSolver() as s:
            log = host.run(model, s, steps=3, energy=flag, on_step=on_step if flag else None)
            runs[flag] = ([i["iter"] for i in log], s.download("X"))
            assert len(log) == 3
            assert all(("energy" in i) == flag and ("linkage" in i) == flag and "integrals" not in i for i in log)
            if flag:
                assert [(ebits(i["energy"]), lbits(i["linkage"])) for i in log] == direct
                assert all(i["energy"]["energy_b"] > 0 for i in log)
    assert runs[True][0] == runs[False][0] and runs[True][1].tobytes() == runs[False][1].tobytes()


def test_command_line_writes_one_line_per_step(tmp_path, capsys):
    from eddy_currents_3d_amd import run, vxc
    path, csv = str(tmp_path / "model.vxc"), str(tmp_path / "energy.csv")
    vxc.write_vxc(path, g3_model(), compression="ZLIB")
    assert run.main([path, "--steps", "3", "--no-output", "--energy", csv]) == 0
    capsys.readouterr()
    lines = open(csv).read().splitlines()
    head = lines[0].split(",")
    assert lines[0].startswith(run.ENERGY_HEADER + ",linkage_") and len(lines) == 4
    assert all(h.startswith("linkage_") and h[8:].isdigit() for h in head[5:])
    assert [int(h[8:]) for h in head[5:]] == sorted(int(h[8:]) for h in head[5:])
    for k, line in enumerate(lines[1:]):
        f = line.split(",")
        assert len(f) == len(head) and int(f[0]) == k and all(np.isfinite(float(v)) for v in f[1:])
        assert float(f[2]) > 0
