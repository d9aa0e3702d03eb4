"""ec3d_domain_integrals on the device: Joule loss and Lorentz force per conducting domain from the resident X and B,
against the float64 twin (tests/domain_integrals_numpy.py, math.fsum per domain), against the float32 field output of
the same state (ec3d_vtk_fields), between the two storage forms, and for what the call must leave alone and refuse.

The bound on a sum.  The per-cell terms are the twin's bit for bit (same expressions, no contraction); what differs is
the order of the additions.  The kernel's longest chain of dependent additions is below 4096 (ec3d_integrals.hip), so
its sum errs by at most 4096 * 2^-53 * sum|t| = 4.5e-13 * sum|t|; fsum's by half an ulp of the result; the scaling
(two or three roundings, relative to the value, which is at most sum|t|) adds 3.3e-16.  1e-12 * sum|t| holds all of
it, and a dropped cell, a wrong neighbour or a cell in the wrong domain misses it by orders of magnitude."""
import ctypes as C

import numpy as np
import pytest

import domain_integrals_numpy as DI
from conftest import load_golden
from test_domain_integrals_host import chunk_edge_geometry

pytestmark = pytest.mark.gpu

FIXTURES = {"g2": "g2_conducting_hole_16x15x14", "g3": "g3_moving_coil_18x16x12", "g8a": "g8a_two_plates_18x16x16",
            "g8b": "g8b_stacked_moving_20x16x14", "g8c": "g8c_side_by_side_20x18x14", "g8d": "g8d_g3_split_18x16x12"}
SUM_BOUND = 1e-12
VTK_BOUND = 1e-6


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def args_of(g):
    return g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"])


_cache = {}


def random_case(key):
    """(assembly arguments, X, B, the twin's records), made once per geometry."""
    if key not in _cache:
        args = chunk_edge_geometry() if key == "chunks" else args_of(load_golden(FIXTURES[key]))
        geo, geoC, valPHYS, _, delta, _ = args
        n = 3 * geo.size + int((np.asarray(geoC) != 0).sum())
        rng = np.random.Generator(np.random.PCG64(20 + sorted(list(FIXTURES) + ["chunks"]).index(key)))
        x, b = rng.standard_normal(n), rng.standard_normal(n)
        _cache[key] = (args, x, b, DI.integrals(geo, geoC, valPHYS, delta, x, b))
    return _cache[key]


def check_against(got, want, bound, what):
    """domain, cells and sigma exactly; each of the four sums within bound * sum|term| (every figure printed first)."""
    assert [r["domain"] for r in got] == [r["domain"] for r in want], what
    for r, w in zip(got, want):
        assert r["cells"] == w["cells"] and r["sigma"] == w["sigma"], (what, r["domain"])
        g4 = np.concatenate([[r["joule_w"]], r["force_n"]])
        w4 = np.concatenate([[w["joule_w"]], w["force_n"]])
        err = np.abs(g4 - w4) / w["abs"]
        print(f"{what} domain {r['domain']}: {r['cells']} cells; |sum - reference| / sum|term| = "
              + " ".join(f"{e:.2e}" for e in err) + f";  sum|term| / |sum| = "
              + " ".join(f"{a / max(abs(v), 1e-300):.0f}" for a, v in zip(w["abs"], w4)))
        assert np.all(np.abs(g4 - w4) <= bound * w["abs"]), (what, r["domain"])


def same_bits(a, b):
    assert len(a) == len(b)
    for r, w in zip(a, b):
        assert (r["domain"], r["cells"]) == (w["domain"], w["cells"])
        assert np.array([r["sigma"], r["joule_w"]]).tobytes() == np.array([w["sigma"], w["joule_w"]]).tobytes()
        assert r["force_n"].tobytes() == w["force_n"].tobytes()


def g3_model():
    """g3 as a model host.run can step: g8d is g3 with its plate split in two, and carries the palette."""
    from eddy_currents_3d_amd import vxc
    g3, g8 = load_golden(FIXTURES["g3"]), load_golden(FIXTURES["g8d"])
    names = [str(x) for x in g8["names"]]
    vox = g8["vox"].copy()
    vox[vox == 2] = 1
    vox[vox > 2] -= 1
    model = vxc.VxcModel(vox, [names[0]] + names[2:], float(str(g8["lattice_dim"])), (1.0, 1.0, 1.0))
    assert np.array_equal(vxc.domain_tables(model)["geoPHYS_C"].reshape(-1), g3["geoPHYS_C"].reshape(-1))
    return model


# ------------------------------------------------------------------------------------------ 1. the twin
@pytest.mark.parametrize("key", sorted(FIXTURES))
def test_random_vectors_equal_the_twin(E, plane_pitch, key):
    args, x, b, want = random_case(key)
    with E.EC3DSolver() as s:
        s.assemble(*args)
        s.upload("X", x)
        s.upload("B", b)
        got = s.domain_integrals(args[4])
    assert len(want) == (1 if key in ("g2", "g3") else 2)
    check_against(got, want, SUM_BOUND, f"{key} ({plane_pitch})")


# ------------------------------------------------------------------------------------- 2. storage forms
@pytest.mark.parametrize("key", ["g3", "g8a"])
def test_both_storage_forms_give_the_same_bits(E, key):
    """The list order is a property of the geometry: bands + tail sums what the structured form sums, in its order."""
    args, x, b, want = random_case(key)
    got = {}
    for structured in (True, False):
        with E.EC3DSolver(structured=structured) as s:
            s.assemble(*args)
            assert (s.info.tail_rows == 0) == structured
            s.upload("X", x)
            s.upload("B", b)
            got[structured] = s.domain_integrals(args[4])
    same_bits(got[True], got[False])
    check_against(got[False], want, SUM_BOUND, f"{key} (bands + tail)")


# --------------------------------------------------------------------------------------- 3. chunk edges
def test_chunk_edges_and_domain_ids(E):
    """Domains 3, 1, 4 of 4840 = 4 * 1024 + 744, 27 and 1024 cells: a chunk tail that ends inside a wave, a domain
    smaller than a wave and a domain of exactly one chunk; the ids in palette order, the records in id order, each
    with its own sigma."""
    args, x, b, want = random_case("chunks")
    valPHYS = args[2]
    for structured in (True, False):
        with E.EC3DSolver(structured=structured) as s:
            s.assemble(*args)
            s.upload("X", x)
            s.upload("B", b)
            got = s.domain_integrals(args[4])
        assert [(r["domain"], r["cells"]) for r in got] == [(1, 27), (3, 4840), (4, 1024)]
        assert [r["sigma"] for r in got] == [valPHYS[d - 1, 1] * DI.SIGMA_SCALE for d in (1, 3, 4)]
        assert len({r["sigma"] for r in got}) == 3
        check_against(got, want, SUM_BOUND, f"chunks (structured={structured})")


# ----------------------------------------------------------------------------------------- 4. real steps
def test_real_steps_agree_with_the_field_output(E):
    """host.run(..., integrals=True) on g3: every step's info["integrals"] is what a direct call in on_step returns,
    the loss is positive, and each sum lies within 1e-6 * sum|term| of the same sum formed from that step's float32
    ec3d_vtk_fields output (every factor of a product carries a rounding to float32, 2^-24 = 6e-8, so a term errs by
    about 1.2e-7 of its magnitude, 2.4e-7 allowing two roundings per factor; the margin is 4 x) -- the field kernel,
    not the twin, is the reference here."""
    from eddy_currents_3d_amd import host, vxc
    model = g3_model()
    t = vxc.domain_tables(model)
    delta, N = t["delta"], t["geoPHYS"].size
    cells = np.flatnonzero(np.asarray(t["geoPHYS_C"]).reshape(-1) != 0)
    direct, fields = [], []

    def on_step(k, s, info):
        direct.append(s.domain_integrals(delta))
        fields.append(s.vtk_fields(delta, N, True))

    with E.EC3DSolver() as s:
        log = host.run(model, s, steps=3, on_step=on_step, integrals=True)
    assert len(log) == 3
    for k, info in enumerate(log):
        same_bits(info["integrals"], direct[k])
        assert all(r["joule_w"] > 0 for r in info["integrals"])
        j = fields[k]["eddy"].astype(np.float64)[cells]
        bb = fields[k]["B"].astype(np.float64)[cells]
        terms = np.concatenate([(j * j).sum(axis=1)[:, None], np.cross(j, bb)], axis=1)
        want = [DI.scaled(t["valPHYS"], delta, d, n, sm, a) for d, n, sm, a in DI.sums_by_domain(t["geoPHYS"], cells, terms)]
        check_against(info["integrals"], want, VTK_BOUND, f"g3 step {k} vs float32 fields")


# ---------------------------------------------------------------------------------------- 5. side effects
def test_the_call_changes_nothing_and_repeats_itself(E):
    args, x, b, _ = random_case("g8a")
    with E.EC3DSolver() as s:
        s.assemble(*args)
        s.upload("X", x)
        s.upload("B", b)
        x0, b0 = s.download("X"), s.download("B")
        first = s.domain_integrals(args[4])
        second = s.domain_integrals(args[4])
        assert s.download("X").tobytes() == x0.tobytes() and s.download("B").tobytes() == b0.tobytes()
    same_bits(first, second)


def test_the_time_loop_is_the_same_with_and_without(E):
    from eddy_currents_3d_amd import host
    model = g3_model()
    runs = {}
    for flag in (False, True):
        with E.EC3DSolver() as s:
            log = host.run(model, s, steps=3, integrals=flag)
            runs[flag] = ([i["iter"] for i in log], s.download("X"))
            assert all(("integrals" in i) == flag for i in log)
    assert runs[True][0] == runs[False][0]
    assert runs[True][1].tobytes() == runs[False][1].tobytes()


# ------------------------------------------------------------------------------------ 6. refusals, edges
def test_poisson_handle_is_refused(E):
    with E.EC3DSolver() as s:
        s.assemble_poisson(16, 8, 8)
        with pytest.raises(E.EC3DError) as err:
            s.domain_integrals((0.004, 0.004, 0.004))
        assert err.value.status == 3


def test_no_conductor_gives_an_empty_list(E):
    g = load_golden("g1_nonconducting_8x7x6")
    with E.EC3DSolver() as s:
        s.assemble(*args_of(g))
        n = C.c_int32(-1)
        out = (E.solver.DomainIntegral * 1)()
        assert s.L.ec3d_domain_integrals(s.h, np.ascontiguousarray(g["delta"], np.float64), 1, C.byref(n), out) == 0
        assert n.value == 0
        assert s.domain_integrals(g["delta"]) == []


def test_z_slab_is_refused(E):
    from eddy_currents_3d_amd.dist import HipAVSlabOps, slab_bounds
    g = load_golden(FIXTURES["g3"])
    k0, k1 = slab_bounds(g["geoPHYS"].shape[0], 0, 2)
    o = HipAVSlabOps(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]), k0, k1, 2)
    try:
        with pytest.raises(E.EC3DError) as err:
            o.local.domain_integrals(g["delta"])
        assert err.value.status == 5
    finally:
        o.close()


def test_small_capacity_is_refused_with_the_count(E):
    args, x, b, _ = random_case("g8a")
    delta = np.ascontiguousarray(args[4], np.float64)
    with E.EC3DSolver() as s:
        s.assemble(*args)
        s.upload("X", x)
        s.upload("B", b)
        n = C.c_int32(0)
        out = (E.solver.DomainIntegral * 2)()
        assert s.L.ec3d_domain_integrals(s.h, delta, 1, C.byref(n), out) == 2 and n.value == 2
        n = C.c_int32(0)
        assert s.L.ec3d_domain_integrals(s.h, delta, 0, C.byref(n), None) == 0 and n.value == 2
        assert s.L.ec3d_domain_integrals(s.h, delta, 2, C.byref(n), out) == 0 and n.value == 2
        same_bits([dict(domain=r.domain, cells=r.cells, sigma=r.sigma, joule_w=r.joule_w,
                        force_n=np.array(r.force_n[:])) for r in out], s.domain_integrals(delta))


def test_multi_handle_is_refused_before_assembling(E):
    from eddy_currents_3d_amd import host
    with E.EC3DMulti(2, devices=[0, 0]) as mu:
        mu.assemble = lambda *a, **k: pytest.fail("assembled before refusing")
        with pytest.raises(ValueError, match="integrals"):
            host.run(g3_model(), mu, steps=1, integrals=True)
