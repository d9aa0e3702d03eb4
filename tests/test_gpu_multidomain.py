"""Models with several conducting domains on the device, against the unmodified reference's captures
tests/golden/g8*_*.npz (tools/make_multidomain_goldens.py) and the restatement tests/multidomain_numpy.py.

* form: the structured A-V form with 55 + 9 D classes where the U ids are in scan order (g8a, g8b, g8d, up to 22
  synthetic domains), bands + tail otherwise (g8c, 24 domains); export_csr == the captured CSR, SpMV == the oracle's
  bit for bit, both plane pitches;
* every captured step: rhs_step / post_update give the captured b bit for bit, the solve equals the GPU-order twin bit
  for bit and takes the reference's iteration count;
* host.run of each fixture: the reference's right-hand sides and iteration counts;
* u_rhs: on g8a-c both rules equal the restatement bit for bit and differ; "all" on g8d is g3's one-domain run bit
  for bit, on g2 / g3 it is the default; bad rules are refused and leave the handle's rule;
* 22 synthetic domains structured, 23 on bands + tail, both converging on every step;
* block multigrid on g8a / g8b and up to 4 domains, refused from 5; several domains on slabs and multi handles still
  return status 5."""
import numpy as np
import pytest

import avmg_numpy as AV
import multidomain_numpy as MD
from conftest import load_golden

pytestmark = pytest.mark.gpu
G8 = {"g8a": "g8a_two_plates_18x16x16", "g8b": "g8b_stacked_moving_20x16x14", "g8c": "g8c_side_by_side_20x18x14",
      "g8d": "g8d_g3_split_18x16x12"}
STRUCTURED = {"g8a": True, "g8b": True, "g8c": False, "g8d": True}


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


def _model(g):
    from eddy_currents_3d_amd import vxc
    return vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                        tuple(float(x) for x in g["adj"]))


def _vtk_vectors(blob):
    """{name: float64 [3 npoints]} of a legacy-VTK field file (big-endian float32 payloads)."""
    import re
    out, pos = {}, 0
    npts = int(re.search(rb"POINT_DATA\s+(\d+)", blob).group(1))
    while True:
        i = blob.find(b"VECTORS ", pos)
        if i < 0:
            return out
        j = blob.index(b"\n", i)
        out[blob[i:j].split()[1].decode()] = np.frombuffer(blob, ">f4", 3 * npts, j + 1).astype(np.float64)
        pos = j + 1 + 12 * npts


def _assemble(s, g):
    s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))


def _check_matrix(s, valA, irow, jcol, oracle, D, structured):
    mi = s.info
    if structured:
        assert mi.tail_rows == 0 and mi.dict_classes == 55 + 9 * D
    else:
        assert mi.tail_rows > 0
    va, ir, jc = s.export_csr()
    assert np.array_equal(ir, irow) and np.array_equal(jc, jcol) and np.array_equal(va, valA)
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(2):
        x = rng.standard_normal(s.n)
        assert np.array_equal(s.spmv(x), oracle.spmv_csr(valA, irow, jcol, x))


@pytest.mark.parametrize("case", sorted(G8))
def test_form_and_matrix(E, oracle, plane_pitch, case):
    g = load_golden(G8[case])
    with E.EC3DSolver() as s:
        _assemble(s, g)
        _check_matrix(s, g["valA"], g["irow"], g["jcol"], oracle, 2, STRUCTURED[case])


@pytest.mark.parametrize("case", sorted(G8))
def test_every_captured_step(E, oracle, case):
    """From the captured previous step (b, x_out) the device's post_update and rhs_step give the restatement's
    vectors and the captured b bit for bit; the solve equals the GPU-order twin bit for bit and takes the reference's
    iteration count; where the reference converges, x lies within 10 tol of its x and the true residual below tol."""
    from eddy_currents_3d_amd import host, vxc
    g = load_golden(G8[case])
    tol, itmax = float(g["tol"]), int(g["itmax"])
    model = _model(g)
    prog = host.SourceProgram(model, vxc.domain_tables(model))
    shape, dt = g["vox"].shape, float(g["dt"])
    T = 0.0
    with E.EC3DSolver() as s:
        _assemble(s, g)
        n = s.n
        for k in range(len(g["iters"])):
            if k == 0:
                s.upload("B", np.zeros(n))
                s.upload("X", np.zeros(n))
            else:
                s.upload("B", g[f"b{k - 1}"])
                s.upload("X", g[f"xout{k - 1}"])
                s.post_update()
                bp, xp = MD.post_update(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape, g[f"b{k - 1}"],
                                        g[f"xout{k - 1}"])
                assert np.array_equal(s.download("B"), bp) and np.array_equal(s.download("X"), xp)
            idx, val, moving = prog.step(T)
            s.rhs_step(idx, val, moving=moving)
            b = s.download("B")
            assert np.array_equal(b, g[f"b{k}"]), f"step {k}"
            x0 = s.download("X")
            it, _ = s.solve_resident(tol, itmax)
            x = s.download("X")
            xt, itt, _, _ = oracle.twin_solve(s, g["valA"], g["irow"], g["jcol"], b, x0, tol, itmax)
            assert it == itt == int(g["iters"][k]) and np.array_equal(x, xt), f"step {k}"
            print(f"{case} step {k}: {it} iterations; x vs the reference's "
                  f"{np.linalg.norm(x - g[f'xout{k}']) / np.linalg.norm(g[f'xout{k}']):.2e}")
            if it <= itmax:      # converged (g8c stalls: U rows and columns in different orders; itmax exit)
                xr = g[f"xout{k}"]
                assert np.linalg.norm(x - xr) <= 10 * tol * np.linalg.norm(xr)
                assert s.true_residual()[0] < tol
            T = T + dt


def test_stalling_case_first_iterates():
    """g8c stalls (the reference takes the itmax exit on every step), so its iterate after 41 iterations is rounding
    noise on both sides.  Its first K = 5 iterates are not: cut there (tests/golden/g8ck_*), the device lands within
    10 tol of the reference's x, on bands + tail, and equals the GPU-order twin bit for bit."""
    import eddy_currents_3d_amd as E
    from oracle import oracle as O
    g, gk = load_golden(G8["g8c"]), load_golden("g8ck_side_by_side_first_iterates")
    assert np.array_equal(gk["b0"], g["b0"])
    tol, itmax = float(gk["tol"]), int(gk["itmax"])
    with E.EC3DSolver() as s:
        _assemble(s, g)
        assert s.info.tail_rows > 0
        x, it, _ = s.solve(gk["b0"], gk["xin0"], tol, itmax)
        xt, itt, _, _ = O.twin_solve(s, g["valA"], g["irow"], g["jcol"], gk["b0"], gk["xin0"], tol, itmax)
    xr = gk["xout0"]
    d = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    print(f"g8c first {it} iterations: x vs the reference's {d:.2e}")
    assert it == itt == int(gk["iters"][0]) and np.array_equal(x, xt) and d <= 10 * tol


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", sorted(G8))
def test_host_run(E, case, tmp_path):
    """The whole run through host.run: step 0's b bit for bit, later b within 10 tol where the reference converged
    (they carry x; g8c takes the itmax exit every step), the reference's iteration count on every step, and the last
    field_N.vtk with the reference's size, byte-identical to the reference's and its four vectors within 10 tol (g8c:
    the distance is printed; neither run converges, so there is nothing to bound: test_stalling_case_first_iterates)."""
    from eddy_currents_3d_amd import host
    g = load_golden(G8[case])
    tol = float(g["tol"])
    seen = []
    with E.EC3DSolver() as s:
        log = host.run(_model(g), s, out_dir=str(tmp_path), on_rhs=lambda k, s, info: seen.append(s.download("B")))
    assert [i["iter"] for i in log] == [int(v) for v in g["iters"]]
    for k, b in enumerate(seen):
        br = g[f"b{k}"]
        if k == 0:
            assert np.array_equal(b, br)
        elif int(g["iters"][k - 1]) <= int(g["itmax"]):
            assert np.linalg.norm(b - br) <= 10 * tol * np.linalg.norm(br)
    last = str(g["vtk_last"])
    ref = g["vtk_" + last[:-4]].tobytes()
    got = (tmp_path / last).read_bytes()
    assert len(got) == len(ref)
    vg, vr = _vtk_vectors(got), _vtk_vectors(ref)
    assert sorted(vg) == sorted(vr) and len(vr) == 4
    for name in vr:
        d = np.linalg.norm(vg[name] - vr[name]) / max(np.linalg.norm(vr[name]), 1e-300)
        print(f"{case}: {last} {name}: rel diff {d:.2e}, file byte-identical {got == ref}")
        if case != "g8c":
            assert d <= 10 * tol, name
    if case != "g8c":                   # the field output step's x is the converged one: the same bytes
        assert got == ref


def test_u_rhs_all_on_split_plate_is_the_one_domain_run(E):
    """g8d is g3 with its plate split into two domains of one material: under "all" every step's X equals g3's
    one-domain run bit for bit (same numbering: the split is a z-plane); under "reference" the run takes g8d's
    captured iteration counts."""
    from eddy_currents_3d_amd import host
    g3, g8 = load_golden("g3_moving_coil_18x16x12"), load_golden(G8["g8d"])
    names3 = [str(x) for x in g8["names"]]
    vox3 = g8["vox"].copy()
    vox3[vox3 == 2] = 1
    vox3[vox3 > 2] -= 1
    names3 = [names3[0]] + names3[2:]
    from eddy_currents_3d_amd import vxc
    m3 = vxc.VxcModel(vox3, names3, float(str(g8["lattice_dim"])), (1.0, 1.0, 1.0))
    assert np.array_equal(vxc.domain_tables(m3)["geoPHYS_C"].reshape(-1), g3["geoPHYS_C"].reshape(-1))
    xs = {}
    for key, model, rule in (("g3", m3, None), ("g8d-all", _model(g8), "all"), ("g8d-ref", _model(g8), "reference")):
        got = []
        with E.EC3DSolver() as s:
            log = host.run(model, s, u_rhs=rule, on_solved=lambda k, s, info: got.append(s.download("X")))
        xs[key] = (got, [i["iter"] for i in log])
    assert xs["g3"][1] == [int(v) for v in g3["iters"]]
    assert xs["g8d-all"][1] == xs["g3"][1]
    for a, b in zip(xs["g8d-all"][0], xs["g3"][0]):
        assert np.array_equal(a, b)
    assert xs["g8d-ref"][1] == [int(v) for v in g8["iters"]]


@pytest.mark.parametrize("name", ["g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12"])
def test_u_rhs_all_with_one_domain_is_the_default(E, name):
    g = load_golden(name)
    n = None
    outs = []
    for rule in ("reference", "all"):
        with E.EC3DSolver() as s:
            _assemble(s, g)
            s.set_u_rhs(rule)
            n = s.n
            s.upload("B", g["b0"])
            s.upload("X", g["xout0"])
            s.post_update()
            idx = np.arange(1, 3 * int(np.prod(g["geoPHYS"].shape)) + 1, 97, dtype=np.int32)
            s.rhs_step(idx, np.linspace(-1.0, 1.0, len(idx)), moving=False)
            outs.append((s.download("B"), s.download("X")))
    assert n and np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_bad_u_rhs_rule_is_refused(E):
    g = load_golden(G8["g8a"])
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.set_u_rhs("all")
        assert s.L.ec3d_set_u_rhs(s.h, 7) == 2 and s.L.ec3d_set_u_rhs(s.h, -1) == 2
        with pytest.raises(ValueError):
            s.set_u_rhs("every")
        s.upload("B", np.zeros(s.n))
        s.upload("X", g["xout1"])
        s.rhs_step(np.zeros(0, np.int32), np.zeros(0), moving=False)
        b_after = s.download("B")
    fresh = {}
    for rule in ("all", "reference"):  # the refused calls left "all" in place, and on g8a the rules differ
        with E.EC3DSolver() as s:
            _assemble(s, g)
            s.set_u_rhs(rule)
            s.upload("B", np.zeros(s.n))
            s.upload("X", g["xout1"])
            s.rhs_step(np.zeros(0, np.int32), np.zeros(0), moving=False)
            fresh[rule] = s.download("B")
    assert np.array_equal(fresh["all"], b_after) and not np.array_equal(fresh["reference"], b_after)


@pytest.mark.parametrize("case", ["g8a", "g8b", "g8c"])
def test_both_u_rhs_rules_equal_the_restatement(E, case):
    """From each captured step's b and x_out: post_update then rhs_step under "reference" and under "all" give
    tests/multidomain_numpy.py's vector of that rule bit for bit ("reference": the captured b), the rules agree on
    every row before max siznod, and differ on some row after it."""
    from eddy_currents_3d_amd import host, vxc
    g = load_golden(G8[case])
    model = _model(g)
    shape, dt = g["vox"].shape, float(g["dt"])
    N = int(np.prod(shape))
    nmax = max(len(c) for _, c in MD.conductors(g["geoPHYS"], g["geoPHYS_C"]))
    prog = host.SourceProgram(model, vxc.domain_tables(model))
    T = 0.0
    prog.step(T)
    differ = 0
    for k in range(1, len(g["iters"])):
        T = T + dt
        idx, val, moving = prog.step(T)
        bp, xp = MD.post_update(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape, g[f"b{k - 1}"],
                                g[f"xout{k - 1}"])
        got = {}
        for rule in ("reference", "all"):
            with E.EC3DSolver() as s:
                _assemble(s, g)
                s.set_u_rhs(rule)
                s.upload("B", g[f"b{k - 1}"])
                s.upload("X", g[f"xout{k - 1}"])
                s.post_update()
                s.rhs_step(idx, val, moving=moving)
                got[rule] = s.download("B")
            want = MD.rhs_step(g["irow"], g["jcol"], g["valA"], g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape,
                               bp, xp, idx, val, moving, rule=rule)
            assert np.array_equal(got[rule], want), (rule, k)
        assert np.array_equal(got["reference"], g[f"b{k}"])
        assert np.array_equal(got["reference"][:3 * N + nmax], got["all"][:3 * N + nmax])
        differ += int(np.count_nonzero(got["reference"] != got["all"]))
    print(f"{case}: U rows whose right-hand side differs between the rules, summed over the steps: {differ}")
    assert differ > 0


@pytest.mark.timeout(600)
@pytest.mark.parametrize("D", [22, 23])
def test_class_count_limit(E, oracle, D, tmp_path):
    """22 stacked blocks: structured with 253 classes; 23 (262 classes would not fit the class byte): bands + tail.
    Both: export_csr equal to the bands + tail export, SpMV equal to the oracle's, and a 5-step host.run converging
    below tol on every step."""
    from eddy_currents_3d_amd import host, vxc
    vox, names = MD.blocks_model(D)
    model = vxc.VxcModel(vox, names, 0.004, (1.0, 1.0, 1.0))
    t = vxc.domain_tables(model)
    with E.EC3DSolver(structured=False) as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        valA, irow, jcol = s.export_csr()
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        _check_matrix(s, valA, irow, jcol, oracle, D, D <= 22)
        res = []
        log = host.run(model, s, steps=5, on_solved=lambda k, s, info: res.append(s.true_residual()[0]))
    assert len(log) == 5 and all(i["iter"] <= int(t["itmax"]) for i in log), log
    assert all(r < float(t["tol"]) for r in res), res


@pytest.mark.parametrize("D", [4, 5])
def test_block_mg_domain_limit(E, D):
    """The block smoothers' table holds 64 classes: 4 conducting domains (63 A-row classes) are accepted, 5 (72) are
    refused with EC3D_PRECOND_E_MATRIX and the handle keeps solving unpreconditioned, as a fresh one does."""
    from eddy_currents_3d_amd import vxc
    from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX
    vox, names = MD.blocks_model(D)
    t = vxc.domain_tables(vxc.VxcModel(vox, names, 0.004, (1.0, 1.0, 1.0)))
    args = (t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
    r = np.random.Generator(np.random.PCG64(7)).standard_normal(3 * vox.size + int(t["ncells0"]))
    with E.EC3DSolver() as s:
        s.assemble(*args)
        assert s.info.tail_rows == 0 and s.info.dict_classes == 55 + 9 * D
        if D <= 4:
            s.set_preconditioner("block-mg")
            assert s.preconditioner()[0] == "block-mg"
            return
        with pytest.raises(E.EC3DError) as e:
            s.set_preconditioner("block-mg")
        assert e.value.status == PRECOND_E_MATRIX and "4" in str(e.value)
        assert s.preconditioner()[0] == "none"
        x, it, _ = s.solve(r, np.zeros_like(r), 1e-6, 300)
    with E.EC3DSolver() as s:
        s.assemble(*args)
        x0, it0, _ = s.solve(r, np.zeros_like(r), 1e-6, 300)
    assert it == it0 and np.array_equal(x, x0)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", ["g8a", "g8b"])
def test_block_mg(E, oracle, case):
    g = load_golden(G8[case])
    tol, itmax = float(g["tol"]), int(g["itmax"])
    sdz, sdy, sdx = g["geoPHYS"].shape
    with E.EC3DSolver() as s:
        _assemble(s, g)
        s.set_preconditioner("block-mg")
        twin = AV.AVMG.from_solver(s, (sdx, sdy, sdz))
        r = np.random.Generator(np.random.PCG64(3)).standard_normal(s.n)
        assert np.array_equal(s.precond_apply(r), twin.apply(r))
        for k in range(len(g["iters"])):
            b = g[f"b{k}"]
            x, it, _ = s.solve(b, g[f"xin{k}"], tol, itmax)
            rel = np.linalg.norm(b - oracle.spmv_csr(g["valA"], g["irow"], g["jcol"], x)) / np.linalg.norm(b)
            print(f"{case} step {k}: block-mg {it} iterations, reference {int(g['iters'][k])}, true residual {rel:.2e}")
            assert rel < tol and it < int(g["iters"][k])


def test_slab_and_multi_still_refuse_several_domains(E):
    g = load_golden(G8["g8b"])
    sdz = g["geoPHYS"].shape[0]
    geo = g["geoPHYS"][:9].copy()                     # planes [0, 9): owned [0, 7) + 2 halo planes, both domains
    geoC = np.zeros(geo.shape, np.int32)
    q = np.concatenate([np.flatnonzero((geo.reshape(-1) == d) & (g["geoPHYS_C"][:9].reshape(-1) != 0))
                        for d in (1, 2)])             # local, domain-major
    geoC.reshape(-1)[q] = 3 * geo.size + 1 + np.arange(len(q))
    with E.EC3DSolver() as s:
        s.assemble_slab(sdz, 0, 9, 0, 7, geo, geoC, g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        s.upload("B", np.zeros(s.n))
        s.upload("X", np.zeros(s.n))
        with pytest.raises(E.EC3DError) as e:
            s.rhs_step(np.zeros(0, np.int32), np.zeros(0))
        assert e.value.status == 5 and "slab" in str(e.value)
        with pytest.raises(E.EC3DError) as e:
            s.post_update()
        assert e.value.status == 5
    with E.EC3DMulti(2, devices=[0, 0]) as m:
        m.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
        with pytest.raises(E.EC3DError) as e:
            m.rhs_step(np.zeros(0, np.int32), np.zeros(0))
        assert e.value.status == 5
