"""What the generated A-V tests (tests/test_gpu_generated_av.py) lean on, pinned on the host before any GPU test
uses it: the captures g9a / g9b (six distinct boundary values, two moving domains, an L-shaped conductor with a hole
next to the box faces; tools/make_multidomain_goldens.py), the restatements of the per-step vectors
(tests/multidomain_numpy.py) and of the field file's vectors (tests/fields_numpy.py), and the generated corpus
(tests/av_generate.py) with the conditions it must meet."""
import re

import numpy as np
import pytest

import av_generate as AG
import fields_numpy as FN
import multidomain_numpy as MD
from conftest import load_golden

G9 = {"g9a": "g9a_two_moving_mixed_bnd_20x16x14", "g9b": "g9b_L_hole_near_faces_17x16x16"}
BND9 = np.array([[-0.95, 0.5], [-1.0, 1.5], [0.0, -0.25]])


def model_of(g):
    from eddy_currents_3d_amd import vxc
    return vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                        tuple(float(x) for x in g["adj"]))


def oracle_code(oracle, args):
    """0 where the oracle assembles, else the code of the STOP the reference would take."""
    try:
        oracle.gen_sparse_matrix(*args)
        return 0
    except RuntimeError as e:
        return int(re.search(r"code (\d+)", str(e)).group(1))


def recovered_sources(g, k, moving):
    """The step's source ids and values read back from the captured b (fixtures without their palette): coil cells
    lie in air, where Jaf holds nothing but the source value."""
    vox = g["vox"].reshape(-1)
    ncell = vox.size
    b = g[f"b{k}"]
    if moving:
        mask = np.ones(3 * ncell, bool)
        for c in range(3):
            mask[c * ncell + np.flatnonzero(vox == 1)] = False
        idx = np.flatnonzero(mask & (b[:3 * ncell] != 0.0))
    else:
        idx = np.concatenate([np.flatnonzero(np.isin(vox, (2, 3))), ncell + np.flatnonzero(np.isin(vox, (4, 5)))])
    return (idx + 1).astype(np.int32), b[idx]


@pytest.mark.parametrize("case", sorted(G9))
def test_g9_tables_and_oracle_csr(oracle, case):
    """vxc.domain_tables reads the boundary record, the lattice factors and the velocities as the reference did, the
    six boundary values are distinct with one 0, and oracle.gen_sparse_matrix equals the captured CSR bit for bit."""
    from eddy_currents_3d_amd import vxc
    g = load_golden(G9[case])
    t = vxc.domain_tables(model_of(g))
    assert np.array_equal(g["BND"], BND9) and len(set(g["BND"].reshape(-1))) == 6 and 0.0 in g["BND"]
    for key in ("geoPHYS", "geoPHYS_C", "valPHYS", "BND", "delta"):
        assert np.array_equal(np.asarray(t[key]).reshape(-1), np.asarray(g[key]).reshape(-1)), key
    assert t["dt"] == float(g["dt"]) and len(set(g["delta"])) == 3
    m = oracle.gen_sparse_matrix(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
    assert np.array_equal(m["irow"], g["irow"]) and np.array_equal(m["jcol"], g["jcol"])
    assert np.array_equal(m["valA"], g["valA"])
    assert np.count_nonzero(g["valA"] == 0.0) > 0                   # BZM = 0: the reference stores explicit zeros
    assert all(int(i) <= int(g["itmax"]) for i in g["iters"])       # converged on every step
    doms = MD.conductors(g["geoPHYS"], g["geoPHYS_C"])
    assert MD.structured_applies(g["geoPHYS"], g["geoPHYS_C"])
    if case == "g9a":
        v = [tuple(g["valPHYS"][d - 1, 2:5]) for d, _ in doms]
        assert len(doms) == 2 and v[0] != v[1] and all(np.all(np.asarray(w) != 0.0) for w in v)
        assert all(min(w) < 0.0 < max(w) for w in v) and g["valPHYS"][0, 1] != g["valPHYS"][1, 1]
    else:
        from eddy_currents_3d_amd.dist import slab_bounds
        assert len(doms) == 1
        on = g["geoPHYS_C"] != 0
        ks = np.flatnonzero(on.any(axis=(1, 2)))
        faces = {int(ks[0]), int(ks[-1]) + 1}                       # planes where the conductor begins / has ended
        sdz = on.shape[0]
        cuts = {slab_bounds(sdz, r, w)[0] for w in (2, 3) for r in range(1, w)}
        assert cuts & faces and any(abs(c - f) == 1 for c in cuts for f in faces)
        js, is_ = np.flatnonzero(on.any(axis=(0, 2))), np.flatnonzero(on.any(axis=(0, 1)))
        assert is_[0] == 1 and js[-1] == on.shape[1] - 2            # one cell from the low-x and the high-y face
        plane = on[ks[0]]
        filled = np.zeros_like(plane)
        filled[js[0]:js[-1] + 1, is_[0]:is_[-1] + 1] = True
        assert np.count_nonzero(filled & ~plane) > 1                # a concave step and a hole


@pytest.mark.parametrize("name", ["g9a", "g9b", "g2v_conducting_moving_16x15x14", "g3_moving_coil_18x16x12"])
def test_restatement_rebuilds_every_captured_b_and_x_in(name):
    g = load_golden(G9.get(name, name))
    shape, dt = g["vox"].shape, float(g["dt"])
    prog = None
    if name in G9:
        from eddy_currents_3d_amd import host, vxc
        model = model_of(g)
        prog = host.SourceProgram(model, vxc.domain_tables(model))
    b = np.zeros(len(g["irow"]) - 1)
    x = np.zeros_like(b)
    T = 0.0
    for k in range(len(g["iters"])):
        if prog is not None:
            idx, val, moving = prog.step(T)
        else:
            moving = name.startswith("g3")
            idx, val = recovered_sources(g, k, moving)
        assert np.array_equal(x, g[f"xin{k}"]), f"x_in of step {k}"
        bk = MD.rhs_step(g["irow"], g["jcol"], g["valA"], g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape, b, x,
                         idx, val, moving)
        assert np.array_equal(bk, g[f"b{k}"]), f"b of step {k}"
        b, x = MD.post_update(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape, g[f"b{k}"], g[f"xout{k}"])
        T = T + dt


def captured_field_files(g):
    """[(step k whose x_out / b the file shows, the file's bytes)]: field_N.vtk is written after step k = N's
    post-update (N counts from 0 like the captured calls)."""
    out = []
    for key in g.files:
        m = re.fullmatch(r"vtk_field_(\d+)", key)
        if m and f"xout{int(m.group(1))}" in g.files:
            out.append((int(m.group(1)), g[key].tobytes()))
    return sorted(out)


@pytest.mark.parametrize("name", ["g1_nonconducting_8x7x6", "g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12",
                                  "g9a", "g9b"])
def test_field_restatement_reproduces_the_captured_files(name):
    from eddy_currents_3d_amd.vtk import field_vtk_bytes
    g = load_golden(G9.get(name, name))
    sdz, sdy, sdx = g["geoPHYS"].shape
    files = captured_field_files(g)
    assert files
    for k, ref in files:
        b, x = MD.post_update(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], float(g["dt"]), g["geoPHYS"].shape,
                              g[f"b{k}"], g[f"xout{k}"])
        f = FN.fields(g["geoPHYS_C"], g["delta"], x, b)
        assert field_vtk_bytes(sdx, sdy, sdz, g["delta"], f) == ref, f"field_{k}.vtk"


def corpus(oracle):
    """[(seed, args, code)] of the committed seed list."""
    out = []
    for seed in AG.CORPUS:
        args = AG.generate(seed)
        out.append((seed, args, oracle_code(oracle, args)))
    return out


def test_generator_is_deterministic_and_varied():
    for seed in AG.CORPUS[:10]:
        a, b = AG.generate(seed), AG.generate(seed)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    shapes = [AG.generate(s)[0].shape for s in AG.CORPUS]
    sizes = {v for sh in shapes for v in sh}
    assert min(sizes) >= 7 and max(sizes) <= 24 and any(v % 2 for v in sizes) and any(v % 2 == 0 for v in sizes)
    bnd = np.concatenate([AG.generate(s)[3].reshape(-1) for s in AG.CORPUS])
    assert {0.0, 1.0, -1.0, 0.5} <= set(bnd)
    for seed in AG.CORPUS:
        geo, geoC, valPHYS, BND, delta, dt = AG.generate(seed)
        N = geo.size
        doms = MD.conductors(geo, geoC)
        ids = np.concatenate([geoC.reshape(-1)[c] for _, c in doms]) if doms else np.zeros(0, np.int64)
        assert np.array_equal(ids, 3 * N + 1 + np.arange(len(ids)))          # domain-major, scan order within
        assert [d for d, _ in doms] == sorted(d for d, _ in doms) and len(doms) <= 4
        assert geo.min() >= 1 and geo.max() == valPHYS.shape[0]
        assert all(valPHYS[d - 1, 1] != 0.0 for d, _ in doms)


def test_corpus_conditions(oracle):
    members = corpus(oracle)
    accepted = [(s, a) for s, a, c in members if c == 0]
    scan = [s for s, a in accepted if MD.structured_applies(a[0], a[1])]
    two_moving = [s for s, a in accepted if len(set(AG.moving_domains(*a[:3]))) >= 2]
    codes = [c for _, _, c in members]
    print(f"corpus: {len(members)} seeds, {len(accepted)} accepted ({len(scan)} in scan order, "
          f"{len(two_moving)} with two differently moving domains), refused with code 1: {codes.count(1)}, "
          f"2: {codes.count(2)}, 3: {codes.count(3)}")
    assert len(accepted) >= 40 and len(scan) >= 15 and len(accepted) - len(scan) >= 15 and len(two_moving) >= 10
    assert codes.count(1) >= 10 and codes.count(3) >= 3
    pats, acls = set(), set()
    for _, a in accepted:
        pats |= AG.u_row_patterns(a[1])
        acls |= AG.a_row_classes(a[1])
    assert pats == set(range(27)) and 1 + 3 * 2 + 9 * 2 in pats
    assert acls == {(d, p) for d in range(3) for p in (1, 2, 3)}
    one_domain = [s for s, a in accepted if len(MD.conductors(a[0], a[1])) == 1]
    assert len(one_domain) >= 5                                                # the slab tests' share


DEFECT_CODES = {k: (3 if k.startswith(("on_face", "third_outside")) else 1) for k in AG.DEFECTS}


@pytest.mark.parametrize("kind", AG.DEFECTS)
def test_every_single_defect_is_refused(oracle, kind):
    assert oracle_code(oracle, AG.single_defect(kind)) == DEFECT_CODES[kind]


@pytest.mark.parametrize("axis", "xyz")
@pytest.mark.parametrize("side", "mp")
def test_near_face_is_accepted(oracle, axis, side):
    geo, geoC, *_ = args = AG.near_face(axis, side)
    assert oracle_code(oracle, args) == 0
    on = np.flatnonzero((geoC != 0).any(axis=tuple(a for a in range(3) if a != AG._AX[axis])))
    assert (on[0] == 1) if side == "m" else (on[-1] == geo.shape[AG._AX[axis]] - 2)
