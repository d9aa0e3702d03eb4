"""CPU-only: the A-V recogniser (csrc/ec3d_sav_csr.cpp: ec3d_csr_to_sav_host, ec3d_sav_cuttable, ec3d_sav_slice) on the
CSR corpus of tests/av_csr_generate.py -- the reference's own multi-domain matrices, one-edit mutations of them and
"saturated" matrices that fill every slot the recogniser admits -- under the default plane pitch and with tile-aligned
planes forced (EC3D_PITCH=2).

* ec3d_probe_csr takes the decision the corpus states, with the member's dimensions, n_cond, pitch and class count.
* tests/support/sav_csr_cases.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers,
  expands every recognised form back to CSR from the form's definition and compares it with the input bit for bit,
  and checks every z-slab ec3d_sav_slice cuts for 2, 3 and 4 ranks.
* ec3d_probe_csr_multi cuts exactly what is recognised and has two planes per rank, and refuses a matrix whose A blocks
  couple across a component's z faces."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import av_csr_generate as G
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "sav_csr_cases.cpp")
TILE = 512
PITCHES = ("auto", "pitched")
RANKS = (2, 3, 4)
HALO = 2          # halo planes per interior side of a slab (ec3d_multi_set_matrix_csr)

CORPUS = G.corpus(O)
BY_NAME = {m.name: m for m in CORPUS}


@pytest.fixture(scope="module")
def E():
    from eddy_currents_3d_amd import build
    build.build()
    import eddy_currents_3d_amd as E
    return E


@pytest.fixture(params=PITCHES)
def pitch(request, monkeypatch):
    if request.param == "pitched":
        monkeypatch.setenv("EC3D_PITCH", "2")
    else:
        monkeypatch.delenv("EC3D_PITCH", raising=False)
    return PITCHES.index(request.param)


def default_pitch(m):
    """ec3d_ctx::pitch's rule: tile-aligned planes when that costs less than 1/16 in rows and there are 8 planes."""
    sdx, sdy, sdz = m.dims
    plane = sdx * sdy
    pp = -(-plane // TILE) * TILE
    return pp if (pp - plane) * 16 <= plane and sdz >= 8 else plane


_probe = {}


def probe(E, m, pitch):
    """(probe of m under this pitch); the environment is the fixture's."""
    if (m.name, pitch) not in _probe:
        _probe[m.name, pitch] = E.probe_csr(*m.csr)
    return _probe[m.name, pitch]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_probe_takes_the_stated_decision(E, pitch, name):
    m = BY_NAME[name]
    p = probe(E, m, pitch)
    assert bool(p.structured) == m.expect[pitch]
    if not p.structured:
        return
    sdx, sdy, sdz = m.dims
    assert (p.sdx, p.sdy, p.sdz, p.n_cond) == (sdx, sdy, sdz, m.n_cond)
    assert p.n_cond == m.n - 3 * sdx * sdy * sdz
    assert p.plane_pitch == (-(-sdx * sdy // TILE) * TILE if pitch else default_pitch(m))
    assert 1 < p.classes <= 256
    if m.family == "generated":
        assert p.classes <= 55 + 9 * max(m.D, 1)
    if m.family == "mutated" and m.dclasses is not None:
        assert p.classes == probe(E, BY_NAME[m.base], pitch).classes + m.dclasses


def test_class_bound_is_met_with_equality(E, monkeypatch):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    full = [m.name for m in CORPUS if m.family == "generated" and m.expect[0] and
            E.probe_csr(*m.csr).classes == 55 + 9 * max(m.D, 1)]
    assert {"seed3", "seed41", "seed63"} <= set(full)


def test_saturated_rule_under_tile_aligned_planes():
    """The corpus's expectation for EC3D_PITCH=2 is the rule itself: recognised exactly when no stored entry joins two
    planes other than straight along z.  Every admitted slot is present: 7 + 5 entries in an interior conducting A row,
    9 + 7 in an interior U row."""
    for m in CORPUS:
        if m.family != "saturated":
            continue
        sdx, sdy, sdz = m.dims
        on = np.zeros((sdz, sdy, sdx), bool)
        for (x0, x1), (y0, y1), (z0, z1) in m.extra["boxes"]:
            on[z0:z1, y0:y1, x0:x1] = True
        cells = np.flatnonzero(on.reshape(-1))
        assert len(cells) == m.n_cond
        assert m.expect == (True, not G.crosses_plane(m.csr, m.dims, cells))
        lens = np.diff(m.irow)
        nC = sdx * sdy * sdz
        assert lens[:3 * nC].max() == 12 and lens[3 * nC:].max() == 16
        r, c = G._rows(m.irow, m.jcol)
        assert np.all(np.diff(c)[np.diff(r) == 0] > 0)                        # ascending columns
        off = np.abs(np.where(r == c, 0.0, m.valA))
        diag = np.zeros(m.n)
        diag[r[r == c]] = m.valA[r == c]
        assert np.all(diag > np.bincount(r, off, m.n))                         # strictly diagonally dominant
        assert len(np.unique(m.valA)) <= 64
    wraps = {w: [m for m in CORPUS if m.wrap == w] for w in G.WRAPS}
    for a, b in zip(wraps["none"], wraps["x"]):
        assert len(b.valA) > len(a.valA)
    for a, b in zip(wraps["x"], wraps["all"]):
        assert len(b.valA) > len(a.valA)


def test_family_counts():
    gen = [m for m in CORPUS if m.family == "generated"]
    yes = [m for m in gen if m.expect[0]]
    assert len(yes) >= 35 and len(gen) - len(yes) >= 10
    assert sum(m.D >= 2 for m in yes) >= 10
    assert all(m.expect[0] == m.expect[1] for m in gen)
    bases = [BY_NAME[f"seed{s}"] for s in G.MUTATION_BASES]
    assert all(b.expect[0] for b in bases)
    assert [b.D for b in bases][:2] == [1, 2] and bases[2].D >= 3
    for mut in G.MUTATIONS:
        assert sum(m.mutation == mut for m in CORPUS) >= 3
    sat = [m for m in CORPUS if m.family == "saturated"]
    assert len(sat) >= 8 and {m.wrap for m in sat} == set(G.WRAPS)
    assert any(m.dims[0] % 2 for m in sat) and {(12, 10, 9), (16, 8, 10), (14, 9, 8)} <= {m.dims for m in sat}
    print(f"generated: {len(yes)} recognised ({sum(m.D >= 2 for m in yes)} with D >= 2), {len(gen) - len(yes)} not; "
          f"mutated: {sum(m.family == 'mutated' for m in CORPUS)}; saturated: {len(sat)}")


def cuttable(m, pitch, ranks):
    return m.expect[pitch] and m.dims[2] >= 2 * ranks and m.wrap != "all"


@pytest.mark.parametrize("ranks", [2, 4])
def test_generated_members_are_cut_when_recognised_and_tall_enough(E, pitch, ranks):
    """Cut exactly when recognised with two planes per rank.  One kind of member has a second reading: without a
    conductor the system is three uncoupled 7-point operators, i.e. ONE such operator on 3 sdz planes (the rows of a
    component's first and last plane are boundary rows), which ec3d_probe_csr_multi cuts plane by plane whenever the
    A-V reading is refused (tests/test_csr_recognition.py, test_which_matrices_can_be_cut_into_z_slabs).  So those
    members are cut when 3 sdz >= ranks; tests/test_gpu_av_csr.py multiplies one of them in four slabs."""
    seen = set()
    for m in CORPUS:
        if m.family != "generated":
            continue
        ok, why = E.probe_csr_multi(*m.csr, ranks)
        as_av = cuttable(m, pitch, ranks)
        as_cube = m.n_cond == 0 and 3 * m.dims[2] >= ranks
        assert ok == (as_av or as_cube), (m.name, why)
        seen.add((m.expect[pitch], as_av, ok))
        if not ok:
            assert ("two z-planes" in why) if m.expect[pitch] else ("not recognised" in why)
    assert (True, True, True) in seen and (False, False, False) in seen
    if ranks == 4:
        assert (True, False, True) in seen
    m = BY_NAME["seed3"]                            # 10 planes, one conductor: five slabs of two planes, not six
    assert m.dims[2] == 10 and m.n_cond > 0 and E.probe_csr_multi(*m.csr, 5)[0]
    ok, why = E.probe_csr_multi(*m.csr, 6)
    assert not ok and "two z-planes" in why


def test_coupling_across_the_z_faces_is_not_cut(E, monkeypatch):
    monkeypatch.delenv("EC3D_PITCH", raising=False)
    m = BY_NAME["sat_interior_12x10x9_all"]
    nC = int(np.prod(m.dims))
    r, c = G._rows(m.irow, m.jcol)
    assert np.any((r < nC) & (c >= nC) & (c < 2 * nC))          # A_x rows reach into A_y through +plane
    ok, why = E.probe_csr_multi(*m.csr, 2)
    assert not ok and "couples across" in why
    assert E.probe_csr_multi(*m.csr, 1)[0]
    assert E.probe_csr_multi(*BY_NAME["sat_interior_12x10x9_none"].csr, 2)[0]


# ------------------------------------------------------------------------------ the form itself, under sanitizers
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(cc)))
    exe = str(tmp_path_factory.mktemp("sav_csr") / "sav_csr_cases")
    subprocess.run([cc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-std=c++17", "-O1", "-g",
                    "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    return exe


def slices_of(sdz):
    from eddy_currents_3d_amd.dist import slab_bounds
    out = []
    for ranks in RANKS:
        for r in range(ranks):
            k0, k1 = slab_bounds(sdz, r, ranks)
            out.append((ranks, r, max(0, k0 - HALO), min(sdz, k1 + HALO), k0, k1))
    return np.array(out, np.int64)


@pytest.mark.parametrize("pitch_name", PITCHES)
def test_form_expands_to_the_input_and_slices_hold_their_planes(program, tmp_path, pitch_name):
    pitch = PITCHES.index(pitch_name)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for m in CORPUS:
            sl = slices_of(m.dims[2])
            f.write(np.array([m.n, len(m.jcol), len(sl)], np.int64).tobytes())
            f.write(np.ascontiguousarray(m.irow, np.int32).tobytes())
            f.write(np.ascontiguousarray(m.jcol, np.int32).tobytes())
            f.write(np.ascontiguousarray(m.valA, np.float64).tobytes())
            f.write(sl.tobytes())
    env = {k: v for k, v in os.environ.items() if k != "EC3D_PITCH"}
    if pitch:
        env["EC3D_PITCH"] = "2"
    out = subprocess.run([program, path], capture_output=True, text=True, env=env)
    assert out.stderr == "", out.stderr          # a sanitizer report
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and not [ln for ln in lines if ln.startswith("FAIL")], "\n".join(lines[-20:])
    assert lines[-1] == f"done {len(CORPUS)}" and len(lines) == len(CORPUS) + 1
    sliced = 0
    for i, (m, ln) in enumerate(zip(CORPUS, lines)):
        w = ln.split()
        assert w[:2] == ["case", str(i)] and w[2] == "structured" and w[4] == "classes" and w[6] == "pitch" and w[8] == "cut"
        assert int(w[3]) == m.expect[pitch], m.name
        assert [int(v) for v in w[9:]] == [r for r in RANKS if cuttable(m, pitch, r)], m.name
        sliced += len(w) - 9
    assert sliced >= 100
    zeros = [m for m in CORPUS if m.expect[pitch] and np.any(m.valA == 0.0)]
    assert len(zeros) >= 3 and any(m.mutation == "wrap_zero" for m in zeros)     # explicit zeros went through
