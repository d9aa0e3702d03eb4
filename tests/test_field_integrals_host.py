"""CPU-only: the twin of ec3d_field_energy and ec3d_domain_linkage (tests/field_integrals_numpy.py) against a field with a
closed form and against tests/fields_numpy.py, its ordered sums against exact ones, its domain lists, the entry points in
the header, the binding and the built library, and the CSV of ``python -m eddy_currents_3d_amd.run --energy``."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import av_generate as AG
import field_integrals_numpy as FI
import fields_numpy
from conftest import REPO, load_golden

CSV_HEADER = "step,T,energy_b,aj_source,aj_eddy"


def two_coil_model():
    """22 x 12 x 10 cells: a conducting plate (domain 2) in the middle, the non-conducting coils 1 and 3 -- 3 x 6 x 4 boxes
    mirrored in x about the box's mid-plane --, air is domain 4.  Built with av_generate._tables, which from_boxes
    calls: from_boxes itself makes every domain it is given a conductor."""
    vox = np.zeros((10, 12, 22), np.uint8)                  # [k, j, i]
    vox[3:7, 3:9, 2:5] = 1
    vox[3:7, 3:9, 17:20] = 3
    vox[3:7, 3:9, 8:14] = 2
    return AG._tables(vox, [2], {2: AG.MU0 * 35.26e6}, {2: np.zeros(3)}, (0.5, -0.95, 1.5, -1.0, -0.25, 0.0),
                      (0.004, 0.005, 0.003), 1e-3)


def mirrored_vectors(geo, geoC, seed=5):
    """(x, b) on two_coil_model: A antisymmetric under the mirror i -> sdx - 1 - i and constant along x inside a coil,
    Jaf = +I on coil 1 and -I on coil 3 (y component), zero elsewhere.  A coil's cells in scan order then carry the
    same sequence of terms A.J as the other's: the mirror reverses every grid row, and a row's three terms are equal."""
    sdz, sdy, sdx = geo.shape
    N = geo.size
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros(3 * N + int((geoC != 0).sum()))
    b = np.zeros_like(x)
    for c in range(3):
        f = rng.standard_normal(geo.shape)
        f[:, :, 2:5] = f[:, :, 2:3]
        f[:, :, sdx // 2:] = -f[:, :, :sdx // 2][:, :, ::-1]
        x[c * N:(c + 1) * N] = f.reshape(-1)
    jy = np.where(geo == 1, 0.37, np.where(geo == 3, -0.37, 0.0))
    b[N:2 * N] = jy.reshape(-1)
    return x, b


def test_uniform_field_has_the_closed_form():
    """A = (-B0 y/2, B0 x/2, 0) on 12 x 11 x 10 cells, spacings powers of two and B0 = 0.75: every A value, difference,
    quotient, square and partial sum is exact, so every interior cell has B = (0, 0, B0) exactly and the ordered sum is
    the real one; the scaling rounds three times, far inside 1e-14."""
    shape, delta, B0 = (10, 11, 12), np.array([2.0 ** -8, 2.0 ** -7, 2.0 ** -9]), 0.75
    x = FI.vector_potential(shape, delta, B0)
    bx, by, bz = FI.curl(delta, x, shape)
    assert not bx.any() and not by.any()
    assert np.all(bz[:, 1:-1, 1:-1] == B0)
    assert np.all(bz[:, 1:-1, [0, -1]] == 0.75 * B0) and np.all(bz[:, [0, -1], 1:-1] == 0.75 * B0)
    assert np.all(bz[:, [0, 0, -1, -1], [0, -1, 0, -1]] == 0.5 * B0)
    r = FI.field_energy(np.zeros(shape, np.int32), delta, x, np.zeros_like(x))
    want = FI.clamped_energy(shape, delta, B0)
    assert r["cells"] == 12 * 11 * 10
    assert abs(r["energy_b"] - want) <= 1e-14 * want
    assert r["energy_axis"][0] == 0.0 and r["energy_axis"][1] == 0.0 and r["energy_axis"][2] == r["energy_b"]
    assert r["aj_source"] == 0.0 and r["aj_eddy"] == 0.0


@pytest.mark.parametrize("name", ["g2_conducting_hole_16x15x14", "g3_moving_coil_18x16x12"])
def test_twin_b_is_the_field_outputs_b_before_rounding(name):
    g = load_golden(name)
    geoC = g["geoPHYS_C"]
    n = 3 * geoC.size + int((np.asarray(geoC) != 0).sum())
    rng = np.random.Generator(np.random.PCG64(3))
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    B = np.stack([v.reshape(-1) for v in FI.curl(g["delta"], x, geoC.shape)], axis=1)
    f = fields_numpy.fields(geoC, g["delta"], x, b)
    assert np.array_equal(B.astype(np.float32), f["B"])
    t = FI.cell_terms(geoC, g["delta"], x, b)
    assert np.array_equal(t["b2"], B * B)
    cond = t["cond"]
    assert np.array_equal(t["j"][cond].astype(np.float32), f["eddy"][cond])


@pytest.mark.parametrize("shape", [(6, 7, 8), (3, 30, 40), (5, 64, 96), (40, 64, 64)])
def test_ordered_sums_are_sums(shape):
    """Small integers sum exactly in any order: the streaming order and the list order drop and double nothing -- on one
    chunk per plane, on planes that end inside a chunk (1200 = 2 * 512 + 176 cells) and on planes of whole chunks."""
    rng = np.random.Generator(np.random.PCG64(11))
    v = rng.integers(-1000, 1000, size=int(np.prod(shape))).astype(np.float64)
    assert FI.stream_sum(v, shape) == v.sum()
    assert FI.list_sum(v) == v.sum()
    assert FI.list_sum(v[:1]) == v[0] and FI.list_sum(v[:1025]) == v[:1025].sum()


def test_streaming_order_wraps_past_1024_chunks():
    shape = (64, 96, 96)
    assert -(-96 * 96 // FI.TILE) * 64 == 1152 > FI.WGS
    rng = np.random.Generator(np.random.PCG64(12))
    v = rng.integers(-1000, 1000, size=int(np.prod(shape))).astype(np.float64)
    assert FI.stream_sum(v, shape) == v.sum()
    w = rng.standard_normal(v.size)
    assert abs(FI.stream_sum(w, shape) - math.fsum(w.tolist())) <= 64 * 2.0 ** -53 * np.abs(w).sum()


@pytest.mark.parametrize("case", ["g3", "two_coils"])
def test_linkage_lists(case):
    if case == "g3":
        g = load_golden("g3_moving_coil_18x16x12")
        geo, geoC, delta = g["geoPHYS"], g["geoPHYS_C"], g["delta"]
    else:
        geo, geoC, _, _, delta, _ = two_coil_model()
    n = 3 * geo.size + int((np.asarray(geoC) != 0).sum())
    rng = np.random.Generator(np.random.PCG64(4))
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    recs = FI.domain_linkage(geo, geoC, delta, x, b)
    ids = [r["domain"] for r in recs]
    assert ids == sorted(ids) and len(set(ids)) == len(ids)
    count = np.bincount(np.asarray(geo).reshape(-1)[np.asarray(geoC).reshape(-1) == 0].astype(np.int64))
    assert [(r["domain"], r["cells"]) for r in recs] == [(d, int(c)) for d, c in enumerate(count) if c]
    assert FI.linkage_lists(geo, geoC) == [(r["domain"], r["cells"]) for r in recs]
    conducting = set(np.asarray(geo).reshape(-1)[np.asarray(geoC).reshape(-1) != 0].tolist())
    assert conducting and not conducting & set(ids)
    if case == "two_coils":
        assert [(r["domain"], r["cells"]) for r in recs] == [(1, 72), (3, 72), (4, 22 * 12 * 10 - 72 * 2 - 144)]
    # the lists and the conductor cells make up the box: the linkages and aj_eddy are the whole of A.J
    e = FI.field_energy(geoC, delta, x, b)
    t = FI.cell_terms(geoC, delta, x, b)
    vol = float(np.prod(delta))
    scale = vol * np.abs(t["a"]).sum()
    assert abs(sum(r["linkage"] for r in recs) - e["aj_source"]) <= 1e-12 * scale
    assert abs(e["aj_source"] + e["aj_eddy"] - vol * math.fsum(t["a"].tolist())) <= 1e-12 * scale


def test_mirrored_coils_have_equal_linkage():
    geo, geoC, _, _, delta, _ = two_coil_model()
    x, b = mirrored_vectors(geo, geoC)
    r = {q["domain"]: q for q in FI.domain_linkage(geo, geoC, delta, x, b)}
    assert r[1]["linkage"] != 0.0 and r[1]["linkage"] == r[3]["linkage"]
    assert np.array_equal(r[1]["jsum"], -r[3]["jsum"]) and r[1]["jsum"][1] != 0.0
    assert r[4]["linkage"] == 0.0 and not r[4]["jsum"].any()


def test_header_binding_and_library_have_the_entry_points():
    txt = open(os.path.join(REPO, "include", "ec3d_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+ec3d_field_energy\s*\(\s*ec3d_handle\s+h\s*,\s*const\s+double\s*\*\s*delta\s*,"
                     r"\s*ec3d_field_energy_info\s*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"\bint\s+ec3d_domain_linkage\s*\(\s*ec3d_handle\s+h\s*,\s*const\s+double\s*\*\s*delta\s*,\s*int32_t\s+cap"
                     r"\s*,\s*int32_t\s*\*\s*ndomains\s*,\s*ec3d_domain_link\s*\*\s*out\s*\)\s*;", txt)
    from eddy_currents_3d_amd import build
    build.build()
    from eddy_currents_3d_amd import host, solver
    import ctypes as C
    nm = subprocess.run(["nm", "-D", "--defined-only", solver.LIBPATH], check=True, capture_output=True, text=True).stdout
    for name in ("ec3d_field_energy", "ec3d_domain_linkage"):
        assert name in solver.EXPORTS and name in set(re.findall(r" T (\w+)", nm))
    assert C.sizeof(solver.FieldEnergy) == 56 and solver.FieldEnergy.aj_source.offset == 40
    assert C.sizeof(solver.DomainLink) == 48 and solver.DomainLink.jsum.offset == 24
    for m in ("field_energy", "domain_linkage"):
        assert hasattr(solver.EC3DSolver, m) and not hasattr(solver.EC3DMulti, m)
    assert inspect.signature(host.run).parameters["energy"].default is False
    assert inspect.signature(host.run_slabs).parameters["energy"].default is False
    f90 = open(os.path.join(REPO, "eddy_currents_3d_amd", "fortran", "ec3d_hip_mod.f90")).read()
    for name in ("ec3d_field_energy", "ec3d_domain_linkage"):
        assert f'bind(C, name="{name}")' in f90 and re.search(r"public ::.*?\b" + name + r"\b", f90, flags=re.S), name


def test_struct_layouts_in_c(tmp_path):
    """The header's structs as a C compiler lays them out: no padding but the named one; the header is strict C99."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "ec3d_hip.h"\n'
                   "typedef char e_is_56[sizeof(ec3d_field_energy_info) == 56 ? 1 : -1];\n"
                   "typedef char axis_at_16[offsetof(ec3d_field_energy_info, energy_axis) == 16 ? 1 : -1];\n"
                   "typedef char src_at_40[offsetof(ec3d_field_energy_info, aj_source) == 40 ? 1 : -1];\n"
                   "typedef char l_is_48[sizeof(ec3d_domain_link) == 48 ? 1 : -1];\n"
                   "typedef char cells_at_8[offsetof(ec3d_domain_link, cells) == 8 ? 1 : -1];\n"
                   "typedef char jsum_at_24[offsetof(ec3d_domain_link, jsum) == 24 ? 1 : -1];\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                        "-I", os.path.join(REPO, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_run_parses_energy_and_writes_the_csv(tmp_path):
    from eddy_currents_3d_amd import run
    a = run.build_parser().parse_args(["model.vxc", "--energy", str(tmp_path / "e.csv")])
    assert a.energy == str(tmp_path / "e.csv")
    assert run.build_parser().parse_args(["model.vxc"]).energy is None
    assert run.ENERGY_HEADER == CSV_HEADER and run.ENERGY_HEADER != run.INTEGRALS_HEADER
    e = dict(cells=10, energy_b=1.0 / 3.0, energy_axis=np.zeros(3), aj_source=-2e-17, aj_eddy=3.5e10)
    link = [dict(domain=1, cells=72, linkage=0.1, jsum=np.zeros(3)), dict(domain=4, cells=5, linkage=-0.0, jsum=np.zeros(3))]
    assert run.energy_header(link) == CSV_HEADER + ",linkage_1,linkage_4"
    line = run.energy_row(2, 0.002, e, link)
    assert line == "2,0.002,0.3333333333333333,-2e-17,35000000000.0,0.1,-0.0"
    assert [float(v) for v in line.split(",")[2:]] == [e["energy_b"], e["aj_source"], e["aj_eddy"], 0.1, -0.0]
    assert run.energy_header([]) == CSV_HEADER


def test_run_refuses_energy_on_several_ranks(monkeypatch, capsys):
    from eddy_currents_3d_amd import run
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        run.main(["model.vxc", "--energy", "e.csv"])
    assert e.value.code == 2 and "--energy runs on one GPU only" in capsys.readouterr().err


def test_run_slabs_refuses_energy_before_assembling():
    from eddy_currents_3d_amd import host
    with pytest.raises(ValueError, match="energy"):
        host.run_slabs(None, 0, 2, energy=True)
