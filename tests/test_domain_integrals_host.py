"""CPU-only: the twin of ec3d_domain_integrals (tests/domain_integrals_numpy.py) against a case with a closed form,
the new entry point in the header, the binding and the built library, the geometry tests/test_gpu_domain_integrals.py
cuts its chunks on, and the CSV of ``python -m eddy_currents_3d_amd.run --integrals``."""
import os
import re
import subprocess

import numpy as np
import pytest

import av_generate as AG
import domain_integrals_numpy as DI
from conftest import REPO

CSV_HEADER = "step,T,domain,cells,joule_w,force_x,force_y,force_z"


def chunk_edge_geometry():
    """40 x 36 x 30 cells, non-conducting solid 2 and the conducting domains 3, 1, 4 (palette order, so a domain's id is
    not its ordinal): boxes at least 3 cells thick, at least 2 cells from every face and from each other, of
    22 x 20 x 11 = 4840 = 18 * 256 + 232 cells (four full 1024-entry chunks and a tail that ends inside a wave),
    3 x 3 x 3 = 27 (less than one wave) and 16 x 8 x 8 = 1024 (exactly one chunk).  The smallest input where a chunk
    tail, a full chunk and a sub-wave domain occur together."""
    vox = np.zeros((30, 36, 40), np.uint8)                  # [k, j, i]
    vox[2:13, 2:22, 2:24] = 3
    vox[16:19, 14:17, 28:31] = 1
    vox[16:24, 2:10, 2:18] = 4
    vox[26:28, 26:30, 30:36] = 2
    C = {3: AG.MU0 * 35.26e6, 1: AG.MU0 * 58.0e6, 4: AG.MU0 * 10.0e6}
    vel = {d: np.zeros(3) for d in C}
    return AG._tables(vox, [3, 1, 4], C, vel, (-0.95, 0.5, -1.0, 1.5, 0.0, -0.25), (0.004, 0.005, 0.003), 1e-3)


def test_chunk_edge_geometry_is_what_the_gpu_test_needs(oracle):
    geo, geoC, valPHYS, BND, delta, dt = chunk_edge_geometry()
    assert geo.shape == (30, 36, 40)
    cond = geoC != 0
    assert {int(d): int((cond & (geo == d)).sum()) for d in (1, 3, 4)} == {1: 27, 3: 4840, 4: 1024}
    assert not cond[geo == 2].any() and 4840 == 18 * 256 + 232
    assert len({valPHYS[d - 1, 1] for d in (1, 3, 4)}) == 3
    m = oracle.gen_sparse_matrix(geo, geoC, valPHYS, BND, delta, dt)      # the reference accepts it
    assert m["n"] == 3 * geo.size + 4840 + 27 + 1024


def test_twin_gives_the_closed_form_on_uniform_fields():
    """Constant Jaf on a box conductor and A linear in the coordinates: B = curl A is uniform, so the force is
    J x B * volume and the loss |J|^2 * volume / sigma.  Spacings are powers of two and the gradients small integers, so
    every A value and every difference is exact; what is left is the rounding of the products, far inside 1e-13."""
    sdz, sdy, sdx = 9, 10, 11
    delta = np.array([2.0 ** -8, 2.0 ** -7, 2.0 ** -9])
    G = np.array([[3.0, -2.0, 5.0], [7.0, 1.0, -4.0], [-6.0, 9.0, 2.0]])    # G[c, a] = d A_c / d x_a
    k, j, i = np.meshgrid(np.arange(sdz), np.arange(sdy), np.arange(sdx), indexing="ij")
    pos = [i * delta[0], j * delta[1], k * delta[2]]
    N = sdz * sdy * sdx
    vox = np.zeros((sdz, sdy, sdx), np.uint8)
    vox[2:6, 3:8, 2:9] = 2                                                  # away from the faces: no clamped difference
    geo, geoC, valPHYS, _, _, _ = AG._tables(vox, [2], {2: AG.MU0 * 35.26e6}, {2: np.zeros(3)}, [0.0] * 6, delta, 1e-3)
    ncond = int((geoC != 0).sum())
    x = np.zeros(3 * N + ncond)
    b = np.zeros(3 * N + ncond)
    jaf = np.array([0.25, -1.5, 0.75])
    for c in range(3):
        x[c * N:(c + 1) * N] = sum(G[c, a] * pos[a] for a in range(3)).reshape(-1)
        b[c * N:(c + 1) * N] = jaf[c]
    B = np.array([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
    J = DI.SIGMA_SCALE * -jaf
    volume = ncond * float(np.prod(delta))
    sigma = 35.26e6 * AG.MU0 * DI.SIGMA_SCALE
    (r,) = DI.integrals(geo, geoC, valPHYS, delta, x, b)
    assert r["domain"] == 2 and r["cells"] == ncond == 4 * 5 * 7 and r["sigma"] == sigma
    assert np.abs(r["force_n"] - np.cross(J, B) * volume).max() <= 1e-13 * np.abs(np.cross(J, B) * volume).max()
    assert abs(r["joule_w"] - J @ J * volume / sigma) <= 1e-13 * (J @ J * volume / sigma)
    assert r["joule_w"] > 0 and np.all(r["abs"][1:] >= np.abs(r["force_n"]))


def test_twin_groups_by_domain_id():
    """Two domains with different fields: each record holds its own cells only, in ascending id order."""
    geo, geoC, valPHYS, BND, delta, dt = chunk_edge_geometry()
    N = geo.size
    n = 3 * N + int((geoC != 0).sum())
    rng = np.random.Generator(np.random.PCG64(7))
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    recs = DI.integrals(geo, geoC, valPHYS, delta, x, b)
    assert [r["domain"] for r in recs] == [1, 3, 4] and [r["cells"] for r in recs] == [27, 4840, 1024]
    b2 = b.copy()
    for c in range(3):                                  # the current of domain 3 doubled: its loss x 4, the others' unchanged
        b2[c * N + np.flatnonzero(geo.reshape(-1) == 3)] *= 2.0
    recs2 = DI.integrals(geo, geoC, valPHYS, delta, x, b2)
    assert recs2[0]["joule_w"] == recs[0]["joule_w"] and recs2[2]["joule_w"] == recs[2]["joule_w"]
    assert recs2[1]["joule_w"] == pytest.approx(4.0 * recs[1]["joule_w"], rel=1e-14)


def test_header_binding_and_library_have_the_entry_point():
    txt = open(os.path.join(REPO, "include", "ec3d_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+ec3d_domain_integrals\s*\(\s*ec3d_handle\s+h\s*,\s*const\s+double\s*\*\s*delta\s*,\s*int32_t\s+cap"
                     r"\s*,\s*int32_t\s*\*\s*ndomains\s*,\s*ec3d_domain_integral\s*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"\}\s*ec3d_domain_integral\s*;", txt)
    from eddy_currents_3d_amd import build
    build.build()
    from eddy_currents_3d_amd.solver import EXPORTS, LIBPATH, DomainIntegral, EC3DMulti, EC3DSolver
    import ctypes as C
    assert "ec3d_domain_integrals" in EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", LIBPATH], check=True, capture_output=True, text=True).stdout
    assert "ec3d_domain_integrals" in set(re.findall(r" T (\w+)", nm))
    assert C.sizeof(DomainIntegral) == 56 and DomainIntegral.force_n.offset == 32      # the struct of the header
    assert hasattr(EC3DSolver, "domain_integrals") and not hasattr(EC3DMulti, "domain_integrals")


def test_struct_layout_in_c(tmp_path):
    """The header's struct as a C compiler lays it out: 56 bytes, no padding but the named one."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "ec3d_hip.h"\n'
                   "typedef char size_is_56[sizeof(ec3d_domain_integral) == 56 ? 1 : -1];\n"
                   "typedef char cells_at_8[offsetof(ec3d_domain_integral, cells) == 8 ? 1 : -1];\n"
                   "typedef char force_at_32[offsetof(ec3d_domain_integral, force_n) == 32 ? 1 : -1];\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only",
                        "-I", os.path.join(REPO, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_run_parses_integrals_and_writes_the_csv(tmp_path):
    from eddy_currents_3d_amd import run
    a = run.build_parser().parse_args(["model.vxc", "--integrals", str(tmp_path / "i.csv")])
    assert a.integrals == str(tmp_path / "i.csv")
    assert run.build_parser().parse_args(["model.vxc"]).integrals is None
    assert run.INTEGRALS_HEADER == CSV_HEADER
    recs = [dict(domain=1, cells=27, sigma=5.8e7, joule_w=0.1, force_n=np.array([1.0 / 3.0, -2e-17, 3.5e10])),
            dict(domain=4, cells=1024, sigma=1e7, joule_w=7.0, force_n=np.array([0.0, 1.0, -1.0]))]
    lines = run.integrals_rows(2, 0.002, recs)
    assert lines == ["2,0.002,1,27,0.1,0.3333333333333333,-2e-17,35000000000.0", "2,0.002,4,1024,7.0,0.0,1.0,-1.0"]
    for line, r in zip(lines, recs):                    # repr() precision: the floats read back to the same bits
        f = line.split(",")
        assert float(f[4]) == r["joule_w"] and [float(v) for v in f[5:]] == r["force_n"].tolist()
    assert run.integrals_rows(0, 0.0, []) == []


def test_run_refuses_integrals_on_several_ranks(monkeypatch, capsys):
    from eddy_currents_3d_amd import run
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        run.main(["model.vxc", "--integrals", "i.csv"])
    assert e.value.code == 2 and "--integrals runs on one GPU only" in capsys.readouterr().err
