"""The interleaved z-march of the structured A-V kernels (csrc/ec3d_kernels.hip walk_zm_il) on grids of SEVERAL columns.

tests/test_gpu_interleaved.py forces the march onto the captured systems, whose plane is one 512-row tile: one column,
one word of U mask, every plane with a conductor setting the same bit.  The systems of tests/av_grids.py are the
smallest on which the rest of the march and of its host lists (csrc/ec3d_sweep_lists.hpp ec3d_il_umask,
ec3d_il_work_list) runs -- bit for bit against the oracle's assembly and CSR product and against the GPU-order twin:

  S1  64 x 72 x 40    9 columns, 2 mask words, two conducting domains (73 classes) with four planes of air between them
                      (the U tiles of columns 2 .. 7 stop at plane 14 and start again at 18), a through hole, column 0
                      without a U tile, the second domain across planes 31 / 32; +-sdx operands from the same tile or the next
  S2  1024 x 8 x 34   16 columns of half a grid row: x.pair(r +- sdx) lies two tiles away, the conductor crosses the tile
                      boundary at x = 512, eight columns hold no U tile
  S3  40 x 30 x 33    planes of 1200 cells in 1536 rows (EC3D_PITCH=2): tiles that start mid-row, one mostly padding

The form is forced as tests/test_gpu_interleaved.py forces it (EC3D_SAV_IL=2, EC3D_SAV_PATCH=0), every other launch knob
deleted first.  What a case is there for is asserted from the library's own account of its launch (visit_order, ulist), so
that a change to the list builder cannot quietly stop exercising it; tests/test_sweep_lists_host.py pins the same lists
on the host.  Every comparison is bit for bit, the true residual excepted (the bounds of test_gpu_interleaved.py)."""
import time

import numpy as np
import pytest

import av_grids as AGR
from oracle import oracle as O
from test_gpu_default_policies import no_knobs
from test_gpu_interleaved import check_visit_order

pytestmark = pytest.mark.gpu

POLICIES = {"nt0": {"EC3D_NT": "0"}, "nt1-keep0": {"EC3D_NT": "1", "EC3D_KEEP": "0"},
            "nt1-keep11": {"EC3D_NT": "1", "EC3D_KEEP": "11"}}
# What choose_sweep and ec3d_spare_pair (csrc/ec3d_context.hip) give the 256^3 A-V handle (rows streamed >= 32 Mi):
# nontemporal streams with nothing kept cacheable, X applied every fourth iteration, the vector kernels on the big plans
# (K2 768 workgroups, K4 and K5 256, plain tile map, two tiles in flight), five launches, the march's default request.
POLICY_256 = {"EC3D_NT": "1", "EC3D_KEEP": "0", "EC3D_XDEFER": "4",
              "EC3D_NBLK_K2": "768", "EC3D_MAP_K2": "0", "EC3D_DEPTH_K2": "2",
              "EC3D_NBLK_K4": "256", "EC3D_MAP_K4": "0", "EC3D_DEPTH_K4": "2",
              "EC3D_NBLK_K5": "256", "EC3D_MAP_K5": "0", "EC3D_DEPTH_K5": "2"}
REQUESTS = [("S1", None), ("S1", 16), ("S1", 64), ("S2", 40), ("S3", 8)]
BARE_COLUMNS = {"S1": {0}, "S2": {0, 1, 2, 3, 12, 13, 14, 15}, "S3": set()}


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def force(monkeypatch, name, nblk=None, env=None):
    no_knobs(monkeypatch)
    for k in ("EC3D_SAV_IL", "EC3D_XASYNC", "EC3D_SAV_PATCH_PX", *POLICY_256):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EC3D_SAV_IL", "2")
    monkeypatch.setenv("EC3D_SAV_PATCH", "0")
    if AGR.GRIDS[name]["pitched"]:
        monkeypatch.setenv("EC3D_PITCH", "2")
    if nblk is not None:
        monkeypatch.setenv("EC3D_NBLK_SPMV", str(nblk))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


_matrix = {}


def matrix_of(name):
    """The oracle's assembly (src/EC3D.f90:465-1049 restated): made once, read-only.  It accepts every system."""
    if name not in _matrix:
        m = O.gen_sparse_matrix(*AGR.system(name))
        for key in ("valA", "irow", "jcol"):
            m[key].setflags(write=False)
        _matrix[name] = m
    return _matrix[name]


def rhs_of(name):
    b = np.random.Generator(np.random.PCG64(2300 + len(name) + ord(name[1]))).standard_normal(matrix_of(name)["n"])
    b.setflags(write=False)
    return b


def build(s, name, route):
    if route == "csr":
        m = matrix_of(name)
        s.set_matrix_csr(m["valA"], m["irow"], m["jcol"])
    else:
        s.assemble(*AGR.system(name))
    D = len(AGR.GRIDS[name]["domains"])
    assert s.info.tail_rows == 0 and s.info.dict_classes == 55 + 9 * D          # the structured form
    assert s.geometry(1).ulist_n == 0 and s.fusion() == (0, 0)                   # the U tiles inside the march; five launches


def launch_features(s, name):
    """From visit_order(1) and ulist(): per workgroup its column and plane range, and what the launch exercises."""
    sdx, sdy, P = AGR.GRIDS[name]["dims"]
    g = s.geometry(1)
    off, tiles = s.visit_order(1)
    tpp, blk = int(g.zm_tpp), int(g.ntiles_front) // 3
    assert tpp == AGR.pitch_of(name) // AGR.TILE and blk == P * tpp
    ul = [int(t) for t in s.ulist()]
    assert ul == AGR.u_tiles(name)                                 # the device lists the U tiles the voxels give
    U = {(t // tpp - 3 * P, t % tpp) for t in ul}
    wgs = []
    for w in range(len(off) - 1):
        v = tiles[off[w]:off[w + 1]].astype(np.int64)
        ax = v[v < blk]
        if len(ax) == 0:
            assert len(v) == 0
            wgs.append(None)
            continue
        col, k0 = int(ax[0] % tpp), int(ax[0] // tpp)
        assert np.array_equal(ax, (k0 + np.arange(len(ax))) * tpp + col)        # one column, consecutive planes
        assert sorted(int(t) for t in v[v >= 3 * blk]) == [(3 * P + k) * tpp + col for k in range(k0, k0 + len(ax)) if (k, col) in U]
        wgs.append((col, k0, k0 + len(ax)))
    def bits(col, k0, k1):
        return "".join("1" if (k, col) in U else "0" for k in range(k0, k1))
    full = [w for w in wgs if w is not None]
    return dict(P=P, columns=len({w[0] for w in full}), bare={c for c in range(tpp) if not any((k, c) in U for k in range(P))},
                empty=sum(1 for w in wgs if w is None), workgroups=len(wgs),
                cuts_inside=sum(1 for c, k0, k1 in full if k0 > 0 and (k0, c) in U and (k0 - 1, c) in U),
                crossings=sum(1 for c, k0, k1 in full if k0 <= 31 and k1 > 32),
                u_dropped=sum(1 for c, k0, k1 in full if "10" in bits(c, k0, k1)),
                u_again=sum(1 for c, k0, k1 in full if "10" in bits(c, k0, k1) and "01" in bits(c, k0, k1)[bits(c, k0, k1).index("10"):]),
                words=-(-P // 32))


def check_features(s, name, nblk):
    f = launch_features(s, name)
    print(f"{name} nblk {nblk}: {f}")
    assert f["P"] > 32 and f["words"] >= 2 and f["columns"] == s.geometry(1).zm_tpp > 1
    assert f["bare"] == BARE_COLUMNS[name]                  # columns that run the copy of the step without U, all the way
    assert f["cuts_inside"] >= 1                            # a segment that starts with a U step behind another workgroup's
    assert f["empty"] >= 1 and f["crossings"] >= 1          # (k0 == k1) entries; ubit(k + 1) at k = 31 lands in word 1
    assert f["u_dropped"] >= 1                              # a U block asked for a step ahead and dropped
    if nblk is not None:                                    # the request the host test quotes: the same counts
        q = AGR.QUOTED[name]
        if nblk == AGR.GRIDS[name]["request"]:
            assert (f["workgroups"], f["empty"], f["cuts_inside"], f["crossings"]) == \
                (q["entries"], q["empty"], q["cuts_inside"], q["crossings"])
    if (name, nblk) == ("S1", 16):
        assert f["u_again"] >= 1                            # ... and a workgroup whose U tiles stop and start again (ufirst)
    return f


# ---- 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, nblk", REQUESTS, ids=lambda v: str(v))
def test_visit_order_and_features(E, name, nblk, monkeypatch):
    force(monkeypatch, name, nblk)
    with E.EC3DSolver() as s:
        build(s, name, "native")
        check_visit_order(s)        # every A tile and every listed U tile exactly once, interleaved
        check_features(s, name, nblk)


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, nblk, route", [("S1", None, "native"), ("S1", 16, "native"), ("S2", 40, "native"),
                                               ("S3", 8, "native"), ("S1", 16, "csr"), ("S3", 8, "csr")],
                         ids=lambda v: str(v))
def test_spmv_export_and_residual(E, name, nblk, route, monkeypatch):
    force(monkeypatch, name, nblk, POLICIES["nt1-keep0"])
    m, b = matrix_of(name), rhs_of(name)
    rng = np.random.Generator(np.random.PCG64(11))
    with E.EC3DSolver() as s:
        build(s, name, route)
        check_visit_order(s)
        check_features(s, name, nblk)
        assert s.n == m["n"]
        va, ir, jc = s.export_csr()
        wa, wi, wj = m["valA"], m["irow"], m["jcol"]
        if route == "csr":
            # ec3d_set_matrix_csr keeps no explicitly stored zero (tests/test_gpu_av_csr.py pins that): the oracle's arrays
            # without the zeros the boundary value 0 put there, stored order kept
            keep = wa != 0.0
            assert not keep.all()
            rows = np.repeat(np.arange(m["n"]), np.diff(wi))
            wi = np.concatenate([[1], 1 + np.cumsum(np.bincount(rows[keep], minlength=m["n"]))]).astype(np.int32)
            wa, wj = wa[keep], wj[keep]
        assert np.array_equal(ir, wi) and np.array_equal(jc, wj) and va.tobytes() == wa.tobytes()
        for _ in range(3):
            x = rng.standard_normal(m["n"])
            assert np.array_equal(s.spmv(x), O.spmv_csr(m["valA"], m["irow"], m["jcol"], x))
        s.upload("B", b)
        s.upload("X", x)
        rel, bn = s.true_residual()
        r = b - O.spmv_csr(m["valA"], m["irow"], m["jcol"], x)
        assert bn == pytest.approx(float(np.linalg.norm(b)), rel=1e-13)
        assert rel == pytest.approx(float(np.linalg.norm(r) / np.linalg.norm(b)), rel=1e-12)


# ---- 3 -----------------------------------------------------------------------------------------------------------------
def solve_vs_twin(s, m, b, x0, tol, itmax, cap, label):
    t0 = time.perf_counter()
    x, it, hist = s.solve(b, x0, tol, itmax, hist_cap=cap)
    rs = s.restart_count()
    t1 = time.perf_counter()
    xo, ito, hs, hr = O.twin_solve(s, m["valA"], m["irow"], m["jcol"], b, x0, tol, itmax, hist_cap=cap)
    print(f"{label}: iter {it} (twin {ito}), restarts {rs} (twin {O.last_restart_count()}), device {t1 - t0:.2f} s, "
          f"twin {time.perf_counter() - t1:.2f} s")
    assert it == ito and rs == O.last_restart_count()
    assert np.array_equal(hist[:, 0], hs, equal_nan=True) and np.array_equal(hist[:, 1], hr, equal_nan=True)
    assert np.array_equal(x, xo)
    return x, it, hist


@pytest.mark.parametrize("name, nblk, policy", [("S1", 16, "nt0"), ("S1", 16, "nt1-keep0"), ("S1", 16, "nt1-keep11"),
                                                ("S1", None, "nt1-keep0"), ("S2", 40, "nt1-keep0"), ("S3", 8, "nt1-keep0")],
                         ids=lambda v: str(v))
def test_solve_bitwise_vs_twin(E, name, nblk, policy, monkeypatch):
    """24 iterations through the itmax exit from x0 = 0, then six more from 0.5 x on the same handle: x, iter, every ||S||
    and ||R|| of the history and the restart count are the twin's."""
    force(monkeypatch, name, nblk, POLICIES[policy])
    m, b = matrix_of(name), rhs_of(name)
    with E.EC3DSolver() as s:
        build(s, name, "native")
        check_features(s, name, nblk)
        x, it, _ = solve_vs_twin(s, m, b, np.zeros(m["n"]), 1e-30, 23, 24, f"{name} {policy} cold")
        assert it == 24
        _, it, _ = solve_vs_twin(s, m, b, 0.5 * x, 1e-30, 5, 8, f"{name} {policy} warm")
        assert it == 6


# ---- 4 -----------------------------------------------------------------------------------------------------------------
def test_s1_under_the_policy_of_the_256_cube_handle(E, monkeypatch):
    """S1 under what the library gives the 256^3 A-V handle (POLICY_256, read from choose_sweep and ec3d_spare_pair): ten
    iterations -- two whole groups of four deferred X updates and a partial one -- and exits by ||S|| and ||R|| inside
    a group, where the pending updates are flushed before the solve returns."""
    force(monkeypatch, "S1", None, POLICY_256)
    m, b = matrix_of("S1"), rhs_of("S1")
    x0 = np.zeros(m["n"])
    with E.EC3DSolver() as s:
        build(s, "S1", "native")
        check_features(s, "S1", None)
        assert s.x_interval() == 4 and s.fusion() == (0, 0)
        g0, g2 = s.geometry(0), s.geometry(2)
        assert (g0.nblk, g0.xcd_group) == (256, 0) and (g2.nblk, g2.xcd_group) == (768, 0)      # K4's grid, K2's
        _, it, hist = solve_vs_twin(s, m, b, x0, 1e-30, 9, 10, "S1 256^3 policy")
        assert it == 10
        bnorm = float(np.linalg.norm(b))
        seen = set()
        for k, col in ((6, 0), (6, 1), (7, 0), (7, 1)):     # just above ||S_k|| / ||b||, ||R_k|| / ||b||: an exit at iteration <= k
            tol = float(hist[k - 1, col]) / bnorm * (1 + 1e-9)
            _, ite, he = solve_vs_twin(s, m, b, x0, tol, 9, 10, f"S1 256^3 policy, tol above {'SR'[col]}_{k}")
            assert ite <= k
            seen.add(((ite - 1) % 4, "S" if he[ite - 1, 0] / bnorm < tol else "R"))
        print(f"exits (position in the group, kind): {sorted(seen)}")
        assert any(pos != 3 for pos, _ in seen) and {kind for _, kind in seen} == {"S", "R"}
