"""CPU-only: the boundary + interior launch pairs of a z-slab (csrc/ec3d_split_sweeps.hpp).

tests/support/split_sweeps_cases.cpp (a stand-alone program, built with the address and undefined-behaviour sanitizers)
makes the sweeps of small slab handles, asks the header for every split -- s: K1 / K3, f: the 2-D-tile kernels of the
three-launch iteration, v: K2 / K5 by planes, r: K2 / K5 by rows -- and prints every field of both sweeps, ok, parts(), the
stride of the partial sums and the visit order of every launch through ec3d_visit_of.

Every printed number is compared with a plain-Python restatement of the rules, written from choose_sweep and
ec3d_dist_set_boundary_* as they stood before the header existed.  Independently of that restatement: the two launches
of a split visit exactly the tiles of the unsplit launch, each once; the boundary launches hold the planes next to the cuts
and nothing else; the two launches' partial sums neither overlap nor pass the stride; a grid on an XCD-aware map is a
whole multiple of 8.

Tile t lies in column t % tpp of plane t // tpp; a structured slab stacks four blocks (A_x, A_y, A_z, U) of blk tiles."""
import os
import shutil
import subprocess

import pytest

from test_sweep_lists_host import slab_split_lists, xcd_local_order

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "split_sweeps_cases.cpp")
TILE = 512
FIELDS = ("ntiles n nblk S nt vec_depth pstride zm_tpp zm_pps patch_npx patch_sdx rp_px rp_py rp_npx rp_sdy rp_sdx rp_pitch "
          "nown win_nt win_blk win_t0 zm_pl0 zm_npl zm_plstep bnd_last halo_store part_off ulist_n il_planes il_nw pair "
          "has_ulist has_il_umask has_il_seg has_rp_flag lo0 lo1 lo2 lo3 hi0 hi1 hi2 hi3").split()
SWEEPS = ("sw", "k2", "k5", "ss") + tuple(f"{x}_{w}" for x in "sfvr" for w in ("bnd", "inte"))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{kind: {name: {key: [int, ...]}}} as the C++ program prints them; a sweep's line becomes {field: value}."""
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(cc)))
    exe = str(tmp_path_factory.mktemp("split_sweeps") / "split_sweeps_cases")
    subprocess.run([cc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-std=c++17", "-O1", "-g",
                    "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    found, cur = {}, None
    for line in out.stdout.splitlines():
        key, *rest = line.split(" ")
        if key == "case":
            cur = found.setdefault(rest[0], {}).setdefault(rest[1], {})
            continue
        assert key not in cur, line
        vals = [int(v) for v in rest]
        if key in SWEEPS:
            assert len(vals) == len(FIELDS), line
            vals = dict(zip(FIELDS, vals))
        cur[key] = vals
    return found


def handles(cases):
    return [(kind, name, c) for kind in ("single", "av") for name, c in cases[kind].items()]


# ---- the rules as the parent stated them, where it stated them -------------------------------------------------------
VEC_BND_CAP = 256     # "boundary list <= 256 workgroups": a literal in both vector splits and in the stride


def planes_held(sw, ss):
    np_ = sw["ntiles"] // ss["zm_tpp"]
    return np_ if np_ * ss["zm_tpp"] == sw["ntiles"] else 0


def parent_split_s(c):
    """choose_sweep: K1 / K3 of the single-component slab, else of the structured slab on a plane window."""
    (halo, nown, sav, _), sw, ss = c["in"], c["sw"], c["ss"]
    si, sb, lb, li = dict(ss), dict(ss), [], []
    if halo > 0 and nown == 0 and ss["zm_tpp"] > 0:
        np_ = planes_held(sw, ss)
        if np_ >= 10:
            tpp, npl = ss["zm_tpp"], np_ - 2
            cols = (tpp + 7) // 8 * 8
            nseg = max(1, (ss["nblk"] + cols // 2) // cols)
            nseg = min(nseg, max(1, npl // 8))
            si.update(zm_pl0=1, zm_npl=npl, zm_pps=(npl + nseg - 1) // nseg, nblk=cols * nseg, part_off=0)
            sb.update(bnd_last=np_ - 1, patch_npx=0, nblk=min(2 * tpp, 768), part_off=si["nblk"])
            return True, sb, si, lb, li
    if sav and halo > 0 and sw["win_nt"] > 0 and ss["zm_tpp"] > 0 and ss["rp_px"] == 0:
        tpp, H, blk = ss["zm_tpp"], 2, sw["win_blk"]
        npo, p0 = sw["win_nt"] // tpp, sw["win_t0"] // tpp
        if npo * tpp == sw["win_nt"] and p0 * tpp == sw["win_t0"] and npo >= 2 * H + 2:
            npi = npo - 2 * H
            owned_only, ui, ub, bl = slab_split_lists(c["ulist"], tpp, blk, p0, npo, H)
            if owned_only:
                cols = (tpp + 7) // 8 * 8
                nseg = max(1, ss["nblk"] // cols)
                nseg = min(nseg, max(1, 3 * npi // 2))
                si.update(win_t0=sw["win_t0"] + H * tpp, win_nt=npi * tpp, ntiles=3 * npi * tpp,
                          zm_pps=(3 * npi + nseg - 1) // nseg, nblk=cols * nseg, part_off=0)
                li = xcd_local_order(ui, tpp, si["nblk"]) if ui else []
                si.update(ulist_n=len(li), has_ulist=0)       # (the device pointers are the caller's to set)
                sb.update(ntiles=0, win_nt=0, ulist_n=len(bl), has_ulist=0, nblk=max(8, min(len(bl), 768) // 8 * 8),
                          part_off=si["nblk"])
                return True, sb, si, bl, li
    return False, sb, si, lb, li


def parent_split_f(c):
    """choose_sweep: the 2-D-tile kernels of the three-launch iteration."""
    (halo, nown, _, _), sw, ss = c["in"], c["sw"], c["ss"]
    fb, fi = dict(ss), dict(ss)
    if halo > 0 and nown == 0 and ss["zm_tpp"] > 0 and ss["patch_npx"] > 0:
        np_ = planes_held(sw, ss)
        if np_ >= 3:
            tpp, npl = ss["zm_tpp"], np_ - 2
            cols = (tpp + 7) // 8 * 8
            fb.update(zm_pl0=0, zm_plstep=np_ - 1, zm_npl=2, zm_pps=1, nblk=cols * 2, part_off=0)
            nseg = max(1, (ss["nblk"] + cols // 2) // cols)
            nseg = min(nseg, max(1, npl // 2))
            fi.update(zm_pl0=1, zm_npl=npl, zm_pps=(npl + nseg - 1) // nseg, nblk=cols * nseg, part_off=fb["nblk"])
            return True, fb, fi, [], []
    return False, fb, fi, [], []


def parent_can_split_planes(c):
    (halo, nown, sav, _), k2, ss = c["in"], c["k2"], c["ss"]
    if sav or halo <= 0 or nown != 0 or k2["ulist_n"] != 0 or ss["zm_tpp"] <= 0 or k2["win_nt"] != 0:
        return False
    return planes_held(k2, ss) >= 3


def parent_split_v(c):
    """ec3d_dist_set_boundary_planes: K2 / K5 as plane windows."""
    k2, ss = c["k2"], c["ss"]
    vb, vi = dict(k2), dict(k2)
    if not parent_can_split_planes(c):
        return False, vb, vi, [], []
    tpp, total = ss["zm_tpp"], k2["ntiles"]
    vb.update(ntiles=2 * tpp, win_nt=tpp, win_blk=total - tpp, win_t0=0, S=0, vec_depth=1,
              nblk=max(8, min(2 * tpp, VEC_BND_CAP) // 8 * 8), part_off=0)
    nti = total - 2 * tpp
    nblk = min(k2["nblk"], max(8, nti // 8 * 8))
    vi.update(ntiles=nti, win_nt=nti, win_blk=total, win_t0=tpp, nblk=nblk, S=nblk // 8 if k2["S"] > 0 else 0,
              part_off=vb["nblk"])
    return True, vb, vi, [], []


def phys_tile(sw, t):
    return t if sw["win_nt"] <= 0 else (t // sw["win_nt"]) * sw["win_blk"] + sw["win_t0"] + t % sw["win_nt"]


def parent_split_r(c):
    """ec3d_dist_set_boundary_rows: K2 / K5 from tile lists."""
    sw = c["sw"]
    visit = [phys_tile(sw, t) for t in range(sw["ntiles"])] + c["ulist"]
    vb, vi = [], []
    for t in visit:
        r0, r1 = t * TILE, (t + 1) * TILE
        (vb if any(lo < r1 and hi > r0 for lo, hi in zip(c["lo"], c["hi"])) else vi).append(t)
    sb, si = dict(sw), dict(sw)
    if not vb or not vi:
        return False, sb, si, vb, vi
    sb.update(ntiles=0, has_ulist=0, ulist_n=len(vb), nblk=min(len(vb), VEC_BND_CAP), S=0, part_off=0)
    si.update(ntiles=0, has_ulist=0, ulist_n=len(vi), nblk=min(len(vi), sw["nblk"]), S=0, part_off=sb["nblk"])
    return True, sb, si, vb, vi


PARENT = {"s": parent_split_s, "f": parent_split_f, "v": parent_split_v, "r": parent_split_r}


def tile_of(sw, b, i):
    """ec3d_tile_of (ec3d_internal.hpp), MODE -1."""
    tpp = sw["zm_tpp"]
    if sw["bnd_last"] >= 0:
        t = i * sw["nblk"] + b
        return -1 if t >= 2 * tpp else (0 if t < tpp else sw["bnd_last"] * tpp) + t % tpp
    if tpp > 0:
        cpx, c, s = (tpp + 7) >> 3, b & 7, b >> 3
        col, seg = c * cpx + s % cpx, s // cpx
        pl = seg * sw["zm_pps"] + i
        if col >= tpp or i >= sw["zm_pps"] or (sw["zm_npl"] > 0 and pl >= sw["zm_npl"]):
            return -1
        t = (sw["zm_pl0"] + (pl * sw["zm_plstep"] if sw["zm_plstep"] > 1 else pl)) * tpp + col
    elif sw["S"] > 0:
        t = (i * 8 + (b & 7)) * sw["S"] + (b >> 3)
    else:
        t = i * sw["nblk"] + b
    return phys_tile(sw, t) if t < sw["ntiles"] else -1


def visit_of(sw, ul):
    """(offsets, tiles) of a launch: per workgroup its front sweep, then its share of the list up to the first hole."""
    off, tiles = [0], []
    for b in range(sw["nblk"]):
        i = 0
        while (t := tile_of(sw, b, i)) >= 0:
            tiles.append(t)
            i += 1
        l = b
        while l < sw["ulist_n"] and ul[l] >= 0:
            tiles.append(ul[l])
            l += sw["nblk"]
        off.append(len(tiles))
    return off, tiles


def test_every_printed_number_follows_the_parents_rules(cases):
    oks = {x: set() for x in PARENT}
    for kind, name, c in handles(cases):
        assert c["in"][3] == int(parent_can_split_planes(c)), name
        got = {}
        for x, rule in PARENT.items():
            ok, bnd, inte, lb, li = rule(c)
            got[x] = (ok, bnd, inte)
            assert c[x + "_ok"] == [int(ok)], (name, x)
            assert c[x + "_bnd"] == bnd and c[x + "_inte"] == inte, (name, x)
            assert c[x + "_parts"] == [bnd["nblk"] + inte["nblk"]], (name, x)
            assert c[x + "_lb"] == lb and c[x + "_li"] == li, (name, x)
            if not ok:      # both members hold the unsplit sweep, which reads the unsplit list
                lb = li = c["us"] if x in "sf" else c["ulist"]
            assert (c[x + "_vb_off"], c[x + "_vb_tiles"]) == visit_of(bnd, lb), (name, x)
            assert (c[x + "_vi_off"], c[x + "_vi_tiles"]) == visit_of(inte, li), (name, x)
            oks[x].add(ok)
        for key, ul in (("ss", c["us"]), ("k2", c["ulist"]), ("sw", c["ulist"])):
            assert (c[key + "_off"], c[key + "_tiles"]) == visit_of(c[key], ul), (name, key)
        # the stride at the end of choose_sweep: room for a vector kernel in two launches as well
        parts = max([c["ss"]["nblk"]] + [b["nblk"] + i["nblk"] for ok, b, i in (got["s"], got["f"]) if ok])
        vmax = max(c["sw"]["nblk"], c["k2"]["nblk"], c["k5"]["nblk"])
        assert c["stride"] == [max(vmax + 256, c["ss"]["nblk"], parts), VEC_BND_CAP], name
    assert all(v == {True, False} for v in oks.values()), oks


# ---- properties that do not depend on the restatement ---------------------------------------------------------------
def launches(c, x):
    return c[x + "_bnd"], c[x + "_inte"], c[x + "_vb_tiles"], c[x + "_vi_tiles"]


UNSPLIT = {"s": "ss", "f": "ss", "v": "k2", "r": "sw"}


def test_a_split_visits_the_unsplit_launchs_tiles_each_once(cases):
    n = 0
    for kind, name, c in handles(cases):
        for x, whole in UNSPLIT.items():
            if not c[x + "_ok"][0]:
                # refused: both members are the unsplit sweep (the two SpMV splits) or the vector kernels' own
                assert c[x + "_bnd"] == c[x + "_inte"] == c[whole], (name, x)
                continue
            _, _, vb, vi = launches(c, x)
            want = c[whole + "_tiles"]
            assert len(set(want)) == len(want) > 0, (name, whole)
            assert sorted(vb + vi) == sorted(want) and vb and vi, (name, x)
            n += 1
    assert n > 300


def test_boundary_launches_hold_the_planes_next_to_the_cuts(cases):
    for name, c in cases["single"].items():
        tpp = c["ss"]["zm_tpp"]
        np_ = c["sw"]["ntiles"] // tpp
        outer = sorted(list(range(tpp)) + list(range((np_ - 1) * tpp, np_ * tpp)))
        for x in "sfvr":                                        # (r: the driver's ranges are those two planes)
            if c[x + "_ok"][0]:
                assert sorted(c[x + "_vb_tiles"]) == outer, (name, x)
    seen = 0
    for name, c in cases["av"].items():
        if not c["s_ok"][0]:
            continue
        sw, tpp = c["sw"], c["ss"]["zm_tpp"]
        blk, p0, npo = sw["win_blk"], sw["win_t0"] // tpp, sw["win_nt"] // tpp
        near = [p0, p0 + 1, p0 + npo - 2, p0 + npo - 1]         # the two owned planes at each cut
        a_tiles = [d * blk + pl * tpp + q for d in range(3) for pl in near for q in range(tpp)]
        u_tiles = [t for t in c["ulist"] if (t - 3 * blk) // tpp in near]
        assert u_tiles and sorted(c["s_vb_tiles"]) == sorted(a_tiles + u_tiles), name
        # ... and the driver's row ranges (those planes of all four blocks) give K2 / K5 the same boundary tiles
        assert c["r_ok"] == [1] and sorted(c["r_vb_tiles"]) == sorted(a_tiles + u_tiles), name
        seen += 1
    assert seen == 4 * 3 * 2 * 3 + 1                             # npo 6, 7, 12 of 5, 6, 7, 12; the odd grid


def test_partial_sums_of_the_two_launches_lie_side_by_side_below_the_stride(cases):
    for kind, name, c in handles(cases):
        for x in "sfvr":
            if not c[x + "_ok"][0]:
                continue
            b, i = c[x + "_bnd"], c[x + "_inte"]
            first, second = sorted((b, i), key=lambda s: s["part_off"])
            assert first["part_off"] == 0 and second["part_off"] == first["nblk"], (name, x)
            assert second["part_off"] + second["nblk"] == c[x + "_parts"][0] <= c["stride"][0], (name, x)
            assert len(c[x + "_vb_off"]) == b["nblk"] + 1 and len(c[x + "_vi_off"]) == i["nblk"] + 1, (name, x)


def test_grids_on_an_xcd_aware_map_are_whole_multiples_of_eight(cases):
    n = 0
    for kind, name, c in handles(cases):
        for key in SWEEPS:
            s = c[key]
            if name.startswith("odd_grid") and s == c["ss"]:               # (made odd on purpose: a split made of it is not)
                continue
            if (s["zm_tpp"] > 0 and s["bnd_last"] < 0) or s["S"] > 0:     # z-march (lists behind one too), moving window
                assert s["nblk"] % 8 == 0 and s["nblk"] > 0, (name, key)
                assert s["S"] in (0, s["nblk"] // 8), (name, key)
                n += 1
    assert n > 1000


def test_the_cases_cross_every_threshold(cases):
    single = {n: c for n, c in cases["single"].items() if n.startswith("t")}
    ok = lambda c, x: bool(c[x + "_ok"][0])
    for name, c in single.items():
        tpp, np_ = c["ss"]["zm_tpp"], c["sw"]["ntiles"] // c["ss"]["zm_tpp"]
        assert ok(c, "s") == (np_ >= 10) and ok(c, "v") == (np_ >= 3), name
        assert ok(c, "f") == (np_ >= 3 and name.endswith("_2d")), name
        assert ok(c, "r") == (np_ >= 3), name       # two planes held: every tile is boundary
    assert {(c["ss"]["zm_tpp"], c["sw"]["ntiles"] // c["ss"]["zm_tpp"]) for c in single.values()} == \
        {(t, p) for t in (1, 2, 3, 8, 12, 32) for p in (2, 3, 9, 10, 11, 24)}
    assert {c["ss"]["nblk"] for n, c in cases["single"].items() if n.startswith("literal")} == {8, 48, 1536}
    for name, c in cases["av"].items():
        if name.startswith("t"):
            assert ok(c, "s") == (c["sw"]["win_nt"] // c["ss"]["zm_tpp"] >= 6) and not ok(c, "f") and not ok(c, "v"), name
    refused = {"single": {"no_halo": "sfv", "ownership_ranges": "sfv", "ragged_last_plane": "sfv", "rows_all_boundary": "r",
                          "rows_no_range": "r"},
               "av": {"u_tile_in_the_halo": "s", "on_2d_tiles": "s", "no_halo": "s", "window_off_a_plane": "s"}}
    for kind, names in refused.items():
        for name, xs in names.items():
            assert not any(ok(cases[kind][name], x) for x in xs), name
    # what each refusal takes away is there without it
    assert all(ok(cases["single"]["t3_p11_w48_2d"], x) for x in "sfvr") and ok(cases["av"]["t3_n7_p2_w48"], "s")
