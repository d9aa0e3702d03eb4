"""CPU-only: the tile lists choose_sweep builds on the host (csrc/ec3d_sweep_lists.hpp).

tests/support/sweep_lists_cases.cpp (a stand-alone program, built with the address and undefined-behaviour sanitizers)
prints, for each case, what it gave a builder and every list that came back.  Every list is compared exactly with a
plain-Python restatement of the rule (written from choose_sweep's own code, before the builders were a header) and checked
for the properties the kernels rely on, which do not depend on that restatement: every tile visited once, holes only
behind a workgroup's last entry, the shares on their XCD's slots, the segments of a column tiling its planes.

Tile t of the four stacked blocks (A_x, A_y, A_z, U) lies in column t % tpp of plane t // tpp."""
import math
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "sweep_lists_cases.cpp")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{kind: {name: {key: [int, ...]}}} as the C++ program prints them ("eff" of a shape case: one float)."""
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("sweep_lists") / "sweep_lists_cases")
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    found, cur = {}, None
    for line in out.stdout.splitlines():
        key, *rest = line.split(" ")
        if key == "case":
            cur = found.setdefault(rest[0], {}).setdefault(rest[1], {})
        else:
            assert key not in cur, line
            cur[key] = float.fromhex(rest[0]) if key == "eff" else [int(v) for v in rest]
    return found


def tdiv(a, b):
    """a / b as C++ divides integers: towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- the XCD-local order -------------------------------------------------------------------------------------------
def xcd_local_order(tiles, tpp, G):
    Gx, L = G // 8, len(tiles)
    byc = sorted(tiles, key=lambda t: t % tpp)            # (sorted is stable, as std::stable_sort)
    share = [sorted(byc[L * x // 8:L * (x + 1) // 8]) for x in range(8)]
    K = max((len(s) + Gx - 1) // Gx for s in share)
    perm = [-1] * (K * G)
    for x in range(8):
        for i, t in enumerate(share[x]):
            perm[(i // Gx) * G + (i % Gx) * 8 + x] = t
    return perm


def test_xcd_local_order(cases):
    seen = set()
    for name, c in cases["xcd"].items():
        (tpp, G), tiles, perm = c["in"], c["tiles"], c["perm"]
        seen.add((tpp, G, len(tiles)))
        assert perm == xcd_local_order(tiles, tpp, G), name
        # every input tile exactly once
        assert sorted(t for t in perm if t >= 0) == sorted(tiles) and len(set(tiles)) == len(tiles), name
        assert len(perm) % G == 0, name
        # a workgroup walks b, b + G, ... up to the first hole: nothing of its share lies behind one
        for b in range(G):
            mine = perm[b::G]
            n = mine.index(-1) if -1 in mine else len(mine)
            assert all(t == -1 for t in mine[n:]), (name, b)
        # slot j * G + i * 8 + x belongs to share x: the eight shares are equal cuts of the tiles ordered by column,
        # each taken in ascending tile order by consecutive workgroups of that XCD label
        L, cut = len(tiles), sorted(tiles, key=lambda t: t % tpp)
        columns_before = -1
        for x in range(8):
            mine = [perm[j * G + i * 8 + x] for j in range(len(perm) // G) for i in range(G // 8)]
            got = [t for t in mine if t >= 0]
            assert mine[:len(got)] == got == sorted(got), (name, x)
            assert len(got) == L * (x + 1) // 8 - L * x // 8, (name, x)
            assert sorted(got) == sorted(cut[L * x // 8:L * (x + 1) // 8]), (name, x)
            if got:
                assert min(t % tpp for t in got) >= columns_before, (name, x)
                columns_before = max(t % tpp for t in got)
    assert seen == {(tpp, G, L) for tpp in (1, 3, 8, 9) for G in (8, 16, 40) for L in (1, 7, 8, 9, 41)}
    # the stable sort is needed: some share holds several planes of one column in the order they were given
    assert any(len({t % c["in"][0] for t in c["tiles"]}) < len(c["tiles"]) and c["tiles"] != sorted(c["tiles"])
               for c in cases["xcd"].values())


# ---- the interleaved z-march ----------------------------------------------------------------------------------------
def il_umask(ulist, tpp, P, tile_flag):
    nw = (P + 31) // 32
    um = [0] * (tpp * nw)
    for t in ulist:
        k, col = tdiv(t, tpp) - 3 * P, t % tpp
        if k < 0 or k >= P:
            return False, nw, um
        um[col * nw + k // 32] |= 1 << (k % 32)
    if tile_flag is not None:
        for t, f in enumerate(tile_flag):
            if f:
                k, col = (t // tpp) % P, t % tpp
                if not (um[col * nw + k // 32] >> (k % 32)) & 1:
                    return False, nw, um
    return True, nw, um


def il_work_list(um, nw, tpp, P, want_il, il_w, min_pps):
    cpx = (tpp + 7) // 8
    bit = lambda col, k: (um[col * nw + k // 32] >> (k % 32)) & 1
    wcol = [sum(il_w if bit(col, k) else 100 for k in range(P)) for col in range(tpp)]
    target = float(sum(wcol)) / float(want_il)
    cuts = []
    for col in range(tpp):
        ns = max(1, int(math.floor(float(wcol[col]) / target + 0.5)))   # llround of a positive quotient
        ns = min(ns, max(1, P // min_pps))
        k0 = acc = 0
        cuts.append([])
        for sgi in range(ns):
            goal = wcol[col] * (sgi + 1) // ns
            k1 = k0
            while k1 < P and (acc < goal or sgi + 1 == ns):
                acc += il_w if bit(col, k1) else 100
                k1 += 1
            cuts[col].append((k0, k1))
            k0 = k1
    max_seg = max(len(c) for c in cuts)
    perx = [[(col,) + cuts[col][sgi] for sgi in range(max_seg) for col in range(x * cpx, min((x + 1) * cpx, tpp))
             if sgi < len(cuts[col])] for x in range(8)]
    per = max(len(p) for p in perx)
    seg = [0] * (per * 8 * 4)
    for x in range(8):
        for j, triple in enumerate(perx[x]):
            seg[(j * 8 + x) * 4:(j * 8 + x) * 4 + 3] = triple
    return per, seg


def check_il_lists(name, c):
    """One case of ec3d_il_umask + ec3d_il_work_list against the restatement and the properties walk_zm_il relies on.
    Returns (nw, um), or None where the builder refused the list (as the restatement must)."""
    tpp, P, want_il, il_w, min_pps, flags = c["in"]
    assert (il_w, min_pps) == (160, 2)
    ok, nw, um = il_umask(c["ulist"], tpp, P, c["tile_flag"] if flags else None)
    assert c["ok"] == [int(ok), nw] and nw == -(-P // 32), name
    if not ok:
        assert set(c) == {"in", "ulist", "tile_flag", "ok"}, name
        return None
    assert c["um"] == um, name
    # the accessor reads the bit of (column, plane) the list set
    visited = {((t // tpp) - 3 * P, t % tpp) for t in c["ulist"]}
    assert c["bits"] == [int((k, col) in visited) for col in range(tpp) for k in range(P)], name
    per, seg = il_work_list(um, nw, tpp, P, want_il, il_w, min_pps)
    assert c["per"] == [per] and c["seg"] == seg, name
    # per * 8 rows of four; the rows of an XCD label that hold a segment come first, the fourth entry is unused
    rows = [c["seg"][4 * b:4 * b + 4] for b in range(len(c["seg"]) // 4)]
    assert len(c["seg"]) == per * 8 * 4 and per >= 1 and all(r[3] == 0 for r in rows), name
    by_col = {}
    for x in range(8):
        mine = rows[x::8]
        n = sum(1 for r in mine if r[2] > r[1])
        assert all(r[2] > r[1] for r in mine[:n]) and all(r == [0, 0, 0, 0] for r in mine[n:]), (name, x)
        for col, k0, k1, _ in mine[:n]:
            assert col // ((tpp + 7) // 8) == x, (name, x)      # columns are dealt to the labels in runs
            by_col.setdefault(col, []).append((k0, k1))
    assert max(sum(1 for r in rows[x::8] if r[2] > r[1]) for x in range(8)) == per, name
    # the segments of a column tile [0, P) without gap or overlap, each of at least min_pps planes
    assert sorted(by_col) == list(range(tpp)), name
    for col, segs in by_col.items():
        segs.sort()
        assert segs[0][0] == 0 and segs[-1][1] == P, (name, col)
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:])), (name, col)
        assert P < min_pps or all(k1 - k0 >= min_pps for k0, k1 in segs), (name, col, segs)
    return nw, um


def test_il_umask_and_work_list(cases):
    seen = set()
    for name, c in cases["il"].items():
        tpp, P, want_il = c["in"][:3]
        if check_il_lists(name, c) is not None:
            seen.add((tpp, P, want_il, len(c["ulist"])))
    sizes = {(tpp, P, w) for tpp in (1, 5, 8, 9) for P in (2, 3, 31, 32, 33, 65) for w in (8, 40, 512)}
    assert {s[:3] for s in seen} == sizes
    for tpp, P, w in sizes:                 # masks: none, all, one column, a checkerboard
        assert {s[3] for s in seen if s[:3] == (tpp, P, w)} >= {0, tpp * P, P, (tpp * P) // 2}


def test_il_lists_of_grids_of_several_columns(cases):
    """The masks of tests/av_grids.py -- the systems tests/test_gpu_interleaved_grids.py runs through walk_zm_il -- at the
    workgroup request quoted for each: the program's list of U tiles is the one the voxels give, the lists are the
    restatement's, and they hold the features the grids are there for, counted (av_grids.features).

    S1_one_block is one block x[9,60) y[10,60) z[3,37) on S1's grid: seven conductor columns of weight 34 * 160 + 6 * 100 =
    6040 and columns 0 and 8 of weight 4000 each, target 50280 / 16 = 3142.5: 7 * 2 + 2 * 1 = 16 segments, 16 of the 32
    entries empty.  S1 itself (two domains, column 8 touched by the second) weighs 4000, 4660, 6 * 5800 and 5140, target
    3037.5: 1 + 2 + 6 * 2 + 2 = 17 segments, 15 entries empty; cuts and crossings as for the one block."""
    import av_grids as AGR
    got = cases["ilgrid"]
    assert set(got) == set(AGR.GRIDS) | {"S1_one_block"}
    for name, c in got.items():
        grid = "S1" if name == "S1_one_block" else name
        tpp, P, want_il, _, _, flags = c["in"]
        sdx, sdy, pitch = c["grid"]
        assert (sdx, sdy, P) == AGR.GRIDS[grid]["dims"] and pitch == AGR.pitch_of(grid) == tpp * 512 and flags == 1
        assert want_il == AGR.GRIDS[grid]["request"]
        assert (pitch > sdx * sdy) == AGR.GRIDS[grid]["pitched"]
        if name in AGR.GRIDS:
            assert c["ulist"] == AGR.u_tiles(name), name
        nw, um = check_il_lists(name, c)
        f = AGR.features(c["seg"], um, nw, P)
        print(name, f)
        assert f == AGR.QUOTED[name], name
        # some column holds no U tile at all exactly where the grid is meant to have one
        bare = [col for col in range(tpp) if not any(c["bits"][col * P:(col + 1) * P])]
        assert bool(bare) == (grid in ("S1", "S2")), name
    # S1: U tiles that stop and start again along z (planes 14 .. 17 of columns 2 .. 7)
    c = got["S1"]
    P = c["in"][1]
    for col in range(2, 8):
        b = c["bits"][col * P:(col + 1) * P]
        assert b[13] == 1 and b[14:18] == [0] * 4 and b[18] == 1, col
    assert not any(c["bits"][:P])               # column 0


def test_il_umask_refuses(cases):
    il = cases["il"]
    c = il["coupled_without_u"]
    tpp, P = c["in"][:2]
    visited = {((t // tpp) - 3 * P, t % tpp) for t in c["ulist"]}
    lone = [t for t, f in enumerate(c["tile_flag"]) if f and ((t // tpp) % P, t % tpp) not in visited]
    assert len(lone) == 1 and c["ok"][0] == 0
    for name, plane in (("u_tile_in_az", 3 * P - 1), ("u_tile_behind_the_block", 4 * P)):
        c = il[name]
        assert [t // tpp for t in c["ulist"] if not 3 * P <= t // tpp < 4 * P] == [plane] and c["ok"][0] == 0


# ---- the z-slab's interior and boundary lists -----------------------------------------------------------------------
def slab_split_lists(ulist, tpp, blk, p0, npo, H):
    ui, ub, owned_only = [], [], True
    for t in ulist:
        pl = tdiv(t - 3 * blk, tpp) - p0
        if t < 3 * blk or pl < 0 or pl >= npo:
            owned_only = False
        elif H <= pl < npo - H:
            ui.append(t)
        else:
            ub.append(t)
    bl = [d * blk + (p0 + pl) * tpp + q for d in range(3) for pl in (0, 1, npo - 2, npo - 1) for q in range(tpp)]
    return owned_only, ui, ub, bl + ub


def test_slab_split_lists(cases):
    seen = set()
    for name, c in cases["slab"].items():
        tpp, blk, p0, npo, H = c["in"]
        owned_only, ui, ub, bl = slab_split_lists(c["ulist"], tpp, blk, p0, npo, H)
        assert c["owned_only"] == [int(owned_only)], name
        if not owned_only:
            assert c["bl"] == [], name
            continue
        seen.add((p0, npo))
        assert (c["ui"], c["ub"], c["bl"]) == (ui, ub, bl), name
        # ui, ub and the A part of bl partition the owned tiles: the U tiles of the list, and with the A tiles of the
        # interior launch's window (H planes narrower at both ends) every A tile of the owned planes
        na = len(c["bl"]) - len(c["ub"])
        a_bnd, tail = c["bl"][:na], c["bl"][na:]
        assert tail == c["ub"] and sorted(c["ui"] + c["ub"]) == sorted(c["ulist"]), name
        assert c["ui"] and c["ub"] and not set(c["ui"]) & set(c["ub"]), name
        assert all(H <= (t - 3 * blk) // tpp - p0 < npo - H for t in c["ui"]), name
        a_int = [d * blk + (p0 + pl) * tpp + q for d in range(3) for pl in range(H, npo - H) for q in range(tpp)]
        a_owned = [d * blk + (p0 + pl) * tpp + q for d in range(3) for pl in range(npo) for q in range(tpp)]
        assert sorted(a_bnd + a_int) == a_owned and len(set(a_bnd)) == len(a_bnd), name
    assert seen == {(0, 6), (0, 7), (3, 6), (3, 7)}
    assert {n for n, c in cases["slab"].items() if c["owned_only"] == [0]} == {"above_the_window", "below_the_window",
                                                                              "in_an_a_block"}


# ---- the runtime-shaped 2-D tiles -----------------------------------------------------------------------------------
def patch_tables(cls, planes, pitch, sdx, sdy, px, py, a0, u0, zero):
    npx, npy = sdx // px, (sdy + py - 1) // py
    tpp = npx * npy
    flag, ulist = [0] * (3 * planes * tpp + 4), []
    for P in range(4 * planes):
        lo, hi = (a0, u0) if P < 3 * planes else (u0, zero)
        for q in range(tpp):
            pyi, pxi = q // npx, q % npx
            cells = [cls[P * pitch + y * sdx + pxi * px + x] for y in range(pyi * py, min(sdy, (pyi + 1) * py)) for x in range(px)]
            if any(lo <= k < hi for k in cells):
                if P < 3 * planes:
                    flag[P * tpp + q] = 1
                else:
                    ulist.append(P * tpp + q)
    return flag, ulist


def test_patch_tables(cases):
    for name, c in cases["patch"].items():
        planes, pitch, sdx, sdy, px, py = c["in"][:6]
        assert (sdx, sdy, pitch) == (16, 6, 128) and pitch > sdx * sdy and sdy % py != 0
        assert (c["flag"], c["ulist"]) == patch_tables(c["cls"], *c["in"]), name
        assert c["flag"][-4:] == [0] * 4 and len(c["flag"]) == 3 * planes * (sdx // px) * -(-sdy // py) + 4
    c = cases["patch"]["marks_8x4"]
    assert c["in"][4:6] == [8, 4]
    tpp = 4                                     # 2 x 2 patches, the second patch row two cells high
    # one coupled cell, in A_y (block 1), plane 1, cell (9, 2): patch (1, 0); U cells (3, 5) of plane 0 and (15, 0) of plane 1
    assert [t for t, f in enumerate(c["flag"]) if f] == [(1 * 2 + 1) * tpp + 1]
    assert c["ulist"] == [(3 * 2 + 0) * tpp + 2, (3 * 2 + 1) * tpp + 1]
    assert cases["patch"]["empty_8x4"]["ulist"] == [] and not any(cases["patch"]["empty_8x4"]["flag"])


def pick_patch_shape(sdx, sdy):
    best, px_out, py_out = 0.0, 0, 0
    if sdx % 2:
        return 0.0, 0, 0
    for px in range(4, min(sdx, 256) + 1, 2):
        if sdx % px or (px < 32 and px != sdx):
            continue
        py = 512 // px
        if py < 2:
            continue
        npy = (sdy + py - 1) // py
        eff = float(px * py) / 512 * float(sdy) / float(npy * py)
        if eff > best + 1e-9 or (eff > best - 1e-9 and abs(px - 128) < abs(px_out - 128)):
            best, px_out, py_out = max(best, eff), px, py
    return best, px_out, py_out


def test_pick_patch_shape(cases):
    got = {tuple(c["in"]): (c["eff"], *c["out"]) for c in cases["shape"].values()}
    assert set(got) == {(16, 15), (18, 16), (102, 102), (256, 256), (15, 16), (101, 102)}
    for (sdx, sdy), g in got.items():
        assert g == pick_patch_shape(sdx, sdy), (sdx, sdy)
        eff, px, py = g
        if sdx % 2:
            assert g == (0.0, 0, 0)
        else:
            assert px % 2 == 0 and sdx % px == 0 and py >= 2 and px * py <= 512 and (px >= 32 or px == sdx)
            assert eff == px * py / 512 * sdy / (-(-sdy // py) * py)
    assert got[(256, 256)] == (1.0, 128, 4) and got[(16, 15)][1:] == (16, 32)


# ---- z segments per column ------------------------------------------------------------------------------------------
def zm_segments(want_s, cols, max_seg, explicit_request):
    if explicit_request:
        nseg = max(1, (want_s + cols // 2) // cols)
    else:
        fit = want_s // cols
        nseg = fit if fit >= 1 and 6 * cols * fit >= 5 * want_s else (3 * want_s + 2 * cols - 1) // (2 * cols)
    return min(nseg, max_seg)


def test_zm_segments(cases):
    got = {tuple(c["in"]): c["nseg"][0] for c in cases["zm"].values()}
    assert set(got) == {(w, cols, m, e) for w in (768, 1024, 1536) for cols in (8, 520) for m in (1000, 2) for e in (0, 1)}
    for k, nseg in got.items():
        assert nseg == zm_segments(*k), k
    # 520 columns: the one segment that fits a round of 768 fills it to 520 / 768 < 5 / 6, so 1.5 rounds (1152 / 520, up)
    assert got[(768, 520, 1000, 0)] == 3 and got[(768, 520, 1000, 1)] == 1
    assert got[(1536, 8, 1000, 0)] == 192 == got[(1536, 8, 1000, 1)] and got[(1536, 8, 2, 0)] == 2
    assert got[(1024, 520, 1000, 0)] == 3 and got[(1024, 520, 1000, 1)] == 2 and got[(1536, 520, 1000, 0)] == 5
