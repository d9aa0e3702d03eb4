"""A-V systems on grids whose xy plane is SEVERAL 512-row tiles: what the interleaved z-march of the structured form
(csrc/ec3d_kernels.hip walk_zm_il) and its host lists (csrc/ec3d_sweep_lists.hpp ec3d_il_umask, ec3d_il_work_list) do only
there -- more than one column, mask words beyond the first, columns without a U tile beside columns with one, U tiles that
stop and start again along z, operands fetched by another workgroup, work lists with empty entries and with cuts inside a
conductor.  The captured fixtures (at most 24 x 24 cells per plane, at most 24 planes) are one column wide.

    system(name) -> (geoPHYS, geoPHYS_C, valPHYS, BND, delta, dt), the arguments of ec3d_assemble (av_generate.from_boxes)
    u_tiles(name) -> the U tiles the device lists for it (tile ids of the four stacked blocks), from the voxels alone
    features(seg, um, nw, P) -> what a work list exercises, counted

Boxes are [a, b) per axis, 0-based, in the order x, y, z.  Every system has six distinct boundary values (one of them 0)
and anisotropic spacing.  No test lives here (the name does not start with test_)."""
import numpy as np

import av_generate as AG

TILE = 512
MU0 = AG.MU0

# name: dims (sdx, sdy, sdz), domains in id order [(boxes, holes, sigma, velocity)], the workgroup request the host test
# quotes, and whether the plane needs EC3D_PITCH=2 (it is no whole number of tiles)
GRIDS = {
    # the plane is 9 tiles of 8 grid rows; column 0 (y < 8) holds no conductor; domain 1 ends at plane 13, domain 2 starts
    # at plane 18 (columns 2 .. 7 lose their U tiles on planes 14 .. 17 and get them back) and crosses planes 31 / 32
    "S1": dict(dims=(64, 72, 40),
               domains=[([((9, 52), (10, 60), (3, 14))], [((28, 36), (30, 38), (3, 14))], 35.26e6, (0.3, -0.2, 0.1)),
                        ([((20, 60), (18, 66), (18, 37))], [], 5.8e6, (0.0, 0.0, 0.0))],
               bnd=(-0.95, 0.5, -1.0, 1.5, 0.0, -0.25), delta=(0.004, 0.005, 0.003), dt=1e-3, request=16, pitched=False),
    # a tile is half a grid row: 16 columns, +-sdx two tiles away; the conductor crosses the tile boundary at x = 512
    "S2": dict(dims=(1024, 8, 34),
               domains=[([((400, 640), (2, 6), (3, 31))], [], 35.26e6, (1.5, -0.7, 0.3))],
               bnd=(0.5, -0.95, 1.5, -1.0, -0.25, 0.0), delta=(0.002, 0.005, 0.004), dt=5e-4, request=40, pitched=False),
    # planes of 1200 cells in 1536 rows: tiles start mid-row at cells 512 and 1024, the third is mostly padding
    "S3": dict(dims=(40, 30, 33),
               domains=[([((5, 34), (4, 26), (3, 30))], [], 35.26e6, (-0.4, 0.9, 0.2))],
               bnd=(1.5, 0.0, -0.25, -0.95, 0.5, -1.0), delta=(0.005, 0.003, 0.004), dt=2e-3, request=8, pitched=True),
}

_cache = {}


def system(name):
    if name not in _cache:
        g = GRIDS[name]
        _cache[name] = AG.from_boxes(g["dims"], [dict(boxes=b, holes=h, C=MU0 * sigma, vel=v) for b, h, sigma, v in g["domains"]],
                                     g["bnd"], g["delta"], g["dt"])
        for a in _cache[name][:5]:
            a.setflags(write=False)
    return _cache[name]


def pitch_of(name):
    sdx, sdy, _ = GRIDS[name]["dims"]
    return (sdx * sdy + TILE - 1) // TILE * TILE


def u_tiles(name):
    """Ascending tile ids of the U block's tiles that hold a conducting cell: tile (3 P + k) * tpp + col."""
    sdx, sdy, sdz = GRIDS[name]["dims"]
    tpp = pitch_of(name) // TILE
    on = np.asarray(system(name)[1]).reshape(sdz, sdx * sdy) != 0
    k, cell = np.nonzero(on)
    return sorted(set(int(t) for t in (3 * sdz + k) * tpp + cell // TILE))


def features(seg, um, nw, P):
    """What the work list `seg` (four int32 per workgroup: column, first plane, end plane, 0) of the mask `um` exercises:
    entries, empty ones (k0 == k1), segments that start with a U step behind a U step of the same column (a cut inside a
    conductor's plane range), segments that step from plane 31 to plane 32 (into the mask's second word)."""
    bit = lambda col, k: (int(um[col * nw + k // 32]) >> (k % 32)) & 1
    rows = [tuple(int(v) for v in seg[4 * b:4 * b + 4]) for b in range(len(seg) // 4)]
    return dict(entries=len(rows), empty=sum(1 for c, k0, k1, _ in rows if k0 == k1),
                cuts_inside=sum(1 for c, k0, k1, _ in rows if k1 > k0 > 0 and bit(c, k0 - 1) and bit(c, k0)),
                crossings=sum(1 for c, k0, k1, _ in rows if k0 <= 31 and k1 > 32),
                columns=len({c for c, k0, k1, _ in rows if k1 > k0}), words=nw)


# what the lists of ec3d_il_umask / ec3d_il_work_list hold for each grid at its quoted request
# (S1_one_block: the one block x[9,60) y[10,60) z[3,37) on S1's grid, tests/support/sweep_lists_cases.cpp; the
# arithmetic behind the two S1 lines is in tests/test_sweep_lists_host.py)
QUOTED = {"S1_one_block": dict(entries=32, empty=16, cuts_inside=7, crossings=9, columns=9, words=2),
          "S1": dict(entries=32, empty=15, cuts_inside=7, crossings=9, columns=9, words=2),
          "S2": dict(entries=48, empty=8, cuts_inside=16, crossings=16, columns=16, words=2),
          "S3": dict(entries=24, empty=15, cuts_inside=6, crossings=3, columns=3, words=2)}
