"""One conducting plate swept through the z-slab cuts: the family of tests/test_av_cut_sweep_host.py and
tests/test_gpu_av_cut_sweep.py.  Importable data only: no GPU, no oracle.

member(sdz, z0, t, hole) is av_generate.from_boxes on a 12 x 11 x sdz grid with one conducting domain, the box
x in [2, 10), y in [2, 9), z in [z0, z0 + t); hole = "z" carves x in [5, 6), y in [5, 6) through every plane (with it
av_generate.u_row_patterns gives all 27 U-row branches of src/EC3D.f90:766-922).  Material, boundary values, spacing and dt
are those of av_generate's directed constructors.

MEMBERS maps a key (sdz, z0, t, hole) to the `world`s it runs at:

    thin plate    sdz 16, t 3, z0 1 .. 12 (every legal one), the z hole in every second member     world 2, 3, 4
    thick plate   sdz 16, t 7, z0 1 .. 8, no hole                                                  world 2, 3, 4
    thin slabs    sdz 8,  t 3 or 4, every legal z0, no hole                                        world 4 (two planes per rank)

At world 2 the cut of the 16-plane grid is plane 8, so for t = 3 the cut lies from four planes under the plate
(z0 = 12) to four planes over it (z0 = 1): one plane inside either face (the geometry the two-plane U halo exists for:
the one-sided A-U stencil of src/EC3D.f90:697-706 reads two planes, both the neighbour's), on a face, one and two
planes outside.

TWO_DOMAIN: the plate split by a z-plane into two domains (U ids in scan order), the interface on the cut of world 2,
one plane below it and one above.  Slabs refuse several domains; the GPU test asserts that refusal.

situations(per_plane, sdz, world) names what a (member, world) pair holds, read off slab_bounds and the per-plane
counts of conducting cells alone; SITUATIONS lists the names.  "below" / "above": the face, the conductor or the
neighbour the situation speaks of lies below / above the cut concerned.
"""
from __future__ import annotations

import numpy as np

import av_generate as AG

SDX, SDY = 12, 11
C = AG.MU0 * 35.26e6
VEL = (1.5, -0.7, 0.3)
BND = (-0.95, 0.5, -1.0, 1.5, 0.0, -0.25)
DELTA = (0.004, 0.005, 0.003)
DT = 1e-3
H = 2                                   # U halo planes per side (dist.HipAVSlabOps.H)


def slab_bounds(sdz, rank, world):
    """eddy_currents_3d_amd.dist.slab_bounds, restated so that this module imports nothing of the package."""
    base, rem = divmod(sdz, world)
    k0 = rank * base + min(rank, rem)
    return k0, k0 + base + (1 if rank < rem else 0)


def member(sdz, z0, t, hole=None):
    dom = dict(boxes=[((2, 10), (2, 9), (z0, z0 + t))], C=C, vel=VEL)
    if hole == "z":
        dom["holes"] = [((5, 6), (5, 6), (0, sdz))]
    elif hole is not None:
        raise ValueError(hole)
    return AG.from_boxes((SDX, SDY, sdz), [dom], BND, DELTA, DT)


def two_domain(zi, sdz=16, t=3):
    """Domain 1 in planes [zi - t, zi), domain 2 in [zi, zi + t): one plate, its internal interface at plane zi."""
    doms = [dict(boxes=[((2, 10), (2, 9), (zi - t, zi))], C=C, vel=VEL),
            dict(boxes=[((2, 10), (2, 9), (zi, zi + t))], C=AG.MU0 * 58e6, vel=(0.0, 0.0, 0.0))]
    return AG.from_boxes((SDX, SDY, sdz), doms, BND, DELTA, DT)


THIN_PLATE = [(16, z0, 3, "z" if z0 % 2 == 0 else None) for z0 in range(1, 13)]
THICK_PLATE = [(16, z0, 7, None) for z0 in range(1, 9)]
THIN_SLABS = [(8, z0, t, None) for t in (3, 4) for z0 in range(1, 8 - t)]
MEMBERS = {**{k: (2, 3, 4) for k in THIN_PLATE + THICK_PLATE}, **{k: (4,) for k in THIN_SLABS}}
PAIRS = [(k, w) for k, ws in MEMBERS.items() for w in ws]
TWO_DOMAIN = (8, 7, 9)                  # interface planes: on the cut of world 2 (plane 8), one below, one above


def key_id(key):
    sdz, z0, t, hole = key
    return f"sdz{sdz}-z{z0}-t{t}" + ("-hole" if hole else "")


def per_plane(geoPHYS_C):
    g = np.asarray(geoPHYS_C)
    return (g != 0).reshape(g.shape[0], -1).sum(axis=1)


def cuts(sdz, world):
    return [slab_bounds(sdz, r, world)[0] for r in range(1, world)]


SITUATIONS = tuple(f"{s} {side}" for s in ("cut one plane inside a face", "cut on a face", "cut one plane outside a face",
                                          "cut two planes outside a face", "rank owns no conductor, some in its halo",
                                          "rank's extended slab holds no conductor", "rank owned entirely by conductor",
                                          "two-plane rank, both planes travel")
                   for side in ("below", "above"))


def situations(per, sdz, world):
    """Set of SITUATIONS the slabs of `world` ranks meet on a grid whose plane k holds per[k] conducting cells."""
    on = lambda k: 0 <= k < sdz and per[k] > 0
    out = set()
    for c in cuts(sdz, world):          # the cut lies between planes c - 1 and c
        # the face lies BELOW the cut: between c - 2 and c - 1 (inside), c - 1 and c (on), ...
        if on(c - 1) and not on(c - 2) and on(c):
            out.add("cut one plane inside a face below")
        if on(c) and not on(c + 1) and on(c - 1):
            out.add("cut one plane inside a face above")
        if on(c - 1) and not on(c):
            out.add("cut on a face below")
        if on(c) and not on(c - 1):
            out.add("cut on a face above")
        if not on(c) and not on(c - 1) and on(c - 2):
            out.add("cut one plane outside a face below")
        if not on(c - 1) and not on(c) and on(c + 1):
            out.add("cut one plane outside a face above")
        if not on(c) and not on(c - 1) and not on(c - 2) and on(c - 3):
            out.add("cut two planes outside a face below")
        if not on(c - 1) and not on(c) and not on(c + 1) and on(c + 2):
            out.add("cut two planes outside a face above")
    total = int(np.sum(per))
    for r in range(world):
        k0, k1 = slab_bounds(sdz, r, world)
        e0, e1 = max(0, k0 - H), min(sdz, k1 + H)
        own, lo, hi = int(np.sum(per[k0:k1])), int(np.sum(per[e0:k0])), int(np.sum(per[k1:e1]))
        if own == 0 and lo > 0:
            out.add("rank owns no conductor, some in its halo below")
        if own == 0 and hi > 0:
            out.add("rank owns no conductor, some in its halo above")
        if own + lo + hi == 0 and total > 0:
            out.add("rank's extended slab holds no conductor " + ("below" if int(np.sum(per[:e0])) > 0 else "above"))
        if all(per[k] > 0 for k in range(k0, k1)):
            if on(k0 - 1):              # the conductor goes on through the cut under the rank
                out.add("rank owned entirely by conductor below")
            if on(k1):
                out.add("rank owned entirely by conductor above")
        if k1 - k0 == H and own > 0:    # the neighbour's U halo is this whole slab, and it travels whatever the rule
            if r > 0:
                out.add("two-plane rank, both planes travel below")
            if r < world - 1:
                out.add("two-plane rank, both planes travel above")
    return out
