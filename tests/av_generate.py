"""Generated A-V geometries: inputs of ec3d_assemble that no hand-made fixture holds.

generate(seed) -> (geoPHYS, geoPHYS_C, valPHYS, BND, delta, dt), deterministic (PCG64(seed)):

* grid: 7 .. 24 cells per axis, odd sizes included;
* materials: 0 .. 4 conducting domains and 0 .. 2 non-conducting ones share the ids 1 .. M in a random order (so a
  conducting domain's id is not its ordinal among the conductors), air is domain M + 1;
* conductors: every conducting domain is a union of 1 .. 3 boxes at least 3 cells thick, half of the seeds carve a
  through hole into one of them; half of the seeds stack the domains along z in id order (then the U ids are in scan
  order and ec3d_assemble keeps the structured form), the others place them anywhere.  Nothing makes the result legal:
  unions leave two-cell steps, boxes reach the box faces, holes leave thin walls -- the reference refuses those, and
  so must the device;
* U ids: domain-major in id order, scan order within a domain (src/vxc2data.f90:625-636, vxc.domain_tables);
* material: every conducting domain its own C; three of four get three velocity components of either sign;
* boundary: six independent values from BND_VALUES (0, +-1, fractions of either sign);
* spacing: anisotropic delta; dt from three values.

Directed constructors, same return value:

* single_defect(kind), kind in DEFECTS: one legal block with exactly one of the defects the reference refuses;
* near_face(axis, side): a legal block one cell from that box face.

CORPUS is the committed seed list; tests/test_generated_av_host.py asserts what it must contain.
"""
from __future__ import annotations

import numpy as np

MU0 = 0.12566370964050292e-05
BND_VALUES = (0.0, 1.0, -1.0, -0.95, 0.5, -0.25, 1.5)
ADJ_VALUES = (0.75, 1.0, 1.25, 1.5)
DT_VALUES = (1e-3, 5e-4, 2e-3)

CORPUS = tuple(range(1, 81))

DEFECTS = tuple([f"on_face_{a}{s}" for a in "xyz" for s in "mp"] +          # a conducting cell on a box face
                [f"two_thick_{a}" for a in "xyz"] +                          # the one-sided stencil's third cell is air
                [f"third_outside_{a}{s}" for a in "xyz" for s in "mp"] +     # ... or falls outside the box
                [f"both_missing_{a}" for a in "xyz"] +                       # a one-cell plate: no neighbour on either side
                ["zero_column"])                                            # a cavity two cells under the surface


def _tables(vox, conducting, C, vel, rng_bnd, delta, dt):
    """vox [sdz, sdy, sdx] of material ids (0 = air), conducting: ids in palette order."""
    M = int(vox.max()) if vox.size else 0
    M = max(M, max(conducting, default=0))
    v = vox.reshape(-1).astype(np.int32)
    cells = v.size
    geo = np.where(v == 0, M + 1, v).astype(np.int8).reshape(vox.shape)
    geoC = np.zeros(cells, np.int32)
    m = 0
    for d in conducting:                                # domain-major, scan order within the domain
        idx = np.flatnonzero(v == d)
        geoC[idx] = 3 * cells + m + 1 + np.arange(idx.size)
        m += idx.size
    valPHYS = np.zeros((M + 1, 5))
    valPHYS[:, 0] = 1.0
    for d in conducting:
        valPHYS[d - 1, 1] = C[d]
        valPHYS[d - 1, 2:5] = vel[d]
    return (geo, geoC.reshape(vox.shape), valPHYS, np.asarray(rng_bnd, np.float64).reshape(3, 2),
            np.asarray(delta, np.float64), float(dt))


def from_boxes(dims, domains, bnd, delta, dt):
    """Conducting domains given as voxels: dims = (sdx, sdy, sdz); domain d = 1 .. D is domains[d - 1], a dict of boxes and
    holes ([a, b) per axis, 0-based, in the order x, y, z; a hole is carved out of the domain's own boxes), C and vel.
    Nothing makes the result legal.  Same return value as generate."""
    sdx, sdy, sdz = dims
    vox = np.zeros((sdz, sdy, sdx), np.uint8)
    for d, dom in enumerate(domains, 1):
        for (x0, x1), (y0, y1), (z0, z1) in dom["boxes"]:
            part = vox[z0:z1, y0:y1, x0:x1]
            part[part == 0] = d
        for (x0, x1), (y0, y1), (z0, z1) in dom.get("holes", ()):
            part = vox[z0:z1, y0:y1, x0:x1]
            part[part == d] = 0
    ids = list(range(1, len(domains) + 1))
    return _tables(vox, ids, {d: float(domains[d - 1]["C"]) for d in ids},
                   {d: np.asarray(domains[d - 1]["vel"], np.float64) for d in ids}, bnd, delta, dt)


def _box(rng, lo, hi, min_thick=3):
    """A random box [a, b) inside [lo, hi) per axis (z, y, x), at least min_thick thick."""
    out = []
    for l, h in zip(lo, hi):
        span = h - l
        t = int(rng.integers(min_thick, max(min_thick, min(span, 9)) + 1))
        t = min(t, span)
        a = int(rng.integers(l, h - t + 1))
        out.append((a, a + t))
    return out


def generate(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sdx, sdy, sdz = (int(v) for v in rng.integers(7, 25, 3))
    shape = (sdz, sdy, sdx)
    D = int(rng.integers(0, 5))
    extra = int(rng.integers(0, 3))
    ids = rng.permutation(D + extra) + 1
    conducting = sorted(int(i) for i in ids[:D])
    others = sorted(int(i) for i in ids[D:])
    stacked = bool(rng.integers(0, 2))
    margin = 0 if rng.integers(0, 8) == 0 else 1        # one seed in eight may reach the box faces
    vox = np.zeros(shape, np.uint8)
    lo = [margin] * 3
    hi = [s - margin for s in shape]
    if stacked and D > 1:                               # z layers in id order; layers may touch
        cuts = np.linspace(lo[0], hi[0], D + 1).astype(int)
    for n, d in enumerate(conducting):
        l, h = list(lo), list(hi)
        if stacked and D > 1:
            l[0], h[0] = int(cuts[n]), int(cuts[n + 1])
            if h[0] - l[0] < 3:
                continue
        for _ in range(int(rng.integers(1, 4))):
            (z0, z1), (y0, y1), (x0, x1) = _box(rng, l, h)
            part = vox[z0:z1, y0:y1, x0:x1]
            part[part == 0] = d
    if D and rng.integers(0, 2):                        # a through hole along a random axis
        d = conducting[int(rng.integers(0, D))]
        own = np.argwhere(vox == d)
        if len(own):
            c = own[int(rng.integers(0, len(own)))]
            ax = int(rng.integers(0, 3))
            sl = [slice(int(c[a]), int(c[a]) + int(rng.integers(1, 3))) for a in range(3)]
            sl[ax] = slice(None)
            part = vox[tuple(sl)]
            part[part == d] = 0
    for d in others:                                    # non-conducting solids (coil-like) in what is still air
        (z0, z1), (y0, y1), (x0, x1) = _box(rng, [0] * 3, list(shape), min_thick=1)
        part = vox[z0:z1, y0:y1, x0:x1]
        part[part == 0] = d
    C = {d: MU0 * float(rng.uniform(1e6, 6e7)) for d in conducting}
    vel = {d: (rng.uniform(-2.0, 2.0, 3) if rng.integers(0, 4) else np.zeros(3)) for d in conducting}
    bnd = rng.choice(BND_VALUES, 6)
    lattice = float(rng.choice((0.002, 0.004, 0.005)))
    delta = lattice * rng.choice(ADJ_VALUES, 3)
    dt = float(rng.choice(DT_VALUES))
    conducting = [d for d in conducting if np.any(vox == d)]
    return _tables(vox, conducting, C, vel, bnd, delta, dt)


_DIRECTED = dict(C={1: MU0 * 35.26e6}, vel={1: np.array([1.5, -0.7, 0.3])},
                 rng_bnd=(-0.95, 0.5, -1.0, 1.5, 0.0, -0.25), delta=(0.004, 0.005, 0.003), dt=1e-3)
_SHAPE = (13, 12, 11)                                   # sdz, sdy, sdx
_AX = {"x": 2, "y": 1, "z": 0}                          # array axis of a coordinate axis


def _block():
    vox = np.zeros(_SHAPE, np.uint8)
    vox[3:9, 3:8, 3:8] = 1
    return vox


def single_defect(kind):
    """One conducting block, legal but for the one defect `kind` names."""
    vox = np.zeros(_SHAPE, np.uint8)
    what, _, tag = kind.rpartition("_")
    ax = _AX[tag[0]] if what != "zero" else None
    sl = [slice(3, 8)] * 3
    if what == "on_face":                               # 5 cells thick, its last plane on the box face
        sl[ax] = slice(0, 5) if tag[1] == "m" else slice(_SHAPE[ax] - 5, _SHAPE[ax])
    elif what == "two_thick":
        sl[ax] = slice(4, 6)
    elif what == "third_outside":                       # low: a one-cell plate at position 2 (1-based); high: cells at
        sl[ax] = slice(1, 2) if tag[1] == "m" else slice(_SHAPE[ax] - 2, _SHAPE[ax])   # sd - 1 and sd
    elif what == "both_missing":
        sl[ax] = slice(5, 6)
    elif kind == "zero_column":
        vox = _block()
        vox[5, 5, 5] = 0                                # x: cells 3, 4 | cavity at 5 | 6, 7: two cells either side
        return _tables(vox, [1], **_DIRECTED)
    else:
        raise ValueError(kind)
    vox[tuple(sl)] = 1
    return _tables(vox, [1], **_DIRECTED)


def near_face(axis, side):
    """A legal 4-cell-thick block whose outermost plane is one cell from the box face `side` ("m" / "p") of `axis`."""
    vox = np.zeros(_SHAPE, np.uint8)
    sl = [slice(3, 8)] * 3
    ax = _AX[axis]
    sl[ax] = slice(1, 5) if side == "m" else slice(_SHAPE[ax] - 5, _SHAPE[ax] - 1)
    vox[tuple(sl)] = 1
    return _tables(vox, [1], **_DIRECTED)


def u_row_patterns(geoPHYS_C):
    """Set of st_x + 3 st_y + 9 st_z over the conducting cells; st = 0 both neighbours conducting, 1 the minus one
    missing, 2 the plus one missing (the 27 U-row branches of src/EC3D.f90:766-922; 1 + 3*2 + 9*2 = 25 is the corner
    whose signs the reference writes differently, :803-806).  Accepted geometries only (no cell misses both)."""
    on = np.asarray(geoPHYS_C) != 0
    p = np.pad(on, 1)
    pat = np.zeros(on.shape, np.int64)
    for mul, ax in ((1, 2), (3, 1), (9, 0)):
        m = np.roll(p, 1, axis=ax)[1:-1, 1:-1, 1:-1]
        q = np.roll(p, -1, axis=ax)[1:-1, 1:-1, 1:-1]
        pat += mul * np.where(~m, 1, np.where(~q, 2, 0))
    return set(int(v) for v in pat[on])


def a_row_classes(geoPHYS_C):
    """Set of (component d, pattern) over the conducting cells; pattern 1 central, 2 one-sided low (the plus neighbour
    missing, src/EC3D.f90:667-671), 3 one-sided high (:672-676)."""
    on = np.asarray(geoPHYS_C) != 0
    p = np.pad(on, 1)
    out = set()
    for d, ax in ((0, 2), (1, 1), (2, 0)):
        m = np.roll(p, 1, axis=ax)[1:-1, 1:-1, 1:-1]
        q = np.roll(p, -1, axis=ax)[1:-1, 1:-1, 1:-1]
        pat = np.where(~q, 2, np.where(~m, 3, 1))
        out |= {(d, int(v)) for v in pat[on]}
    return out


def moving_domains(geoPHYS, geoPHYS_C, valPHYS):
    """Velocity triples of the conducting domains that hold cells and move."""
    geo = np.asarray(geoPHYS).reshape(-1)
    doms = sorted(set(int(d) for d in geo[np.asarray(geoPHYS_C).reshape(-1) != 0]))
    return [tuple(valPHYS[d - 1, 2:5]) for d in doms if np.any(valPHYS[d - 1, 2:5] != 0.0)]
