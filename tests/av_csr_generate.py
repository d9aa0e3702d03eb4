"""CSR matrices for the A-V recogniser (csrc/ec3d_sav_csr.cpp), the production route of the drop-in symbol: what the
reference assembles, what it never assembles but the recogniser's contract admits, and what it must refuse.

corpus(oracle) -> [Member], deterministic, three families:

* generated: oracle.gen_sparse_matrix of every oracle-accepted member of av_generate.CORPUS and EXTRA_SEEDS and of the
  six av_generate.near_face blocks.  Recognised exactly when the U ids are in scan order
  (multidomain_numpy.structured_applies).
* mutated: one edit (MUTATIONS) of each member of MUTATION_BASES -- recognised members with 1, 2 and >= 3 conducting
  domains.  The expected decision of every edit is the TABLE's, under the default pitch and under EC3D_PITCH=2.
* saturated: built from nothing (saturated()): a box, a set of conducting cells that may touch the box faces and the
  first and last plane, and EVERY slot the recogniser admits filled -- the 7 bands of all four blocks, the U slots
  m = -2 .. 2 of a conducting cell's A rows whose target cell is conducting, the 9 A slots and 7 U bands of every U row
  whose target exists.  Values depend on (block, slot) only; the diagonal exceeds the sum of everything else a row can
  hold, so every row is strictly diagonally dominant.  Three wrap settings: "none" (no entry leaves its grid line),
  "x" (offsets along x also cross a row end, inside the plane), "all" (any entry whose target exists: across row ends,
  plane ends and the z faces of a component).  Recognised under the default pitch; with tile-aligned planes
  (EC3D_PITCH=2) exactly when no entry crosses a plane boundary, i.e. unless the setting is "all".

Every column these matrices hold is a row +- at most two planes away in the device numbering, which the ghost zone of
every work vector covers: ordinary inputs of the parity tests.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import av_generate as AG
import multidomain_numpy as MD

EXTRA_SEEDS = ()                 # seeds beyond av_generate.CORPUS; every one is run
MUTATION_BASES = (3, 16, 63)     # recognised, D = 1, 2, >= 3 (asserted by tests/test_av_csr_host.py)
WRAPS = ("none", "x", "all")

# name: (default pitch, EC3D_PITCH=2, change of the class count where recognised: a number or None = not stated)
TABLE = {
    "wrap_x": (True, True, 1),
    "wrap_plane": (True, False, None),
    "wrap_zero": (True, True, 0),
    "off_plus2": (False, False, None),
    "u_row_two_away": (False, False, None),
    "air_row_u_col": (False, False, None),
    "u_ids_swapped": (False, False, None),
    "all_distinct": (False, False, None),
    "stored_order_a": (False, False, None),
    "stored_order_u": (False, False, None),
}
MUTATIONS = tuple(TABLE)


@dataclass
class Member:
    name: str
    family: str                  # "generated" | "mutated" | "saturated"
    valA: np.ndarray
    irow: np.ndarray             # 1-based, int32
    jcol: np.ndarray             # 1-based, int32
    dims: tuple                  # (sdx, sdy, sdz)
    n_cond: int
    D: int                       # conducting domains (saturated: conducting boxes)
    expect: tuple                # (recognised under the default pitch, under EC3D_PITCH=2)
    base: str | None = None      # mutated: the generated member it was made from
    mutation: str | None = None
    dclasses: int | None = None  # mutated: classes - the base's classes where recognised and stated
    wrap: str | None = None      # saturated
    extra: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.irow) - 1

    @property
    def csr(self):
        return self.valA, self.irow, self.jcol


# ------------------------------------------------------------------------------------------------ CSR edits
def _rows(irow, jcol):
    return np.repeat(np.arange(len(irow) - 1, dtype=np.int64), np.diff(irow)), np.asarray(jcol, np.int64) - 1


def _from_coo(n, r, c, v):
    """CSR (1-based) with ascending columns in every row; entries keep their values bit for bit."""
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    assert not np.any((np.diff(r) == 0) & (np.diff(c) == 0)), "duplicate entry"
    irow = np.concatenate([[1], 1 + np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return np.ascontiguousarray(v, np.float64), irow, (c + 1).astype(np.int32)


def insert(csr, row, col, value):
    """The matrix with one more stored entry (row, col), 0-based, at its place in ascending column order."""
    valA, irow, jcol = csr
    p0, p1 = irow[row] - 1, irow[row + 1] - 1
    cols = jcol[p0:p1] - 1
    assert col not in cols and 0 <= col < len(irow) - 1
    p = p0 + int(np.searchsorted(cols, col))
    ir = irow.copy()
    ir[row + 1:] += 1
    return np.insert(valA, p, value), ir, np.insert(jcol, p, col + 1).astype(np.int32)


def swap_stored(csr, row):
    """Two adjacent entries of `row` exchanged in place (value and column): same matrix, another stored order."""
    valA, irow, jcol = csr
    p = irow[row] - 1 + (irow[row + 1] - irow[row]) // 2 - 1
    assert irow[row + 1] - irow[row] >= 2 and p >= irow[row] - 1
    valA, jcol = valA.copy(), jcol.copy()
    valA[[p, p + 1]] = valA[[p + 1, p]]
    jcol[[p, p + 1]] = jcol[[p + 1, p]]
    return valA, irow, jcol


def mutate(name, csr, dims, geoC):
    """The edit `name` of TABLE on a recognised matrix of the reference's; geoC [sdz, sdy, sdx] its U ids."""
    valA, irow, jcol = csr
    sdx, sdy, sdz = dims
    plane, nC = sdx * sdy, sdx * sdy * sdz
    nA = 3 * nC
    n = len(irow) - 1
    cond = np.flatnonzero(np.asarray(geoC).reshape(-1) != 0)
    k, j = sdz // 2, sdy // 2
    if name in ("wrap_x", "wrap_zero"):                 # i = 0, j >= 1: the slot -1 is the row end of the same plane
        r = nC + k * plane + j * sdx                    # (an A_y row)
        return insert(csr, r, r - 1, 0.375 if name == "wrap_x" else 0.0)
    if name == "wrap_plane":                            # i = 0, j = 0, k >= 1: the slot -1 lies in the plane before
        r = 2 * nC + k * plane
        return insert(csr, r, r - 1, 0.375)
    if name == "off_plus2":
        r = k * plane + j * sdx + sdx // 2 - 1
        return insert(csr, r, r + 2, 0.375)
    if name == "u_row_two_away":
        m = len(cond) // 2
        return insert(csr, nA + m, int(cond[m]) + 2, 0.375)
    if name == "air_row_u_col":
        air = np.flatnonzero(np.asarray(geoC).reshape(-1) == 0)
        q = int(air[len(air) // 2])
        return insert(csr, nC + q, nA + len(cond) // 2, 0.375)
    if name == "u_ids_swapped":                         # the first and the last U unknown exchanged
        perm = np.arange(n, dtype=np.int64)
        perm[nA], perm[n - 1] = n - 1, nA
        r, c = _rows(irow, jcol)
        return _from_coo(n, perm[r], perm[c], np.asarray(valA, np.float64))
    if name == "all_distinct":                          # no two rows share their coefficients any more
        r, _ = _rows(irow, jcol)
        return valA * (1.0 + (r + 1) * 2.0 ** -30), irow, jcol
    if name == "stored_order_a":
        return swap_stored(csr, k * plane + j * sdx + sdx // 2)
    if name == "stored_order_u":
        return swap_stored(csr, nA + len(cond) // 2)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ saturated
# coefficient of (block 0 .. 3, slot 0 .. 15): fixed, all different, none a power of two
_COEF = np.random.Generator(np.random.PCG64(20251019)).uniform(0.05, 0.45, (4, 16)) * \
    np.where(np.random.Generator(np.random.PCG64(7)).integers(0, 2, (4, 16)) == 1, 1.0, -1.0)
_COEF[:, 3] = 1.0 + np.abs(_COEF).sum(axis=1)           # the diagonal: more than everything else a row can hold


def saturated(dims, boxes, wrap):
    """(valA, irow, jcol, n_cond) of the matrix that fills every admitted slot.  boxes: [((x0, x1), (y0, y1), (z0, z1))]
    of conducting cells, half-open."""
    sdx, sdy, sdz = dims
    plane, nC = sdx * sdy, sdx * sdy * sdz
    nA = 3 * nC
    on = np.zeros((sdz, sdy, sdx), bool)
    for (x0, x1), (y0, y1), (z0, z1) in boxes:
        on[z0:z1, y0:y1, x0:x1] = True
    on = on.reshape(-1)
    cells = np.flatnonzero(on)
    nU = len(cells)
    uid = np.full(nC, -1, np.int64)
    uid[cells] = np.arange(nU)
    step = (1, sdx, plane)
    band = (-plane, -sdx, -1, 0, 1, sdx, plane)
    band_axis = (2, 1, 0, None, 0, 1, 2)
    band_sign = (-1, -1, -1, 0, 1, 1, 1)
    q_all = np.arange(nC, dtype=np.int64)
    coord = (q_all % sdx, q_all // sdx % sdy, q_all // plane)
    size = (sdx, sdy, sdz)

    def reach(q, axis, m):
        """May the entry of the cells q that lies m steps along `axis` be stored?  (the target's existence is the
        caller's business.)"""
        if wrap == "all" or m == 0:
            return np.ones(len(q), bool)
        t = coord[axis][q] + m
        inside = (t >= 0) & (t < size[axis])
        if wrap == "x" and axis == 0:                   # across a row end, but not out of the plane
            tq = q + m
            return inside | ((tq >= 0) & (tq < nC) & (tq // plane == q // plane))
        return inside

    R, Cc, V = [], [], []

    def put(rows, cols, block, slot):
        R.append(rows)
        Cc.append(cols)
        V.append(np.full(len(rows), _COEF[block, slot]))

    for d in range(3):                                  # A rows: bands, then U slots
        for b in range(7):
            ok = np.ones(nC, bool) if b == 3 else reach(q_all, band_axis[b], band_sign[b])
            col = d * nC + q_all + band[b]
            ok &= (col >= 0) & (col < nA)
            put(d * nC + q_all[ok], col[ok], d, b)
        for m in range(-2, 3):
            t = cells + m * step[d]
            ok = reach(cells, d, m) & (t >= 0) & (t < nC)
            ok[ok] = on[t[ok]]
            put(d * nC + cells[ok], nA + uid[t[ok]], d, 7 + m + 2)
    urow = nA + np.arange(nU, dtype=np.int64)
    for d in range(3):                                  # U rows: A slots, then U bands
        for jj in (-1, 0, 1):
            t = cells + jj * step[d]
            ok = reach(cells, d, jj) & (t >= 0) & (t < nC)
            put(urow[ok], d * nC + t[ok], 3, 7 + 3 * d + jj + 1)
    for b in range(7):
        t = cells + band[b]
        ok = (np.ones(nU, bool) if b == 3 else reach(cells, band_axis[b], band_sign[b])) & (t >= 0) & (t < nC)
        ok[ok] = on[t[ok]]
        put(urow[ok], nA + uid[t[ok]], 3, b)
    valA, irow, jcol = _from_coo(nA + nU, np.concatenate(R), np.concatenate(Cc), np.concatenate(V))
    return valA, irow, jcol, nU


# (name, (sdx, sdy, sdz), conducting boxes)
SATURATED_BOXES = (
    ("interior_12x10x9", (12, 10, 9), [((3, 9), (2, 8), (2, 7))]),
    ("fills_xy_16x8x10", (16, 8, 10), [((0, 16), (0, 8), (3, 7))]),
    ("fills_y_plane0_14x9x8", (14, 9, 8), [((4, 11), (0, 9), (0, 4))]),
    ("odd_two_boxes_11x9x10", (11, 9, 10), [((0, 5), (2, 7), (1, 5)), ((6, 11), (3, 9), (5, 10))]),
)


def crosses_plane(csr, dims, n_cond_cells):
    """Does any stored entry join cells of different xy planes other than straight along z?  (what tile-aligned planes
    cannot hold.)  n_cond_cells: scan-order cell of every U unknown."""
    valA, irow, jcol = csr
    sdx, sdy, sdz = dims
    plane, nC = sdx * sdy, sdx * sdy * sdz
    r, c = _rows(irow, jcol)
    cell = np.concatenate([np.tile(np.arange(nC, dtype=np.int64), 3), np.asarray(n_cond_cells, np.int64)])
    dq = cell[c] - cell[r]
    return bool(np.any((cell[c] // plane != cell[r] // plane) & (np.abs(dq) % plane != 0)))


# --------------------------------------------------------------------------------------------------- corpus
_corpus = None


def corpus(oracle):
    """Every member, made once.  oracle: the module oracle.oracle (built)."""
    global _corpus
    if _corpus is not None:
        return _corpus
    from test_generated_av_host import oracle_code
    out, bases = [], {}
    sources = [(f"seed{s}", AG.generate(s)) for s in tuple(AG.CORPUS) + tuple(EXTRA_SEEDS)]
    sources += [(f"near_{a}{s}", AG.near_face(a, s)) for a in "xyz" for s in "mp"]
    for name, args in sources:
        if oracle_code(oracle, args) != 0:
            continue
        geo, geoC = args[0], args[1]
        m = oracle.gen_sparse_matrix(*args)
        sdz, sdy, sdx = geo.shape
        ok = MD.structured_applies(geo, geoC)
        mem = Member(name, "generated", m["valA"], m["irow"], m["jcol"], (sdx, sdy, sdz),
                     int(np.count_nonzero(geoC)), len(MD.conductors(geo, geoC)), (ok, ok), extra=dict(geoC=geoC))
        out.append(mem)
        bases[name] = mem
    for seed in MUTATION_BASES:
        b = bases[f"seed{seed}"]
        for mut in MUTATIONS:
            valA, irow, jcol = mutate(mut, b.csr, b.dims, b.extra["geoC"])
            d0, d1, dcls = TABLE[mut]
            out.append(Member(f"{b.name}_{mut}", "mutated", valA, irow, jcol, b.dims, b.n_cond, b.D, (d0, d1),
                              base=b.name, mutation=mut, dclasses=dcls))
    for name, dims, boxes in SATURATED_BOXES:
        for wrap in WRAPS:
            valA, irow, jcol, nU = saturated(dims, boxes, wrap)
            out.append(Member(f"sat_{name}_{wrap}", "saturated", valA, irow, jcol, dims, nU, len(boxes),
                              (True, wrap != "all"), wrap=wrap, extra=dict(boxes=boxes)))
    _corpus = out
    return out
