"""Generated CSR matrices that are not grid stencils: inputs of ec3d_set_matrix_csr / sprsbcgstabwr_ that take the
generic band + tail path, or the specialised 7-band kernels on something other than the 7-point grid operator.

case(name) -> (valA, irow, jcol, intent): the reference's 1-based CSR triple (float64, int32, int32) and what the case
is there for -- intent = dict(n, nbands, band_offset, tail_rows, dict, solve, zero):

* nbands / band_offset / tail_rows: the storage form the case must reach (default tile and slice sizes, 512 / 64),
  written down by hand here and checked against the restatement of the split rule (tests/bands_tail_numpy.py) by
  tests/test_generated_csr_host.py;
* dict: the dictionary form of seven bands is possible (at most 256 distinct coefficient 7-tuples);
* solve: strictly diagonally dominant (diagonal = 1.5 x the row's absolute off-diagonal sum, off-diagonals of mixed
  sign, unsymmetric), so BiCGSTAB converges in a few dozen iterations;
* zero: the matrix stores explicit 0.0 entries (they do not survive ec3d_export_csr).

Everything is deterministic (PCG64 seeded by a checksum of the case's name) and vectorised: the largest case has
2^21 + 3 rows.  Rows and offsets are 0-based in this file; the triple that comes out is 1-based.
"""
from __future__ import annotations

import zlib

import numpy as np

N0 = 1537                       # three full tiles of 512 rows plus one row: n_pad = 2048
TRI = (-1, 0, 1)
WRAP128 = (-2048, -128, -1, 0, 1, 128, 2048)        # n = 128 * 16 * 12
WRAP256 = (-2048, -256, -1, 0, 1, 256, 2048)        # n = 256 * 8 * 9
N128, N256 = 128 * 16 * 12, 256 * 8 * 9


def _values(rng, k):
    """k coefficients of either sign, 0.5 <= |v| < 1.5."""
    return rng.uniform(0.5, 1.5, k) * rng.choice((-1.0, 1.0), k)


class _Rows:
    """Entries (row, col, value, key) gathered in any order; a row's stored order is ascending key."""

    def __init__(self, n):
        self.n, self.r, self.c, self.v, self.k = n, [], [], [], []

    def add(self, rows, cols, vals, key):
        rows = np.atleast_1d(np.asarray(rows, np.int64))
        self.r.append(rows)
        self.c.append(np.broadcast_to(np.asarray(cols, np.int64), rows.shape))
        self.v.append(np.broadcast_to(np.asarray(vals, np.float64), rows.shape))
        self.k.append(np.broadcast_to(np.asarray(key, np.float64), rows.shape))

    def bands(self, rng, offsets, keep=None):
        """Every in-range slot of every offset (of the rows `keep(rows, offset)` selects), keyed by the offset."""
        for d in offsets:
            rows = np.arange(max(0, -d), min(self.n, self.n - d), dtype=np.int64)
            if keep is not None:
                rows = rows[keep(rows, d)]
            self.add(rows, rows + d, _values(rng, len(rows)), d)

    def csr(self, dominant=False):
        r, c, v, k = (np.concatenate(a) for a in (self.r, self.c, self.v, self.k))
        order = np.lexsort((k, r))
        r, c, v = r[order], c[order], v[order].copy()
        if dominant:
            diag = c == r
            off = np.bincount(r[~diag], np.abs(v[~diag]), self.n)
            assert np.array_equal(np.bincount(r[diag], minlength=self.n), np.ones(self.n)), "one diagonal entry per row"
            # a row without off-diagonals keeps its own diagonal value (|v| >= 0.5)
            v[diag] = np.where(off[r[diag]] > 0, 1.5 * off[r[diag]], np.abs(v[diag]))
        irow = np.concatenate([[1], 1 + np.cumsum(np.bincount(r, minlength=self.n))]).astype(np.int32)
        return v, irow, (c + 1).astype(np.int32)


def _intent(n, offsets, tail_rows=0, dict=False, solve=False, zero=False):
    return {"n": n, "nbands": len(offsets), "band_offset": [int(d) for d in sorted(offsets)], "tail_rows": tail_rows,
            "dict": dict, "solve": solve, "zero": zero}


def _banded(rng, n, offsets, solve):
    m = _Rows(n)
    m.bands(rng, offsets)
    return (*m.csr(dominant=solve), _intent(n, offsets, solve=solve))


def _grid2d(rng, sdx, sdy, reach, solve):
    """A 2-D stencil on sdx x sdy: every neighbour (dx, dy) of `reach` that lies inside the grid."""
    n = sdx * sdy
    i = np.arange(n) % sdx
    m = _Rows(n)
    offsets = sorted(dx + sdx * dy for dx, dy in reach)
    for dx, dy in reach:
        d = dx + sdx * dy
        m.bands(rng, [d], keep=lambda rows, _d: (i[rows] + dx >= 0) & (i[rows] + dx < sdx))
    return (*m.csr(dominant=solve), _intent(n, offsets, solve=solve))


def _stencil27(rng, solve):
    """27-point stencil on 12 x 11 x 10: every offset is carried by >= 75 % of the rows, so there are 27 candidates for
    16 bands.  Rows that carry (dx, dy, dz): (12 - |dx|)(11 - |dy|)(10 - |dz|) -- 1320; 1210, 1200, 1188 (two each);
    1100, 1089, 1080 (four each); 990 (eight).  The 15 most frequent are certain; the 16th is one of the four offsets
    +-12 +-132 that 1080 rows carry, and the split rule gives it to the smallest of them, -144."""
    sdx, sdy, sdz = 12, 11, 10
    n = sdx * sdy * sdz
    q = np.arange(n)
    i, j = q % sdx, (q // sdx) % sdy
    m = _Rows(n)
    kept = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                d = dx + sdx * dy + sdx * sdy * dz
                m.bands(rng, [d], keep=lambda rows, _d: ((i[rows] + dx >= 0) & (i[rows] + dx < sdx) &
                                                         (j[rows] + dy >= 0) & (j[rows] + dy < sdy)))
                if abs(dx) + abs(dy) + abs(dz) <= 1 or (abs(dx) + abs(dy) + abs(dz) == 2 and not (dy and dz)):
                    kept.append(d)
    kept.append(-144)
    assert len(kept) == 16
    # a row has a tail when it stores an entry off the 16 bands: dy dz != 0 and its offset is not -144 (the entries in
    # ascending column order: whatever follows the first such entry goes with it)
    k = q // (sdx * sdy)
    tail = np.zeros(n, bool)
    for dz in (-1, 1):
        for dy in (-1, 1):
            for dx in (-1, 0, 1):
                if dx + sdx * dy + sdx * sdy * dz == -144:
                    continue
                tail |= ((i + dx >= 0) & (i + dx < sdx) & (j + dy >= 0) & (j + dy < sdy) & (k + dz >= 0) & (k + dz < sdz))
    return (*m.csr(dominant=solve), _intent(n, kept, tail_rows=int(tail.sum()), solve=solve))


def _threshold(rng):
    """Tridiagonal, plus offset +9 on 599 rows (39 % of 1537: under the 40 % rule, 614.8 rows) and +13 on 631 (41 %)."""
    m = _Rows(N0)
    m.bands(rng, TRI)
    r9 = rng.choice(N0 - 13, 599, replace=False)
    r13 = rng.choice(N0 - 13, 631, replace=False)
    m.add(r9, r9 + 9, _values(rng, 599), 9)
    m.add(r13, r13 + 13, _values(rng, 631), 13)
    return (*m.csr(), _intent(N0, (-1, 0, 1, 13), tail_rows=599))


def _sampling(rng):
    """n = 2^21 + 3: band discovery looks at every second row (stride n // 2^20 = 2: rows 0, 2, 4, ...).  Offset +7 is
    carried by the odd rows only -- half of all rows, but none of the sample -- so it is no band and every such row has
    a one-entry tail."""
    n = (1 << 21) + 3
    m = _Rows(n)
    m.bands(rng, TRI)
    odd = np.arange(1, n - 7, 2, dtype=np.int64)
    m.add(odd, odd + 7, _values(rng, len(odd)), 7)
    return (*m.csr(), _intent(n, TRI, tail_rows=len(odd)))


def _wrap(rng, offsets, n, classes, solve, extra=False):
    """Seven bands at the offsets of a 7-point grid operator with EVERY in-range slot nonzero: the +-1 slots at the ends
    of an x-row and the +-sdx slots at the ends of a plane too, which a grid operator leaves empty.  classes > 0: the
    rows draw their seven coefficients from that many 7-tuples (at most 7 x classes distinct tuples once the slots that
    fall outside the matrix are zero: first / last row, x-row and plane); 0: every row its own."""
    m = _Rows(n)
    if classes:
        cls = rng.integers(0, classes, n)
        table = _values(rng, classes * 7).reshape(classes, 7)
        for b, d in enumerate(offsets):
            rows = np.arange(max(0, -d), min(n, n - d), dtype=np.int64)
            m.add(rows, rows + d, table[cls[rows], b], d)
    else:
        m.bands(rng, offsets)
    tail = 0
    if extra:                   # one row carries an eighth entry: a tail, so the matrix is no grid operator any more
        m.add(n // 2 + 77, 5, 0.625, 1e9)
        tail = 1
    return (*m.csr(dominant=solve), _intent(n, offsets, tail_rows=tail, dict=classes > 0, solve=solve))


def _tri_with(rng, n=N0, drop=(), extra=(), solve=False, tail_rows=None):
    """Tridiagonal base with rows emptied (`drop`) and extra entries (row, col, value, key): a key orders the entry
    among the row's band entries, whose keys are their offsets -1, 0, 1."""
    m = _Rows(n)
    drop = np.asarray(sorted(drop), np.int64)
    m.bands(rng, TRI, keep=lambda rows, d: ~np.isin(rows, drop))
    for r, c, v, k in extra:
        m.add(r, c, v, k)
    valA, irow, jcol = m.csr(dominant=solve)
    offs = TRI if n > 1 else (0,)
    tr = len({int(e[0]) for e in extra}) if tail_rows is None else tail_rows
    return valA, irow, jcol, _intent(n, offs, tail_rows=tr, solve=solve)


def _far(rng, rows, n=N0):
    """One entry per row in a column at least 20 away from the diagonal (on no band), stored behind the bands."""
    rows = np.asarray(rows, np.int64)
    cols = (rows + rng.integers(20, n - 20, len(rows))) % n
    return [(int(r), int(c), float(v), 1e9) for r, c, v in zip(rows, cols, _values(rng, len(rows)))]


def _long_row(rng, solve):
    cols = rng.choice(np.setdiff1d(np.arange(N0), [699, 700, 701]), 300, replace=False)       # stored unsorted
    extra = [(700, int(c), float(v), 1e9 + q) for q, (c, v) in enumerate(zip(cols, _values(rng, 300)))]
    return _tri_with(rng, extra=extra, solve=solve)


def _reordered(rng, kind):
    """Rows whose stored order breaks the ascending-band rule; what stays on the bands is the leading run."""
    rows = rng.choice(np.arange(2, N0 - 2), 40, replace=False)
    m = _Rows(N0)
    m.bands(rng, TRI, keep=lambda r, d: ~np.isin(r, rows))
    for r in rows:
        a, b, c, e = (float(v) for v in _values(rng, 4))
        if kind == "band_nonband_band":         # -1 | far, 0, +1
            seq = [(r - 1, a), ((r + 700) % N0, e), (r, b), (r + 1, c)]
        elif kind == "duplicates":              # -1, 0 | 0, +1
            seq = [(r - 1, a), (r, b), (r, e), (r + 1, c)]
        else:                                   # descending: +1 | 0, -1
            seq = [(r + 1, c), (r, b), (r - 1, a)]
        for q, (col, v) in enumerate(seq):
            m.add(r, col, v, q)
    return (*m.csr(), _intent(N0, TRI, tail_rows=len(rows)))


def _extreme(rng):
    """Subnormal coefficients and coefficients of 1e+-150 beside ordinary ones, on the bands and in a tail."""
    pool = np.array([5e-324, 3e-310, -2e-308, 1e150, -1e150, 1e-150, -1e-150, 1.0, -0.75])
    valA, irow, jcol, it = _tri_with(rng, extra=_far(rng, rng.choice(N0, 90, replace=False)))
    valA = np.where(rng.random(len(valA)) < 0.5, valA, pool[rng.integers(0, len(pool), len(valA))])
    assert np.all(valA != 0.0) and np.any(np.abs(valA) < 2.3e-308) and np.any(np.abs(valA) > 1e149)
    return valA, irow, jcol, it


def _explicit_zeros(rng):
    extra = _far(rng, [10, 600, 1500]) + [(1200, 3, 0.0, 1e9), (1200, 7, 0.25, 2e9)]
    valA, irow, jcol, it = _tri_with(rng, extra=extra, tail_rows=4)
    valA = valA.copy()
    valA[rng.choice(len(valA), 200, replace=False)] = 0.0           # band slots and tail entries alike
    it["zero"] = True
    return valA, irow, jcol, it


_BUILD = {
    # ---- band counts
    "nb1": lambda g: _banded(g, N0, (0,), True),
    "nb2": lambda g: _banded(g, N0, (0, 5), False),
    "nb3": lambda g: _banded(g, N0, TRI, True),
    "nb5": lambda g: _grid2d(g, 40, 39, [(0, -1), (-1, 0), (0, 0), (1, 0), (0, 1)], True),
    "nb9": lambda g: _grid2d(g, 40, 39, [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], True),
    "nb16": lambda g: _banded(g, N0, tuple(range(-8, 8)), True),
    "stencil27": lambda g: _stencil27(g, True),
    "threshold": _threshold,
    "sampling": _sampling,
    # ---- seven bands that are not the 7-point grid
    "seven_m3p3": lambda g: _banded(g, N0, tuple(range(-3, 4)), True),
    "seven_p1p7": lambda g: _banded(g, N0, tuple(range(1, 8)), False),
    "wrap128_dict": lambda g: _wrap(g, WRAP128, N128, 24, True),
    "wrap128_dia": lambda g: _wrap(g, WRAP128, N128, 0, True),
    "wrap256_dict": lambda g: _wrap(g, WRAP256, N256, 24, True),
    "wrap256_dia": lambda g: _wrap(g, WRAP256, N256, 0, False),
    "wrap128_extra": lambda g: _wrap(g, WRAP128, N128, 24, False, extra=True),
    # ---- tail shapes on the tridiagonal base
    "empty_rows": lambda g: _tri_with(g, drop=[0, 5, 511, 512, 1024, 1536] + list(g.choice(np.arange(20, 1500), 20,
                                                                                           replace=False))),
    "long_row": lambda g: _long_row(g, True),
    "tail63": lambda g: _tri_with(g, extra=_far(g, g.choice(N0, 63, replace=False))),
    "tail64": lambda g: _tri_with(g, extra=_far(g, g.choice(N0, 64, replace=False))),
    "tail65": lambda g: _tri_with(g, extra=_far(g, g.choice(N0, 65, replace=False))),
    "tail_last_tile": lambda g: _tri_with(g, extra=_far(g, [1536])),
    "tail_tiles_0_2": lambda g: _tri_with(g, extra=_far(g, np.concatenate([g.choice(512, 30, replace=False),
                                                                           1024 + g.choice(512, 30, replace=False)]))),
    "band_nonband_band": lambda g: _reordered(g, "band_nonband_band"),
    "duplicates": lambda g: _reordered(g, "duplicates"),
    "descending": lambda g: _reordered(g, "descending"),
    "explicit_zeros": _explicit_zeros,
    "extreme_values": _extreme,
    # ---- sizes
    "n1": lambda g: _tri_with(g, n=1),
    "n2": lambda g: _tri_with(g, n=2),
    "n511": lambda g: _tri_with(g, n=511),
    "n512": lambda g: _tri_with(g, n=512),
    "n513": lambda g: _tri_with(g, n=513, solve=True),
}
CASES = tuple(_BUILD)
SOLVE = ("nb1", "nb3", "nb5", "nb9", "nb16", "stencil27", "seven_m3p3", "wrap128_dict", "wrap128_dia", "wrap256_dict",
         "long_row", "n513")
WRAP = ("wrap128_dict", "wrap128_dia", "wrap256_dict", "wrap256_dia")
WRAP_OFFSETS = {"wrap128_dict": WRAP128, "wrap128_dia": WRAP128, "wrap128_extra": WRAP128, "wrap256_dict": WRAP256,
                "wrap256_dia": WRAP256}
DROPIN = ("nb3", "stencil27", "wrap128_dict")
_cache = {}


def case(name):
    if name not in _cache:
        rng = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))
        valA, irow, jcol, intent = _BUILD[name](rng)
        for a in (valA, irow, jcol):
            a.setflags(write=False)
        _cache[name] = (valA, irow, jcol, intent)
    return _cache[name]


def wrap_slots(name):
    """0-based (row, offset) of every wrap slot of a wrap case: +-1 at the ends of an x-row, +-sdx at the ends of a
    plane -- the slots a 7-point grid operator leaves empty and that lie inside the matrix."""
    offs = WRAP_OFFSETS[name]
    sdx, kdz = offs[5], offs[6]
    n = case(name)[3]["n"]
    r = np.arange(n)
    out = []
    for d, sel in ((-1, r % sdx == 0), (1, r % sdx == sdx - 1), (-sdx, r % kdz < sdx), (sdx, r % kdz >= kdz - sdx)):
        rows = r[sel & (r + d >= 0) & (r + d < n)]
        out.append((rows, d))
    return out
