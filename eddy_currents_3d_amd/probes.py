"""Probe sets for EC3DSolver.set_probes: pure host helpers, no GPU and no library.

A probe is a cell of the box, numbered ``i + j*sdx + k*sdx*sdy`` from 0; ``dims`` is ``(sdx, sdy, sdz)`` throughout and
a corner is ``(i, j, k)``.  ``probe_line`` and ``probe_box`` build the usual sets -- a line across the plate (the
reference README's Line X and Line Y), a point, one plane of the field --, ``cells_to_ijk`` turns numbers back into
indices, and the CSV helpers write and read what ``python -m eddy_currents_3d_amd.run --probes FILE`` produces.
"""
from __future__ import annotations

import numpy as np

COMPONENTS = ("ax", "ay", "az", "eddy_x", "eddy_y", "eddy_z", "source_x", "source_y", "source_z", "bx", "by", "bz", "u")
CSV_HEADER = "step,T,probe,i,j,k," + ",".join(COMPONENTS)
KEYS = (("a", 3), ("eddy", 3), ("source", 3), ("b", 3), ("u", 1))   # EC3DSolver.probe_sample's arrays, in component order


def _corner(c, dims, what):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or len(dims) != 3:
        raise ValueError(f"{what}: a corner is (i, j, k) and dims is (sdx, sdy, sdz)")
    if any(not 0 <= v < int(d) for v, d in zip(c, dims)):
        raise ValueError(f"{what}: cell {c} is outside the box {tuple(int(d) for d in dims)}")
    return c


def probe_line(c0, c1, dims):
    """The cells from c0 = (i0, j0, k0) to c1 = (i1, j1, k1), both included: with n = max(|di|, |dj|, |dk|), step
    t = 0 .. n is the cell i0 + (2*t*di + n) // (2*n) (floor division: the nearest cell, halves upwards), likewise j and
    k.  n + 1 cells without duplicates -- the longest axis advances by one every step --; n = 0 is one cell.  int64
    cell numbers; ValueError when an end lies outside ``dims``."""
    c0, c1 = _corner(c0, dims, "probe_line"), _corner(c1, dims, "probe_line")
    d = [b - a for a, b in zip(c0, c1)]
    n = max(abs(v) for v in d)
    t = np.arange(n + 1, dtype=np.int64)
    i, j, k = (a + ((2 * t * v + n) // (2 * n) if n else 0 * t) for a, v in zip(c0, d))
    sdx, sdy = int(dims[0]), int(dims[1])
    return i + j * sdx + k * sdx * sdy


def probe_box(lo, hi, dims):
    """Every cell of the box with the inclusive corners lo and hi (in any order per axis), in scan order, i fastest; a
    plane is a box one cell thick.  int64 cell numbers; ValueError when a corner lies outside ``dims``."""
    lo, hi = _corner(lo, dims, "probe_box"), _corner(hi, dims, "probe_box")
    r = [np.arange(min(a, b), max(a, b) + 1, dtype=np.int64) for a, b in zip(lo, hi)]
    sdx, sdy = int(dims[0]), int(dims[1])
    return (r[0][None, None, :] + r[1][None, :, None] * sdx + r[2][:, None, None] * (sdx * sdy)).reshape(-1)


def cells_to_ijk(cells, dims):
    """(n, 3) int64 array of (i, j, k) of every cell number; ValueError when one lies outside ``dims``."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    sdx, sdy, sdz = (int(d) for d in dims)
    if cells.size and (cells.min() < 0 or cells.max() >= sdx * sdy * sdz):
        raise ValueError(f"cells_to_ijk: a cell lies outside the box {(sdx, sdy, sdz)}")
    return np.stack([cells % sdx, cells // sdx % sdy, cells // (sdx * sdy)], axis=1)


def stack(sample):
    """EC3DSolver.probe_sample's / probe_read's dict -> one float64 array (..., nprobes, 13) in component order."""
    return np.concatenate([np.asarray(sample[k], np.float64).reshape(np.shape(sample["u"]) + (w,)) for k, w in KEYS], axis=-1)


def csv_rows(step, T, cells, dims, values):
    """CSV lines of one step: ``values`` is that step's (nprobes, 13) array, floats at repr() precision."""
    ijk = cells_to_ijk(cells, dims)
    values = np.asarray(values, np.float64)
    return [",".join([str(int(step)), repr(float(T)), str(p), str(int(i)), str(int(j)), str(int(k))]
                     + [repr(float(v)) for v in values[p]]) for p, (i, j, k) in enumerate(ijk)]


def read_csv(path):
    """What csv_rows wrote, back: dict(step, probe (int64 arrays, one entry per line), T (float64), ijk (n, 3), values
    (n, 13) float64) -- the same doubles, repr() round-trips."""
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or lines[0] != CSV_HEADER:
        raise ValueError(f"{path}: not a probe file (header {CSV_HEADER!r} expected)")
    rows = [line.split(",") for line in lines[1:] if line]
    return dict(step=np.array([int(r[0]) for r in rows], np.int64), T=np.array([float(r[1]) for r in rows], np.float64),
                probe=np.array([int(r[2]) for r in rows], np.int64),
                ijk=np.array([[int(v) for v in r[3:6]] for r in rows], np.int64).reshape(-1, 3),
                values=np.array([[float(v) for v in r[6:]] for r in rows], np.float64).reshape(-1, len(COMPONENTS)))


def _triple(text, what):
    try:
        c = tuple(int(v) for v in text.split(","))
    except ValueError:
        c = ()
    if len(c) != 3:
        raise ValueError(f"{what}: I,J,K expected, got {text!r}")
    return c


def parse_point(text):
    """'I,J,K' -> (i, j, k)."""
    return _triple(text, "--probe")


def parse_span(text, what="--probe-line"):
    """'I0,J0,K0:I1,J1,K1' -> ((i0, j0, k0), (i1, j1, k1))."""
    ends = text.split(":")
    if len(ends) != 2:
        raise ValueError(f"{what}: I0,J0,K0:I1,J1,K1 expected, got {text!r}")
    return _triple(ends[0], what), _triple(ends[1], what)


def cells_from_options(points, lines, boxes, dims):
    """The probe list of the command line: the points, then the lines, then the boxes, each in the order given."""
    parts = [probe_box(parse_point(p), parse_point(p), dims) for p in points or ()]
    parts += [probe_line(*parse_span(s, "--probe-line"), dims) for s in lines or ()]
    parts += [probe_box(*parse_span(s, "--probe-box"), dims) for s in boxes or ()]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)
