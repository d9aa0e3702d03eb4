"""Generated 7-point operators on a box, as a caller of ec3d_set_matrix_csr + ec3d_set_precond_grid would bring them.

case(name, dims) -> (valA, irow, jcol, c): the reference's 1-based CSR triple (float64, int32, int32), rows numbered
r = i + j sdx + k sdx sdy, every row's entries in ascending column order, and the same coefficients as a (7, n) band
array in offset order (-z, -y, -x, diag, +x, +y, +z), zero where the neighbour lies beyond the box.

* "poisson": oracle.poisson_csr itself (default spacing and BND): what ec3d_assemble_poisson builds.
* "jump":    -div(kappa grad u), kappa = 1 outside and 10^3 inside an off-centre sub-box (cells [a // 4, a // 4 +
             max(2, a // 3)) of every axis a), on spacings (0.002, 0.003, 0.005).  The face coefficient between two
             cells is the harmonic mean 2 ka kb / (ka + kb) over h^2; a face of the box is a ghost-cell Dirichlet face
             (u_ghost = -u_cell: 2 kappa / h^2 on the diagonal).  Symmetric, strictly diagonally dominant in the rows
             next to a face, weakly elsewhere.
* "convect": jump's diffusion with kappa = 1 everywhere plus first-order upwind convection along (1, -0.5, 0.25): the
             velocity is s (1, -0.5, 0.25) with s = 1000, so the cell Peclet numbers |u_a| h_a / kappa are (2, 1.5,
             1.25).  The upwind neighbour of a cell at an inflow face is a zero ghost value (the coupling is dropped,
             the diagonal keeps |u_a| / h_a).  A nonsymmetric M-matrix: off-diagonals <= 0, rows diagonally dominant.

drop_bands(valA, irow, jcol, c, dims, qs): the same matrix without the entries of the bands qs (a 5-band matrix when
the +-z bands of a two-plane box go).  with_entry: one more entry at the end of a row (a tail entry).
Everything is deterministic; results are cached and read-only."""
from __future__ import annotations

import numpy as np

DELTA = (0.002, 0.003, 0.005)
KAPPA_IN = 1.0e3
DIRECTION = (1.0, -0.5, 0.25)
SPEED = 1000.0
CASES = ("poisson", "jump", "convect")
# band q: (axis of the [k, j, i] array, direction)
_Q = ((0, -1), (1, -1), (2, -1), None, (2, 1), (1, 1), (0, 1))
_cache = {}


def offsets(dims):
    sdx, sdy, _ = dims
    return (-sdx * sdy, -sdx, -1, 0, 1, sdx, sdx * sdy)


def _neighbour(F, axis, sgn, fill):
    """F at the neighbour along `axis` in direction sgn; `fill` beyond the box."""
    out = np.full_like(F, fill)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    if sgn < 0:
        dst[axis], src[axis] = slice(1, None), slice(None, -1)
    else:
        dst[axis], src[axis] = slice(None, -1), slice(1, None)
    out[tuple(dst)] = F[tuple(src)]
    return out


def _inside(shape, axis, sgn):
    return _neighbour(np.ones(shape, bool), axis, sgn, False)


def kappa_of(dims, jump=True):
    sdx, sdy, sdz = dims
    k = np.ones((sdz, sdy, sdx))
    if jump:
        k[tuple(slice(a // 4, a // 4 + max(2, a // 3)) for a in (sdz, sdy, sdx))] = KAPPA_IN
    return k


def _diffusion(dims, kappa):
    """(7, sdz, sdy, sdx) bands of -div(kappa grad u) with ghost-cell Dirichlet faces."""
    h = {2: DELTA[0], 1: DELTA[1], 0: DELTA[2]}     # spacing of array axis 2 = x, 1 = y, 0 = z
    c = np.zeros((7,) + kappa.shape)
    for q, ad in enumerate(_Q):
        if ad is None:
            continue
        axis, sgn = ad
        kn = _neighbour(kappa, axis, sgn, 0.0)
        ins = _inside(kappa.shape, axis, sgn)
        face = np.where(ins, 2.0 * kappa * kn / (kappa + np.where(ins, kn, 1.0)), 0.0) / h[axis] ** 2
        c[q] = -face
        c[3] = c[3] + np.where(ins, face, 2.0 * kappa / h[axis] ** 2)
    return c


def _convection(dims, c):
    h = {2: DELTA[0], 1: DELTA[1], 0: DELTA[2]}
    vel = {2: SPEED * DIRECTION[0], 1: SPEED * DIRECTION[1], 0: SPEED * DIRECTION[2]}
    shape = c.shape[1:]
    for q, ad in enumerate(_Q):
        if ad is None:
            continue
        axis, sgn = ad
        if vel[axis] * sgn >= 0:        # the upwind neighbour lies against the velocity
            continue
        w = abs(vel[axis]) / h[axis]
        c[q] = c[q] - np.where(_inside(shape, axis, sgn), w, 0.0)
        c[3] = c[3] + w
    return c


def bands_to_csr(dims, c, skip=()):
    """1-based CSR of the band array c (7, n): every slot whose neighbour lies inside the box, in offset order, the
    bands `skip` left out."""
    sdx, sdy, sdz = dims
    n = sdx * sdy * sdz
    shape = (sdz, sdy, sdx)
    rows, cols, vals = [], [], []
    r = np.arange(n)
    for q, (ad, off) in enumerate(zip(_Q, offsets(dims))):
        if q in skip:
            continue
        m = np.ones(n, bool) if ad is None else _inside(shape, *ad).reshape(-1)
        rows.append(r[m])
        cols.append(r[m] + off)
        vals.append(c[q][m])
    rows, cols, vals = (np.concatenate(a) for a in (rows, cols, vals))
    order = np.lexsort((cols, rows))
    irow = np.concatenate([[1], 1 + np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return vals[order].astype(np.float64), irow, (cols[order] + 1).astype(np.int32)


def _build(name, dims):
    if name == "poisson":
        from oracle import oracle as O
        import mg_numpy as M
        valA, irow, jcol = O.poisson_csr(*dims)
        return valA, irow, jcol, M.bands_of(*dims, (0.00333, 0.00333, 0.00333))
    c = _diffusion(dims, kappa_of(dims, jump=name == "jump"))
    if name == "convect":
        c = _convection(dims, c)
    c = np.ascontiguousarray(c.reshape(7, -1))
    return (*bands_to_csr(dims, c), c)


def case(name, dims):
    key = (name, tuple(dims))
    if key not in _cache:
        out = _build(name, tuple(dims))
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def drop_bands(c, dims, qs):
    """(valA, irow, jcol, c) of the operator c without the bands qs."""
    c = c.copy()
    c[list(qs)] = 0.0
    return (*bands_to_csr(dims, c, skip=qs), c)


def with_entry(valA, irow, jcol, row, col, value):
    """The triple with one more entry (0-based row, col) stored at the end of its row."""
    p = int(irow[row + 1]) - 1
    irow2 = irow.copy()
    irow2[row + 1:] += 1
    return np.insert(valA, p, value), irow2, np.insert(jcol, p, col + 1).astype(np.int32)


def set_entry(valA, irow, jcol, row, col, value):
    """The triple with the stored entry (0-based row, col) replaced."""
    p0, p1 = int(irow[row]) - 1, int(irow[row + 1]) - 1
    p = p0 + int(np.flatnonzero(jcol[p0:p1] == col + 1)[0])
    out = valA.copy()
    out[p] = value
    return out, irow, jcol
