"""float64 numpy restatement of the four point vectors of field_N.vtk (writeVtk_field, src/utilites.f90:222-289).

Written from the reference's loops: the same expressions in the same order, evaluated in float64 and rounded to
float32 once (REAL(.., 4)).  Uaf = x, Jaf = b in the reference's numbering [Ax | Ay | Az | U]; arrays [k, j, i].
"""
from __future__ import annotations

import numpy as np

EDDY_SCALE = -0.07957747154594766788444e7   # :239


def _clamped(a, ax):
    """a(n_plus) - a(n_minus) along array axis ax, the neighbour index clamped to the cell itself at the box faces
    (:280-284)."""
    n = a.shape[ax]
    ip = np.minimum(np.arange(n) + 1, n - 1)
    im = np.maximum(np.arange(n) - 1, 0)
    return np.take(a, ip, axis=ax) - np.take(a, im, axis=ax)


def fields(geoPHYS_C, delta, x, b):
    """dict(A, eddy (None without conductors), source, B), each float32 (ncells, 3), as EC3DSolver.vtk_fields."""
    gc = np.asarray(geoPHYS_C)
    shape = gc.shape
    N = gc.size
    cond = gc.reshape(-1) != 0
    U = [np.asarray(x[c * N:(c + 1) * N], np.float64) for c in range(3)]
    J = [np.asarray(b[c * N:(c + 1) * N], np.float64) for c in range(3)]
    fa = np.stack(U, axis=1).astype(np.float32)                                 # :222-233
    if cond.any():                                                              # size_PHYS_C /= 0
        fe = np.stack([np.where(cond, EDDY_SCALE * j, 0.0) for j in J], axis=1).astype(np.float32)   # :237-250
        fs = np.stack([np.where(cond, 0.0, j) for j in J], axis=1).astype(np.float32)                # :253-264
    else:
        fe = None
        fs = np.stack(J, axis=1).astype(np.float32)                             # :267-273
    ax, ay, az = (u.reshape(shape) for u in U)
    dx, dy, dz = (float(d) for d in delta)
    X, Y, Z = 2, 1, 0                                                           # array axis of i, j, k
    bx = 0.5 * _clamped(az, Y) / dy - 0.5 * _clamped(ay, Z) / dz                # :285
    by = 0.5 * _clamped(ax, Z) / dz - 0.5 * _clamped(az, X) / dx                # :286
    bz = 0.5 * _clamped(ay, X) / dx - 0.5 * _clamped(ax, Y) / dy                # :287
    fb = np.stack([bx.reshape(-1), by.reshape(-1), bz.reshape(-1)], axis=1).astype(np.float32)
    return dict(A=fa, eddy=fe, source=fs, B=fb)
