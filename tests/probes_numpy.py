"""float64 numpy twin of ec3d_probe_sample (include/ec3d_hip.h; csrc/ec3d_probes.hip): the four point vectors of
field_N.vtk at chosen cells WITHOUT their rounding to float32 -- the expressions of tests/fields_numpy.py, in the same
order -- and the cells' scalar potential.

x, b in the reference's numbering [Ax | Ay | Az | U] (what EC3DSolver.download returns); geoPHYS_C[k, j, i] holds the
1-based number of a conductor cell's U unknown in that numbering (0 outside the conductors), so u = x[geoPHYS_C - 1].
"""
from __future__ import annotations

import numpy as np

from fields_numpy import EDDY_SCALE, _clamped


def whole_box(geoPHYS_C, delta, x, b):
    """(ncells, 13) float64: a, eddy, source, b, u of every cell in scan order."""
    gc = np.asarray(geoPHYS_C)
    shape = gc.shape
    N = gc.size
    x, b = np.asarray(x, np.float64), np.asarray(b, np.float64)
    uid = gc.reshape(-1).astype(np.int64)
    cond = uid != 0
    U = [x[c * N:(c + 1) * N] for c in range(3)]
    J = [b[c * N:(c + 1) * N] for c in range(3)]
    out = np.zeros((N, 13), np.float64)
    for c in range(3):
        out[:, c] = U[c]
        out[:, 3 + c] = np.where(cond, EDDY_SCALE * J[c], 0.0)
        out[:, 6 + c] = np.where(cond, 0.0, J[c])
    ax, ay, az = (u.reshape(shape) for u in U)
    dx, dy, dz = (float(d) for d in delta)
    X, Y, Z = 2, 1, 0                                                           # array axis of i, j, k
    out[:, 9] = (0.5 * _clamped(az, Y) / dy - 0.5 * _clamped(ay, Z) / dz).reshape(-1)
    out[:, 10] = (0.5 * _clamped(ax, Z) / dz - 0.5 * _clamped(az, X) / dx).reshape(-1)
    out[:, 11] = (0.5 * _clamped(ay, X) / dx - 0.5 * _clamped(ax, Y) / dy).reshape(-1)
    out[cond, 12] = x[uid[cond] - 1]
    return out


def sample(geoPHYS_C, delta, x, b, cells):
    """(nprobes, 13) float64 at the 0-based cell numbers i + j*sdx + k*sdx*sdy, in the caller's order."""
    return np.ascontiguousarray(whole_box(geoPHYS_C, delta, x, b)[np.asarray(cells, np.int64)])
