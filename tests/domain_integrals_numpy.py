"""float64 numpy twin of ec3d_domain_integrals (include/ec3d_hip.h): Joule loss and Lorentz force per conducting domain.

The per-cell terms are the expressions of the header, evaluated in float64 one operation at a time (numpy contracts
nothing), from the very J and B of tests/fields_numpy.py before their rounding to float32:

    J = s * Jaf on the conductor cells,  B = curl A (central differences clamped at the box faces)
    q = Jx*Jx + Jy*Jy + Jz*Jz,  f = J x B

Each domain's terms are summed with math.fsum (the correctly rounded sum: no order to agree on), and the scaling is the
library's: sigma = C_d * 0.07957747154594766788444e7, joule_w = (dx*dy*dz) * sum(q) / sigma, force_n = (dx*dy*dz) *
sum(f).  Uaf = x, Jaf = b in the reference's numbering [Ax | Ay | Az | U]; arrays [k, j, i].
"""
from __future__ import annotations

import math

import numpy as np

from fields_numpy import EDDY_SCALE, _clamped

SIGMA_SCALE = 0.07957747154594766788444e7      # 1 / mu0: valPHYS(:, 2) is mu0 * sigma


def cell_terms(geoPHYS_C, delta, x, b):
    """(cells, terms): the flat indices of the conductor cells in scan order and their float64 terms [len(cells), 4] =
    (q, fx, fy, fz)."""
    gc = np.asarray(geoPHYS_C)
    shape, N = gc.shape, gc.size
    cells = np.flatnonzero(gc.reshape(-1) != 0)
    ax, ay, az = (np.asarray(x[c * N:(c + 1) * N], np.float64).reshape(shape) for c in range(3))
    dx, dy, dz = (float(d) for d in delta)
    X, Y, Z = 2, 1, 0                                                           # array axis of i, j, k
    bx = (0.5 * _clamped(az, Y) / dy - 0.5 * _clamped(ay, Z) / dz).reshape(-1)[cells]
    by = (0.5 * _clamped(ax, Z) / dz - 0.5 * _clamped(az, X) / dx).reshape(-1)[cells]
    bz = (0.5 * _clamped(ay, X) / dx - 0.5 * _clamped(ax, Y) / dy).reshape(-1)[cells]
    jx, jy, jz = (EDDY_SCALE * np.asarray(b[c * N:(c + 1) * N], np.float64)[cells] for c in range(3))
    q = jx * jx + jy * jy + jz * jz
    fx = jy * bz - jz * by
    fy = jz * bx - jx * bz
    fz = jx * by - jy * bx
    return cells, np.stack([q, fx, fy, fz], axis=1)


def sums_by_domain(geoPHYS, cells, terms):
    """[(domain id, cells, fsum of the four terms, fsum of their magnitudes)] in ascending id order."""
    dom = np.asarray(geoPHYS).reshape(-1)[cells].astype(np.int64)
    out = []
    for d in sorted(set(dom.tolist())):
        t = terms[dom == d]
        out.append((d, len(t), np.array([math.fsum(t[:, c].tolist()) for c in range(4)]),
                    np.array([math.fsum(np.abs(t[:, c]).tolist()) for c in range(4)])))
    return out


def scaled(valPHYS, delta, d, n, s, a):
    """One record of EC3DSolver.domain_integrals from a domain's four sums s; ``abs``: the same scaling applied to the
    sums of magnitudes a (joule, fx, fy, fz) -- what a bound on the summation error is stated in."""
    dx, dy, dz = (float(v) for v in delta)
    vol = dx * dy * dz
    sigma = float(np.asarray(valPHYS, np.float64)[d - 1, 1]) * SIGMA_SCALE
    return dict(domain=int(d), cells=int(n), sigma=sigma, joule_w=vol * s[0] / sigma, force_n=vol * s[1:4],
                abs=np.array([vol * a[0] / sigma, vol * a[1], vol * a[2], vol * a[3]]))


def integrals(geoPHYS, geoPHYS_C, valPHYS, delta, x, b):
    """The list EC3DSolver.domain_integrals returns, every record with one more key ``abs`` (see scaled)."""
    cells, terms = cell_terms(geoPHYS_C, delta, x, b)
    return [scaled(valPHYS, delta, d, n, s, a) for d, n, s, a in sums_by_domain(geoPHYS, cells, terms)]
