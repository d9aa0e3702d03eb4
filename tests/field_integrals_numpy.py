"""numpy twin of ec3d_field_energy and ec3d_domain_linkage (include/ec3d_hip.h; csrc/ec3d_integrals.hip): every per-cell
term in float64 one operation at a time, every sum in the device's order, so the results are the library's bit for bit.

Per cell, from the J and B of tests/fields_numpy.py before their rounding to float32:

    B = curl A (central differences clamped at the box faces),  J = s * Jaf in every cell
    a = (Ax*Jx + Ay*Jy) + Az*Jz

    cell_terms(geoPHYS_C, delta, x, b)   dict(b2 [N, 3], a [N], j [N, 3], cond [N]) in scan order
    stream_sum(v, shape)                 a per-cell array summed as the streaming pass adds it
    list_sum(v)                          a domain's entries summed as k_dom_partials + k_dom_final add them
    field_energy(...)                    what EC3DSolver.field_energy returns
    domain_linkage(...)                  what EC3DSolver.domain_linkage returns
    clamped_energy(shape, delta, B0)     closed form of energy_b for A = (-B0 y/2, B0 x/2, 0)

Uaf = x, Jaf = b in the reference's numbering [Ax | Ay | Az | U]; arrays [k, j, i].  No test lives here."""
from __future__ import annotations

import numpy as np

from device_sums_numpy import THREADS, TILE, WGS, block_sum, stream_partials, strided  # noqa: F401  (re-exported)
from fields_numpy import EDDY_SCALE, _clamped

DOM_CHUNK = 1024                                       # EC3D_DOM_CHUNK
INV_MU0 = 0.07957747154594766788444e7                  # the literal behind s = -1 / mu0


def curl(delta, x, shape):
    """(bx, by, bz), each [k, j, i]: Vector_field_B before its rounding."""
    N = int(np.prod(shape))
    ax, ay, az = (np.asarray(x[c * N:(c + 1) * N], np.float64).reshape(shape) for c in range(3))
    dx, dy, dz = (float(d) for d in delta)
    X, Y, Z = 2, 1, 0
    bx = 0.5 * _clamped(az, Y) / dy - 0.5 * _clamped(ay, Z) / dz
    by = 0.5 * _clamped(ax, Z) / dz - 0.5 * _clamped(az, X) / dx
    bz = 0.5 * _clamped(ay, X) / dx - 0.5 * _clamped(ax, Y) / dy
    return bx, by, bz


def cell_terms(geoPHYS_C, delta, x, b):
    gc = np.asarray(geoPHYS_C)
    N = gc.size
    bx, by, bz = (v.reshape(-1) for v in curl(delta, x, gc.shape))
    A = [np.asarray(x[c * N:(c + 1) * N], np.float64) for c in range(3)]
    J = [EDDY_SCALE * np.asarray(b[c * N:(c + 1) * N], np.float64) for c in range(3)]
    a = (A[0] * J[0] + A[1] * J[1]) + A[2] * J[2]
    return dict(b2=np.stack([bx * bx, by * by, bz * bz], axis=1), a=a, j=np.stack(J, axis=1),
                cond=gc.reshape(-1) != 0)


def stream_sum(v, shape):
    """k_field_energy + k_energy_collapse: every xy plane cut into ceil(sdx*sdy / 512) chunks (cells past the plane's end
    add +0.0), workgroup w of G = min(chunks, 1024) takes chunks w, w + G, ..., thread t cell 2t, then cell 2t + 1."""
    sdz, kdz = shape[0], shape[1] * shape[2]
    cpp = -(-kdz // TILE)
    p = np.zeros((sdz, cpp * TILE))
    p[:, :kdz] = np.asarray(v, np.float64).reshape(sdz, kdz)
    return strided(stream_partials(p.reshape(sdz * cpp, THREADS, 2)))


def list_sum(v):
    """k_dom_partials + k_dom_final over one domain's entries in scan order: chunks of 1024, thread t of a chunk adds its
    entries t, t + 256, t + 512, t + 768; thread t of the domain's workgroup the chunk sums t, t + 256, ..."""
    v = np.asarray(v, np.float64)
    nch = -(-len(v) // DOM_CHUNK)
    p = np.zeros(nch * DOM_CHUNK)
    p[:len(v)] = v
    p = p.reshape(nch, 4, THREADS)
    with np.errstate(invalid="ignore"):
        acc = np.zeros((nch, THREADS))
        for e in range(4):
            acc = acc + p[:, e, :]
        return strided(block_sum(acc))


def field_energy(geoPHYS_C, delta, x, b, terms=None):
    gc = np.asarray(geoPHYS_C)
    t = cell_terms(gc, delta, x, b) if terms is None else terms
    dx, dy, dz = (float(d) for d in delta)
    vol = dx * dy * dz
    half = vol * (0.5 * INV_MU0)
    s = [stream_sum(t["b2"][:, c], gc.shape) for c in range(3)]
    src = stream_sum(np.where(t["cond"], 0.0, t["a"]), gc.shape)
    eddy = stream_sum(np.where(t["cond"], t["a"], 0.0), gc.shape)
    return dict(cells=int(gc.size), energy_b=half * ((s[0] + s[1]) + s[2]), energy_axis=np.array([half * v for v in s]),
                aj_source=vol * src, aj_eddy=vol * eddy)


def domain_linkage(geoPHYS, geoPHYS_C, delta, x, b, terms=None):
    g = np.asarray(geoPHYS).reshape(-1).astype(np.int64)
    t = cell_terms(geoPHYS_C, delta, x, b) if terms is None else terms
    dx, dy, dz = (float(d) for d in delta)
    vol = dx * dy * dz
    out = []
    for d in sorted(set(g[~t["cond"]].tolist())):
        sel = np.flatnonzero((g == d) & ~t["cond"])                      # scan order
        out.append(dict(domain=int(d), cells=int(len(sel)), linkage=vol * list_sum(t["a"][sel]),
                        jsum=np.array([vol * list_sum(t["j"][sel, c]) for c in range(3)])))
    return out


def linkage_lists(geoPHYS, geoPHYS_C):
    """[(domain id, cells)] of the non-conducting domains, ascending id: what the library's host loop must find."""
    g = np.asarray(geoPHYS).reshape(-1).astype(np.int64)
    n = np.bincount(g[np.asarray(geoPHYS_C).reshape(-1) == 0])
    return [(int(d), int(c)) for d, c in enumerate(n) if c]


def vector_potential(shape, delta, B0):
    """x = [Ax | Ay | Az] of A = (-B0 y/2, B0 x/2, 0) at the cell centres (i + 1/2) dx, (j + 1/2) dy."""
    sdz, sdy, sdx = shape
    dx, dy, _ = (float(d) for d in delta)
    xs = (np.arange(sdx) + 0.5) * dx
    ys = (np.arange(sdy) + 0.5) * dy
    ax = np.broadcast_to((-B0 * ys / 2)[None, :, None], shape)
    ay = np.broadcast_to((B0 * xs / 2)[None, None, :], shape)
    return np.concatenate([ax.reshape(-1), ay.reshape(-1), np.zeros(int(np.prod(shape)))])


def clamped_energy(shape, delta, B0):
    """energy_b of vector_potential in real arithmetic.  Bz = 0.5 dAy/di / dx - 0.5 dAx/dj / dy, each half B0/2 where the
    difference spans two cells and B0/4 where it is clamped to one (the faces i = 1, sdx and j = 1, sdy); Bx = By = 0:
    (sdx - 2)(sdy - 2) columns of B0, 2 (sdx - 2) + 2 (sdy - 2) edge columns of 3 B0 / 4 and 4 corner columns of B0 / 2."""
    sdz, sdy, sdx = shape
    dx, dy, dz = (float(d) for d in delta)
    cols = (sdx - 2) * (sdy - 2) + (2 * (sdx - 2) + 2 * (sdy - 2)) * 9 / 16 + 4 / 4
    return dx * dy * dz * 0.5 * INV_MU0 * B0 * B0 * cols * sdz
