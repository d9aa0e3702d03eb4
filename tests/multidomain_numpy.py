"""numpy restatement of the reference's time-step vectors for models with several conducting domains.

The reference (src/EC3D.f90:277-433) loops over the conducting domains m = 1..size_PHYS_C, and within each over
n = 1..siznod(m):  A rows of the domain's n-th cell get a*Uaf + Jaf (a = 2C/dt of that domain), and the U row
3*nCells + n gets s = (row 3*nCells + n's A part) . Uaf.  So only the U rows n <= max_m siznod(m) receive their s
(rule "reference"); every later U row keeps 0.  Rule "all" gives every U row its s.  Sums run sequentially over the
row's stored (ascending) entries, as the reference's loop does.

Also the condition under which ec3d_assemble keeps the structured form: U ids (geoPHYS_C) in scan order, at most 22
conducting domains.
"""
from __future__ import annotations

import numpy as np

MAXDOM = 22   # EC3D_SAV_MAXDOM


def conductors(geoPHYS, geoPHYS_C):
    """[(domain id, cells in scan order)] in the order of their U ids (domain-major, src/vxc2data.f90:624-650)."""
    geo = np.asarray(geoPHYS).reshape(-1).astype(np.int64)
    gc = np.asarray(geoPHYS_C).reshape(-1).astype(np.int64)
    cond = np.flatnonzero(gc)
    by_id = cond[np.argsort(gc[cond], kind="stable")]
    out = []
    for q in by_id:
        d = int(geo[q])
        if not out or out[-1][0] != d:
            out.append((d, []))
        out[-1][1].append(int(q))
    return [(d, np.array(sorted(c), np.int64)) for d, c in out]


def structured_applies(geoPHYS, geoPHYS_C):
    """ec3d_assemble's structured form: the domain-major U ids equal scan order, and D <= MAXDOM."""
    gc = np.asarray(geoPHYS_C).reshape(-1).astype(np.int64)
    ids = gc[gc != 0]
    ncells = gc.size
    return bool(np.array_equal(ids, 3 * ncells + 1 + np.arange(ids.size))
                and len(conductors(geoPHYS, geoPHYS_C)) <= MAXDOM)


def cel_bnd(vox_shape, geoPHYS_C):
    """cel_bndX/Y/Z (0-based A ids) and cel_bndUx/y/z (0-based U ids, i.e. geoPHYS_C - 1): conducting cells with a
    non-conducting neighbour along that axis (src/EC3D.f90:758-760, :938-940)."""
    gc = np.asarray(geoPHYS_C).reshape(vox_shape).astype(np.int64)
    N = gc.size
    on = gc != 0
    A, U = [], []
    for d, ax in enumerate((2, 1, 0)):   # x, y, z = the last, middle, first array axis
        lo = np.roll(on, 1, axis=ax)
        hi = np.roll(on, -1, axis=ax)
        edge = on & ~(lo & hi)
        q = np.flatnonzero(edge.reshape(-1))
        A.append(d * N + q)
        U.append(gc.reshape(-1)[q] - 1)
    return A, U


def post_update(geoPHYS, geoPHYS_C, valPHYS, dt, vox_shape, b, x):
    """src/EC3D.f90:412-433 on copies: (Jaf, Uaf) after the solve."""
    b, x = b.copy(), x.copy()
    N = int(np.prod(vox_shape))
    nsub = valPHYS.shape[0]
    vp = np.asarray(valPHYS).reshape(-1, order="F")
    for d, cells in conductors(geoPHYS, geoPHYS_C):
        a = 2.0 * vp[1 * nsub + d - 1] / dt
        for c in range(3):
            q = c * N + cells
            b[q] = a * x[q] - b[q]
    A, _ = cel_bnd(vox_shape, geoPHYS_C)
    for lst in A:
        b[lst] = 0.0
        x[lst] = 0.0
    return b, x


def rhs_step(irow, jcol, valA, geoPHYS, geoPHYS_C, valPHYS, dt, vox_shape, b, x, src_idx, src_val, moving,
             rule="reference"):
    """src/EC3D.f90:277-404 on a copy of Jaf (b) given Uaf (x): the next right-hand side.  src_idx 1-based."""
    b = b.copy()
    N = int(np.prod(vox_shape))
    nsub = valPHYS.shape[0]
    vp = np.asarray(valPHYS).reshape(-1, order="F")
    doms = conductors(geoPHYS, geoPHYS_C)
    if moving:                                          # :277-296 keep the inertial part of the A rows
        keep = np.concatenate([c * N + cells for _, cells in doms for c in range(3)]) if doms else np.zeros(0, int)
        saved = b[keep].copy()
        b[:] = 0.0
        b[keep] = saved
    for i, v in zip(np.asarray(src_idx, np.int64), np.asarray(src_val, np.float64)):   # :298-367, in order
        b[i - 1] = v
    if not doms:
        return b
    nU = sum(len(c) for _, c in doms)
    nu = nU if rule == "all" else max(len(c) for _, c in doms)
    for d, cells in doms:                               # :370-393
        a = 2.0 * vp[1 * nsub + d - 1] / dt
        for c in range(3):
            q = c * N + cells
            b[q] = a * x[q] + b[q]
    for n in range(nu):                                 # U row 3N + n (0-based n), its A columns, stored order
        r = 3 * N + n
        s = 0.0
        for e in range(irow[r] - 1, irow[r + 1] - 1):
            k = jcol[e] - 1
            if k < 3 * N:
                s = s + valA[e] * x[k]
        b[r] = s
    A, U = cel_bnd(vox_shape, geoPHYS_C)                # :396-402 (U ids index Jaf as they are)
    for lst in U + A:
        b[lst] = 0.0
    return b


def blocks_model(D):
    """D separated 4x4x4 conducting blocks stacked along z, 2 planes apart (so the U ids are in scan order), materials
    alternating between two conductivities, a one-plane coil loop above the stack: (vox [sdz, sdy, sdx], palette
    names) of a 5-step transient, for vxc.VxcModel(vox, names, 0.004, (1, 1, 1)).  With 3x3x3 blocks, whose cells are
    all but one on a face, BiCGSTAB stalls after the first step; these converge on every step (D = 22 and 23)."""
    sdx, sdy, sdz = 10, 10, 6 * D + 6
    vox = np.zeros((sdz, sdy, sdx), np.uint8)
    for m in range(D):
        vox[2 + 6 * m:6 + 6 * m, 3:7, 3:7] = m + 1
    c, z = D + 1, sdz - 3                               # +x, -x, +y, -y sides of the loop (oracle.put_coil's order)
    vox[z, 1, 2:8] = c
    vox[z, 8, 2:8] = c + 1
    vox[z, 1:9, 8] = c + 2
    vox[z, 1:9, 1] = c + 3
    names = [f"m{m + 1} D=1 C='mu0*{35.26e6 if m % 2 == 0 else 58e6:.6g}'" for m in range(D)]
    names += ["axp D=1 SRCx=Fp", "axm D=1 SRCx=Fm", "ayp D=1 SRCy=Fp", "aym D=1 SRCy=Fm",
              "param tran stop=5m step=1m", "p2 solver tol=1m itmax=10000 dir=blk",
              "f1 func Fp=a*cos(p2*f*t) a='183/(dx*2*dz)' p2='2*pi' f=50 t=t",
              "f2 func Fm=a*cos(p2*f*t) a='-183/(dx*2*dz)' p2='2*pi' f=50 t=t"]
    return vox, names
