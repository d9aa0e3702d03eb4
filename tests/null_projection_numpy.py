"""Numpy restatement of the left-null-vector projection of the A-V system (csrc/ec3d_transpose.hip, csrc/ec3d_null.hip;
DESIGN.md section 16).

The system's CSR comes in the reference's numbering ([Ax | Ay | Az | U], 1-based irow / jcol as the fixtures hold it).

  Ordered     a sparse product whose rows add their terms one by one from +0.0, every product and every sum rounded on
              its own, stored zeros left out.  Ordered.of_csr is y = A x with a row's terms in ascending column (the
              reference's order); Ordered.of_csr_t is y = A^T x with the terms of row j -- the entries of column j of
              A -- in ascending SOURCE row, which is ec3d_spmv_t's order: expected to equal the device bit for bit.
  components  connected components of the conducting cells (6-neighbourhood) in scan order of their first cell, each
              a list of cells in scan order; seed_rows: the U row of every component's middle cell.
  csr_transpose
              A^T as a CSR of its own, for a fast product (oracle.spmv_csr) inside the Krylov iterations.
  bicgstab    the reference's iteration (src/solvers.f90:3-50: the ||S|| and ||R|| exits, the restart rule) with an
              optional projection of the initial residual.  Plain numpy dot products: the device's Krylov iterates
              differ from these through the summation order, so nothing here is a bit-for-bit claim.
  left_null_vectors
              per component: A^T y = -A^T e_m from y = 0 to null_tol, w = y + e_m; then Gram-Schmidt in component
              order, a vector that keeps less than MIN_KEEP of its norm being dropped.
  project     v - Q (Q^T v), all coefficients taken first, then subtracted in component order.
  project_device
              the same on vectors in device numbering with every sum in the device's order (k_null_dots, k_null_collapse,
              k_null_sub through tests/device_sums_numpy.py): expected to equal ec3d_null_project bit for bit.

No test lives here (the name does not start with test_)."""
from __future__ import annotations

import numpy as np

from device_sums_numpy import THREADS, TILE, stream_dot, stream_partials

MIN_KEEP = 1e-6          # EC3D_NULL_MIN_KEEP of include/ec3d_hip.h
DEFAULT_NULL_TOL = 1e-10


class Ordered:
    """y[row] = sum of val * x[src] over the row's terms in their stored order, from +0.0."""

    def __init__(self, n, row, src, val):
        # row ascending, the terms of a row in the order they are added
        self.n = int(n)
        start = np.searchsorted(row, np.arange(self.n))
        k = np.arange(len(row)) - start[row]
        self.steps = []
        for q in range(int(k.max()) + 1 if len(k) else 0):
            m = k == q
            self.steps.append((row[m], src[m], val[m]))

    @classmethod
    def of_csr(cls, valA, irow, jcol):
        n = len(irow) - 1
        row = np.repeat(np.arange(n), np.diff(irow.astype(np.int64)))
        keep = valA != 0.0
        return cls(n, row[keep], jcol[keep].astype(np.int64) - 1, valA[keep])

    @classmethod
    def of_csr_t(cls, valA, irow, jcol):
        n = len(irow) - 1
        row = np.repeat(np.arange(n), np.diff(irow.astype(np.int64)))
        keep = valA != 0.0
        row, col, val = row[keep], jcol[keep].astype(np.int64) - 1, valA[keep]
        o = np.lexsort((row, col))          # by column, then by source row
        return cls(n, col[o], row[o], val[o])

    def __call__(self, x):
        y = np.zeros(self.n)
        for row, src, val in self.steps:
            y[row] = y[row] + val * x[src]
        return y

    def abs_sum(self, x):
        """sum of |terms| per row: the scale of the rounding error of any summation order"""
        y = np.zeros(self.n)
        for row, src, val in self.steps:
            y[row] = y[row] + np.abs(val * x[src])
        return y


def csr_transpose(valA, irow, jcol):
    """(valT, irowT, jcolT): the 1-based CSR of A^T, a row's entries in ascending column (= ascending source row of A)."""
    n = len(irow) - 1
    row = np.repeat(np.arange(n), np.diff(irow.astype(np.int64)))
    col = jcol.astype(np.int64) - 1
    o = np.lexsort((row, col))
    irowT = np.concatenate(([0], np.cumsum(np.bincount(col, minlength=n)))) + 1
    return np.ascontiguousarray(valA[o]), irowT.astype(np.int32), (row[o] + 1).astype(np.int32)


def components(geoPHYS_C):
    """[(cells in scan order)] of the connected conducting components, in scan order of their first cell."""
    cond = np.asarray(geoPHYS_C) > 0
    sdz, sdy, sdx = cond.shape
    label = np.full(cond.shape, -1, np.int64)
    out = []
    for q in np.flatnonzero(cond.reshape(-1)):
        k, j, i = np.unravel_index(q, cond.shape)
        if label[k, j, i] >= 0:
            continue
        c = len(out)
        label[k, j, i] = c
        stack, cells = [(k, j, i)], []
        while stack:
            k, j, i = stack.pop()
            cells.append((k * sdy + j) * sdx + i)
            for dk, dj, di in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
                a, b, e = k + dk, j + dj, i + di
                if 0 <= a < sdz and 0 <= b < sdy and 0 <= e < sdx and cond[a, b, e] and label[a, b, e] < 0:
                    label[a, b, e] = c
                    stack.append((a, b, e))
        out.append(np.sort(np.array(cells, np.int64)))
    return out


def seed_rows(geoPHYS_C):
    """0-based row, in the reference's numbering, of the U unknown on every component's middle cell (scan order)."""
    g = np.asarray(geoPHYS_C)
    nC = g.size
    cond = np.flatnonzero(g.reshape(-1) > 0)            # U unknown m lives on cell cond[m]
    return [3 * nC + int(np.searchsorted(cond, cells[len(cells) // 2])) for cells in components(g)]


def project(Q, v):
    if not len(Q):
        return v, np.zeros(0)
    c = np.array([q @ v for q in Q])
    for ci, q in zip(c, Q):
        v = v - ci * q
    return v, c


def project_device(Q_dev, r_dev, n, launched=None):
    """(r, c, rr_part): ec3d_null_project on vectors in device numbering, zero padded to n_pad (oracle.device_system).
    c_i = stream_dot(Q_i, r), all taken first; r = r - c_i Q_i in component order, every term a rounded product and a
    rounded difference; rr_part: the per-workgroup partials of r.r as k_null_sub leaves them -- one per workgroup of its
    launch (`launched`: the residual launch's count, where that is not the streaming launch's own).  Rows >= n enter
    every sum as +0.0 and come back as they went in."""
    r = np.array(r_dev, np.float64)
    assert len(r) % TILE == 0 and all(len(q) == len(r) for q in Q_dev)
    live = np.arange(len(r)) < n
    c = np.array([stream_dot(np.where(live, q, 0.0), np.where(live, r, 0.0)) for q in Q_dev])
    x = np.where(live, r, 0.0)
    for ci, q in zip(c, Q_dev):
        x = x - ci * np.where(live, q, 0.0)
    r[:n] = x[:n]
    return r, c, stream_partials((x * x).reshape(-1, THREADS, 2), launched=launched)


def bicgstab(op, b, x0, tol, itmax, Q=None):
    """(x, iter, removed): iter as the library returns it (itmax + 1: no exit); Q: the initial residual is projected."""
    x = np.array(x0, np.float64)
    r = b - op(x)
    removed = 0.0
    bnorm = np.sqrt(b @ b)
    if bnorm == 0.0:
        return x, 0, removed
    if Q is not None and len(Q):
        r, c = project(Q, r)
        removed = float(np.sqrt(c @ c) / bnorm)
    r0, p = r.copy(), r.copy()
    rr0 = r @ r0
    for it in range(1, itmax + 2):
        ap = op(p)
        alpha = rr0 / (ap @ r0)
        s = r - alpha * ap
        if np.sqrt(s @ s) / bnorm < tol:
            return x + alpha * p, it, removed
        as_ = op(s)
        omega = (as_ @ s) / (as_ @ as_)
        x = x + alpha * p + omega * s
        r = s - omega * as_
        rr = r @ r
        if np.sqrt(rr) / bnorm < tol:
            return x, it, removed
        rr0_new = r @ r0
        beta = (alpha / omega) * rr0_new / rr0
        if abs(rr0_new) / bnorm < tol:
            r0, p, rr0 = r.copy(), r.copy(), rr
        else:
            p = r + beta * (p - omega * ap)
            rr0 = rr0_new
    return x, itmax + 1, removed


def adjoint_cap(n):
    return int(20.0 * n ** (1.0 / 3.0)) + 2000


def left_null_vectors(At, n, seeds, null_tol=DEFAULT_NULL_TOL):
    """(Q, info): Q the orthonormal left null vectors kept; info per component dict(seed, iterations, residual, kept,
    reached) with residual = ||A^T w|| / ||w|| of the vector before the orthogonalisation.  At: any callable x -> A^T x."""
    Q, info = [], []
    cap = adjoint_cap(n)
    for m in seeds:
        e = np.zeros(n)
        e[m] = 1.0
        c = -At(e)
        y, it, _ = bicgstab(At, c, np.zeros(n), null_tol, cap)
        w = y + e
        n0 = np.sqrt(w @ w)
        rec = dict(seed=int(m), iterations=int(it), residual=float(np.linalg.norm(At(w)) / n0), kept=False,
                   reached=it <= cap)
        w, _ = project(Q, w)
        n1 = np.sqrt(w @ w)
        if n1 > MIN_KEEP * n0:
            Q.append(w / n1)
            rec["kept"] = True
        info.append(rec)
    return Q, info


_SETUPS = {}


def setup_for(oracle, name, g):
    """dict(A, At, Q, info, seeds) of fixture `name` (g: its arrays), computed once per process: A and At are fast
    products through oracle.spmv_csr, Q and info come from left_null_vectors at the default null_tol."""
    if name not in _SETUPS:
        valA, irow, jcol = g["valA"], g["irow"], g["jcol"]
        T = csr_transpose(valA, irow, jcol)
        A = lambda v: oracle.spmv_csr(valA, irow, jcol, v)
        At = lambda v: oracle.spmv_csr(T[0], T[1], T[2], v)
        seeds = seed_rows(g["geoPHYS_C"])
        Q, info = left_null_vectors(At, len(irow) - 1, seeds)
        _SETUPS[name] = dict(A=A, At=At, Q=Q, info=info, seeds=seeds)
    return _SETUPS[name]
