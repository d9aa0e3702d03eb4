"""Numpy restatement of the left null vectors of the time-harmonic operator and their projection (k_hb_spmv_h, the
set-up and the k_hbn_* kernels of csrc/ec3d_harmonic.hip), bit for bit.

    OperatorH            y = A^H x, A = K + j omega M of harmonic_numpy.Operator: row j adds the entries of column j of
                         A in ascending SOURCE row from +0.0, a term conj(a) x = (ar xr + ai xi, ar xi - ai xr), every
                         product and sum rounded on its own; stored zeros (both coefficients 0) are left out.  Takes and
                         returns (re, im) pairs like Operator, so harmonic_numpy.bicgstab runs on it as it stands.
    adjoint_cap(n)       20 n^(1/3) + 2000, the iteration cap of an adjoint solve
    left_null_vectors    per seed row m: c = A^H (-e_m), the solve A^H y = c from y = 0 to null_tol
                         (harmonic_numpy.bicgstab), w = y + e_m, ||A^H w|| / ||w||, classical Gram-Schmidt against the
                         vectors kept (all <Q_i, w> first, then the subtractions in order), each part divided by
                         sqrt(sum(re^2 + im^2)); a vector that keeps less than MIN_KEEP of its norm is dropped.
    project_device       the three launches in front of a projected solve, on vectors in device numbering
    bicgstab_projected   harmonic_numpy.bicgstab with the projected initial residual
    projected_residual   ||P (b - A x)|| / ||b|| and removed = sqrt(sum |c_i|^2) / ||b||

No test lives here (the name does not start with test_)."""
from __future__ import annotations

import numpy as np

import device_sums_numpy as DS
import harmonic_numpy as HN

MIN_KEEP = 1e-6          # EC3D_NULL_MIN_KEEP of include/ec3d_hip.h
DEFAULT_NULL_TOL = 1e-10


def cmul_conj(a, b):
    """conj(a) b on (re, im) pairs"""
    return a[0] * b[0] + a[1] * b[1], a[0] * b[1] - a[1] * b[0]


class OperatorH:
    """(K + j omega M)^H of an harmonic_numpy.Operator, the reference numbering."""

    def __init__(self, op):
        self.n, self.nC = op.n, op.nC
        keep = (op.re != 0.0) | (op.im != 0.0)
        src, dst, a, b = op.row[keep], op.col[keep], op.re[keep], op.im[keep]
        o = np.lexsort((src, dst))                              # by column of A, then by source row
        src, dst, a, b = src[o], dst[o], a[o], b[o]
        start = np.searchsorted(dst, np.arange(self.n))
        k = np.arange(len(dst)) - start[dst]
        self.steps = [(dst[k == q], src[k == q], a[k == q], b[k == q]) for q in range(int(k.max()) + 1)]

    def __call__(self, x):
        yr, yi = np.zeros(self.n), np.zeros(self.n)
        with np.errstate(invalid="ignore", over="ignore"):
            for r, c, a, b in self.steps:
                pr, pi = cmul_conj((a, b), (x[0][c], x[1][c]))
                yr[r] = yr[r] + pr
                yi[r] = yi[r] + pi
        return yr, yi

    def abs_sum(self, x):
        """sum of |a| |x| per row: the scale of the rounding error of any summation order"""
        y = np.zeros(self.n)
        for r, c, a, b in self.steps:
            y[r] = y[r] + np.hypot(a, b) * np.hypot(x[0][c], x[1][c])
        return y


def adjoint_cap(n):
    return int(20.0 * np.cbrt(float(n))) + 2000


def _norm2(sums, a):
    return sums(a[0] * a[0] + a[1] * a[1])


def _dot(sums, a, b):
    return tuple(sums(t) for t in HN.cdot_terms(a, b))


def left_null_vectors(op, opH, sums, seeds, null_tol=DEFAULT_NULL_TOL):
    """(Q, info): Q the kept vectors as (re, im) pairs; info per seed dict(seed, iterations, restarts, residual, kept,
    reached).  A seed whose solve took no exit within the cap, or whose true residual ||A^H w|| exceeds
    2 null_tol ||c||, ends the set-up as the device's does: reached = False in the last record and no Q (None)."""
    n = op.n
    cap = adjoint_cap(n)
    zero = (np.zeros(n), np.zeros(n))
    Q, info = [], []
    with np.errstate(all="ignore"):
        for m in seeds:
            neg = np.zeros(n)
            neg[m] = -1.0
            c = opH((neg, np.zeros(n)))
            y, it, restarts, _, kind = HN.bicgstab(opH, sums, c, zero, null_tol, cap)
            w = (np.array(y[0]), np.array(y[1]))
            w[0][m] = w[0][m] + 1.0
            true = np.sqrt(_norm2(sums, opH(w)))            # c - A^H y = -A^H w: the adjoint system's true residual
            n0 = np.sqrt(_norm2(sums, w))
            reached = kind != 0 and bool(true / np.sqrt(_norm2(sums, c)) <= 2.0 * null_tol)
            rec = dict(seed=int(m), iterations=int(it), restarts=int(restarts), residual=float(true / n0), kept=False,
                       reached=reached)
            info.append(rec)
            if not reached:
                return None, info
            n1 = n0
            if Q:
                coef = [_dot(sums, q, w) for q in Q]
                for ci, q in zip(coef, Q):
                    t = HN.cmul(ci, q)
                    w = (w[0] - t[0], w[1] - t[1])
                n1 = np.sqrt(_norm2(sums, w))
            if np.isfinite(n0) and np.isfinite(n1) and n1 > MIN_KEEP * n0:
                Q.append((w[0] / n1, w[1] / n1))
                rec["kept"] = True
    return Q, info


def _device_terms(v):
    """[n_pad] per-row terms in device numbering -> [nchunk, 256, 2]: thread t owns rows t and t + 256 of a chunk"""
    return v.reshape(-1, 2, DS.THREADS).transpose(0, 2, 1)


def project_device(Q_dev, r_dev, n, launched=None):
    """(r, c, rr_part): the projection's launches on complex vectors in device numbering, n_pad pairs each.
    c_i = <Q_i, r> (fixed-order sums of the row terms' two parts), all taken first; r = r - c_i Q_i in component order,
    every term a rounded cmul and a rounded difference per part; rr_part: the per-workgroup partials of ||r||^2 that
    the subtraction leaves in the HP_RR slot, one per workgroup of the launch (`launched`: where that is not the
    streaming launch's own count).  Rows >= n enter every sum as +0.0 and come back as they went in."""
    r = np.array(r_dev, np.complex128)
    assert len(r) % DS.TILE == 0 and all(len(q) == len(r) for q in Q_dev)
    live = np.arange(len(r)) < n
    part = lambda z: (np.where(live, z.real, 0.0), np.where(live, z.imag, 0.0))
    x = part(r)
    with np.errstate(all="ignore"):
        Qp = [part(np.asarray(q, np.complex128)) for q in Q_dev]
        c = [tuple(DS.strided(DS.stream_partials(_device_terms(t))) for t in HN.cdot_terms(q, x)) for q in Qp]
        for ci, q in zip(c, Qp):
            t = HN.cmul(ci, q)
            x = (x[0] - t[0], x[1] - t[1])
        rr = DS.stream_partials(_device_terms(x[0] * x[0] + x[1] * x[1]), launched=launched)
    r.real[:n], r.imag[:n] = x[0][:n], x[1][:n]
    return r, np.array([complex(a, b) for a, b in c]), rr


def _project(sums, Q, r):
    coef = [_dot(sums, q, r) for q in Q]
    for ci, q in zip(coef, Q):
        t = HN.cmul(ci, q)
        r = (r[0] - t[0], r[1] - t[1])
    return r, coef


def removed_of(coef, bnorm):
    s = 0.0
    for cr, ci in coef:
        s += cr * cr + ci * ci
    return float(np.sqrt(s) / bnorm)


def bicgstab_projected(op, sums, Q, b, x0, tol, itmax, trace=None):
    """(x, iter, restarts, relres, kind, removed): harmonic_numpy.bicgstab -- restated line for line, because its
    initial residual is not a parameter -- from R = (b - A x0) - sum c_i Q_i, c_i = <Q_i, b - A x0>; ||b||, the exits
    and the restart rule as they are.  trace as there."""
    sub = lambda a, c: (a[0] - c[0], a[1] - c[1])
    add = lambda a, c: (a[0] + c[0], a[1] + c[1])
    norm2 = lambda a: _norm2(sums, a)
    dot = lambda a, c: _dot(sums, a, c)
    cmul, cdiv = HN.cmul, HN.cdiv
    with np.errstate(all="ignore"):
        x = (np.array(x0[0], np.float64), np.array(x0[1], np.float64))
        r, coef = _project(sums, Q, sub(b, op(x)))
        r0, p = r, r
        bnorm = np.sqrt(norm2(b))
        rr = norm2(r)
        if bnorm == 0.0:
            return x, 0, 0, 0.0, 0, 0.0
        removed = removed_of(coef, bnorm)
        rr0 = (rr, 0.0)
        restarts = 0
        rnorm = np.sqrt(rr)
        for it in range(1, itmax + 2):
            ap = op(p)
            alpha = cdiv(rr0, dot(r0, ap))
            s = sub(r, cmul(alpha, ap))
            snorm = np.sqrt(norm2(s))
            if snorm / bnorm < tol:
                return add(x, cmul(alpha, p)), it, restarts, snorm / bnorm, 1, removed
            as_ = op(s)
            d2, d3 = dot(as_, s), norm2(as_)
            omega = cdiv(d2, (d3, 0.0))
            x = add(add(x, cmul(alpha, p)), cmul(omega, s))
            r = sub(s, cmul(omega, as_))
            rr = norm2(r)
            rr0n = dot(r0, r)
            rnorm = np.sqrt(rr)
            if rnorm / bnorm < tol:
                return x, it, restarts, rnorm / bnorm, 2, removed
            beta = cdiv(cmul(cdiv(alpha, omega), rr0n), rr0)
            if np.sqrt(rr0n[0] * rr0n[0] + rr0n[1] * rr0n[1]) / bnorm < tol:
                r0, p, rr0 = r, r, (rr, 0.0)
                restarts += 1
            else:
                p = add(r, cmul(beta, sub(p, cmul(omega, ap))))
                rr0 = rr0n
            if trace is not None:
                trace.append((it, x, restarts))
        return x, max(itmax + 1, 0), restarts, rnorm / bnorm, 0, removed


def projected_residual(op, sums, Q, b, x):
    """(||P (b - A x)|| / ||b||, removed)"""
    with np.errstate(all="ignore"):
        y = op(x)
        r, coef = _project(sums, Q, (b[0] - y[0], b[1] - y[1]))
        bnorm = np.sqrt(_norm2(sums, b))
        return float(np.sqrt(_norm2(sums, r)) / bnorm), removed_of(coef, bnorm)
