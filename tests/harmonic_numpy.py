"""Numpy restatement of the time-harmonic A-V solve (csrc/ec3d_harmonic.hip, k_build_table_harmonic of
csrc/ec3d_assemble.hip), bit for bit.

    classes(geoPHYS, geoPHYS_C)        per row of the reference numbering [Ax | Ay | Az | U]: its class, and the ids
    tables(valPHYS, BND, delta, ids)   re[ncls, 16] -- the transient table without its dt terms -- and m[ncls, 16], the
                                       unit imaginary table, from the material values and the grid alone
    entries(...)                       (row, col, slot, class) of every table slot of every row, in the order the row
                                       kernel adds them (ascending column)
    Operator                           the complex CSR in reference numbering and its ordered row product: a term is
                                       (ar xr - ai xi, ar xi + ai xr), every product and sum rounded on its own, a row
                                       adds from +0.0, a term whose two coefficients are 0 is left out
    cmul, cdiv, cdot_terms             the scalar arithmetic of the kernels
    DeviceSums                         the fixed-order sums on vectors in device numbering (thread t owns rows t and
                                       t + 256 of a chunk) through tests/device_sums_numpy.py
    bicgstab                           src/solvers.f90:3-50 in that arithmetic: expected to equal ec3d_harmonic_solve
                                       bit for bit (X^, iter, restarts)
    load_part                          ec3d_harmonic_load's X and B
    source_phasor                      host.run_harmonic's 64-point Fourier coefficient of a source function

No test lives here (the name does not start with test_)."""
from __future__ import annotations

import numpy as np

import device_sums_numpy as DS

A0 = 27


def ids_of(ndom_c):
    u0 = A0 + 9 * ndom_c
    return dict(a0=A0, u0=u0, zero=u0 + 27, ncls=u0 + 28)


def classes(geoPHYS, geoPHYS_C):
    """(cls[n_ref], ids, cond_dom_of): the class of every row; the conducting domains in scan order of their first cell."""
    geo = np.asarray(geoPHYS).astype(np.int64)
    gc = np.asarray(geoPHYS_C).astype(np.int64)
    sdz, sdy, sdx = geo.shape
    nC = geo.size
    cond = gc.reshape(-1) != 0
    doms = []
    for d in geo.reshape(-1)[cond]:
        if not doms or d != doms[-1]:
            assert d not in doms, "a conducting domain resumes: not the structured form"
            doms.append(int(d))
    ids = ids_of(max(len(doms), 1))
    k, j, i = np.meshgrid(np.arange(sdz), np.arange(sdy), np.arange(sdx), indexing="ij")
    t = lambda a, n: np.where(a == 0, 0, np.where(a == n - 1, 2, 1))
    bt = (t(i, sdx) + 3 * t(j, sdy) + 9 * t(k, sdz)).reshape(-1)
    cflat = np.pad(gc, 2).astype(np.int64)     # two zero cells around: a conductor never touches the box
    core = lambda dk, dj, di: cflat[2 + dk:2 + dk + sdz, 2 + dj:2 + dj + sdy, 2 + di:2 + di + sdx].reshape(-1) != 0
    shift = [(0, 0, 1), (0, 1, 0), (1, 0, 0)]
    cls = np.empty(3 * nC + int(cond.sum()), np.int64)
    ordinal = np.zeros(nC, np.int64)
    for o, d in enumerate(doms):
        ordinal[geo.reshape(-1) == d] = o
    pu = np.zeros(nC, np.int64)
    for d in range(3):
        sk, sj, si = shift[d]
        um, up = core(-sk, -sj, -si), core(sk, sj, si)
        pat = np.where(~up, 2, np.where(~um, 3, 1))
        cls[d * nC:(d + 1) * nC] = np.where(cond, ids["a0"] + 9 * ordinal + 3 * d + pat - 1, bt)
        st = np.where(~um, 1, np.where(~up, 2, 0))
        pu += st * 3 ** d
    cls[3 * nC:] = ids["u0"] + pu[cond]
    return cls, ids, doms or [1]


def tables(valPHYS, BND, delta, ids, cond_dom_of, shape=None):
    """(re, m), [ncls, 16] each.  Slots 0..6: the bands -z, -y, -x, diagonal, +x, +y, +z; A rows 7..11: U(cell + m step_d),
    m = -2..2; U rows 7 + 3 d + j: A_d(cell + (j - 1) step_d)."""
    vp = np.asarray(valPHYS, np.float64)
    BND = np.asarray(BND, np.float64)
    delta = np.asarray(delta, np.float64)
    s = 1.0 / (delta * delta)
    ds = 0.5 / delta
    re = np.zeros((ids["ncls"], 16))
    m = np.zeros((ids["ncls"], 16))

    def bands(tt):
        lo, hi, dg = np.zeros(3), np.zeros(3), np.zeros(3)
        for d in range(3):
            if tt[d] == 0:
                lo[d], hi[d], dg[d] = 0.0, BND[d, 1] * s[d], 1.0
            elif tt[d] == 2:
                lo[d], hi[d], dg[d] = BND[d, 0] * s[d], 0.0, 1.0
            else:
                lo[d], hi[d], dg[d] = -s[d], -s[d], 2.0
        on_box = any(x != 1 for x in tt)
        diag = (dg[0] * s[0] + dg[1] * s[1]) + dg[2] * s[2] if on_box else 2.0 * ((s[0] + s[1]) + s[2])
        return np.array([lo[2], lo[1], lo[0], diag, hi[0], hi[1], hi[2]])

    for q in range(27):
        re[q, :7] = bands((q % 3, (q // 3) % 3, q // 9))
    for q in range(ids["a0"], ids["u0"]):
        e = q - A0
        pat, d, dom = e % 3 + 1, (e // 3) % 3, cond_dom_of[e // 9]
        c = bands((1, 1, 1))
        C = vp[dom - 1, 1]
        for dd in range(3):
            h = vp[dom - 1, 2 + dd] / (2.0 * delta[dd])
            c[2 - dd] = c[2 - dd] - h
            c[4 + dd] = c[4 + dd] + h
        re[q, :7] = c
        m[q, 3] = C
        u = {1: {+1: -C * ds[d], -1: +C * ds[d]},
             2: {0: -3.0 * C * ds[d], -1: +4.0 * C * ds[d], -2: -1.0 * C * ds[d]},
             3: {0: +3.0 * C * ds[d], +1: -4.0 * C * ds[d], +2: +1.0 * C * ds[d]}}[pat]
        for mm, v in u.items():
            re[q, 7 + mm + 2] = v
    for q in range(ids["u0"], ids["zero"]):
        p = q - ids["u0"]
        st = (p % 3, (p // 3) % 3, p // 9)
        nmiss = sum(x != 0 for x in st)
        quirk = st == (1, 2, 2)
        for d in range(3):
            if st[d] == 0:
                re[q, 2 - d], re[q, 4 + d] = -s[d], -s[d]
            elif st[d] == 1:
                re[q, 2 - d], re[q, 4 + d] = 0.0, -2.0 * s[d]
            else:
                re[q, 2 - d], re[q, 4 + d] = -2.0 * s[d], 0.0
            if nmiss == 0:
                m[q, 7 + 3 * d + 0] = 0.5 * (1.0 / delta[d])
                m[q, 7 + 3 * d + 2] = 0.5 * (-1.0 / delta[d])
            elif st[d] != 0:
                av = 2.0 / delta[d]
                neg = st[d] == 1
                if quirk and d < 2:
                    neg = not neg
                m[q, 7 + 3 * d + 1] = -av if neg else av
        re[q, 3] = 2.0 * ((s[0] + s[1]) + s[2])
    return re, m


def entries(geoPHYS_C, cls, ids):
    """(row, col, slot), reference numbering, 0-based: every slot of every row's class, whether its coefficients are zero
    or not, in the order the row kernel visits them; slots that point outside the box or at a cell without U are left out."""
    gc = np.asarray(geoPHYS_C).astype(np.int64)
    sdz, sdy, sdx = gc.shape
    nC = gc.size
    flat = gc.reshape(-1)
    cond = np.flatnonzero(flat != 0)
    u_of = np.full(nC, -1, np.int64)
    u_of[cond] = 3 * nC + np.arange(len(cond))
    step = [1, sdx, sdx * sdy]
    off = [-step[2], -step[1], -1, 0, 1, step[1], step[2]]
    cell = np.arange(nC)
    ii, jj, kk = cell % sdx, (cell // sdx) % sdy, cell // (sdx * sdy)
    pos, sd = [ii, jj, kk], [sdx, sdy, sdz]

    def inside(q, d, mstep):
        return (pos[d][q] + mstep >= 0) & (pos[d][q] + mstep < sd[d])

    axis_of_band = [2, 1, 0, 0, 0, 1, 2]
    sign_of_band = [-1, -1, -1, 0, 1, 1, 1]
    rows, cols, slots, order = [], [], [], []
    for d in range(3):          # A rows: bands, then the U couplings
        for b in range(7):
            ok = inside(cell, axis_of_band[b], sign_of_band[b])
            rows.append(d * nC + cell[ok]); cols.append(d * nC + cell[ok] + off[b])
            slots.append(np.full(ok.sum(), b)); order.append(np.full(ok.sum(), b))
        c = cond
        for mm in range(-2, 3):
            ok = inside(c, d, mm)
            tgt = np.where(ok, u_of[np.clip(c + mm * step[d], 0, nC - 1)], -1)
            ok &= tgt >= 0
            rows.append(d * nC + c[ok]); cols.append(tgt[ok])
            slots.append(np.full(ok.sum(), 7 + mm + 2)); order.append(np.full(ok.sum(), 7 + mm + 2))
    c = cond                    # U rows: the A couplings, then the bands
    urow = u_of[c]
    for d in range(3):
        for j in range(3):
            ok = inside(c, d, j - 1)
            rows.append(urow[ok]); cols.append(d * nC + c[ok] + (j - 1) * step[d])
            slots.append(np.full(ok.sum(), 7 + 3 * d + j)); order.append(np.full(ok.sum(), 3 * d + j))
    for b in range(7):
        ok = inside(c, axis_of_band[b], sign_of_band[b])
        tgt = np.where(ok, u_of[np.clip(c + off[b], 0, nC - 1)], -1)
        ok &= tgt >= 0
        rows.append(urow[ok]); cols.append(tgt[ok])
        slots.append(np.full(ok.sum(), b)); order.append(np.full(ok.sum(), 9 + b))
    row, col, slot, order = (np.concatenate(a) for a in (rows, cols, slots, order))
    o = np.lexsort((order, row))
    return row[o], col[o], slot[o]


def cmul(a, b):
    """a b on (re, im) pairs of float64 (arrays or scalars)."""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def cdiv(a, b):
    with np.errstate(all="ignore"):
        d = b[0] * b[0] + b[1] * b[1]
        return (a[0] * b[0] + a[1] * b[1]) / d, (a[1] * b[0] - a[0] * b[1]) / d


def cdot_terms(a, b):
    """row terms of <a, b> = sum conj(a) b"""
    return a[0] * b[0] + a[1] * b[1], a[0] * b[1] - a[1] * b[0]


def split(z):
    z = np.asarray(z, np.complex128)
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


class Operator:
    """K + j omega M of a fixture in the reference numbering."""

    def __init__(self, g, omega):
        self.cls, self.ids, self.doms = classes(g["geoPHYS"], g["geoPHYS_C"])
        self.re_t, self.m_t = tables(g["valPHYS"], g["BND"], g["delta"], self.ids, self.doms)
        self.omega = float(omega)
        self.im_t = self.omega * self.m_t                      # one rounding per entry
        self.n = len(self.cls)
        row, col, slot = entries(g["geoPHYS_C"], self.cls, self.ids)
        self.row, self.col, self.slot = row, col, slot
        self.re, self.im = self.re_t[self.cls[row], slot], self.im_t[self.cls[row], slot]
        keep = (self.re != 0.0) | (self.im != 0.0)
        r, c, a, b = row[keep], col[keep], self.re[keep], self.im[keep]
        start = np.searchsorted(r, np.arange(self.n))
        k = np.arange(len(r)) - start[r]
        self.steps = [(r[k == q], c[k == q], a[k == q], b[k == q]) for q in range(int(k.max()) + 1)]
        self.nC = np.asarray(g["geoPHYS_C"]).size

    def __call__(self, x):
        """x: (re, im) -> (re, im), the ordered row product"""
        yr, yi = np.zeros(self.n), np.zeros(self.n)
        with np.errstate(invalid="ignore", over="ignore"):
            for r, c, a, b in self.steps:
                pr, pi = cmul((a, b), (x[0][c], x[1][c]))
                yr[r] = yr[r] + pr
                yi[r] = yi[r] + pi
        return yr, yi

    def dense(self):
        A = np.zeros((self.n, self.n), np.complex128)
        A[self.row, self.col] = self.re + 1j * self.im
        return A


class DeviceSums:
    """Sums over vectors of the reference numbering as the device adds them: scattered to device rows (row_map), zero
    elsewhere up to n_pad, thread t of a chunk adding row t, then row t + 256."""

    def __init__(self, row_map, n_pad, wgs=DS.WGS):
        self.rm, self.n_pad, self.wgs = np.asarray(row_map, np.int64), int(n_pad), wgs

    def __call__(self, terms):
        d = np.zeros(self.n_pad)
        d[self.rm] = terms
        t = d.reshape(-1, 2, DS.THREADS).transpose(0, 2, 1)
        return DS.strided(DS.stream_partials(t, self.wgs))


def bicgstab(op, sums, b, x0, tol, itmax, trace=None):
    """(x, iter, restarts, relres, kind): x, b as (re, im) pairs of float64 arrays; kind 1: the ||S|| exit, 2: the ||R||
    exit, 0: none.  trace (a list): (iteration, x, restarts)
    behind every iteration that took no exit -- what a solve with itmax = iteration - 1 returns."""
    sub = lambda a, c: (a[0] - c[0], a[1] - c[1])
    add = lambda a, c: (a[0] + c[0], a[1] + c[1])
    norm2 = lambda a: sums(a[0] * a[0] + a[1] * a[1])
    dot = lambda a, c: tuple(sums(t) for t in cdot_terms(a, c))
    with np.errstate(all="ignore"):
        x = (np.array(x0[0], np.float64), np.array(x0[1], np.float64))
        r = sub(b, op(x))
        r0, p = r, r
        bnorm = np.sqrt(norm2(b))
        rr = norm2(r)
        if bnorm == 0.0:
            return x, 0, 0, 0.0, 0
        rr0 = (rr, 0.0)
        restarts = 0
        rnorm = np.sqrt(rr)
        for it in range(1, itmax + 2):
            ap = op(p)
            alpha = cdiv(rr0, dot(r0, ap))
            s = sub(r, cmul(alpha, ap))
            snorm = np.sqrt(norm2(s))
            if snorm / bnorm < tol:
                return add(x, cmul(alpha, p)), it, restarts, snorm / bnorm, 1
            as_ = op(s)
            d2, d3 = dot(as_, s), norm2(as_)
            omega = cdiv(d2, (d3, 0.0))
            x = add(add(x, cmul(alpha, p)), cmul(omega, s))
            r = sub(s, cmul(omega, as_))
            rr = norm2(r)
            rr0n = dot(r0, r)
            rnorm = np.sqrt(rr)
            if rnorm / bnorm < tol:
                return x, it, restarts, rnorm / bnorm, 2
            beta = cdiv(cmul(cdiv(alpha, omega), rr0n), rr0)
            if np.sqrt(rr0n[0] * rr0n[0] + rr0n[1] * rr0n[1]) / bnorm < tol:
                r0, p, rr0 = r, r, (rr, 0.0)
                restarts += 1
            else:
                p = add(r, cmul(beta, sub(p, cmul(omega, ap))))
                rr0 = rr0n
            if trace is not None:
                trace.append((it, x, restarts))
        return x, max(itmax + 1, 0), restarts, rnorm / bnorm, 0


def load_part(op, g, cel_bnd, x, b, part):
    """(X, B) of ec3d_harmonic_load.  cel_bnd: the handle's six lists (1-based unknown ids); the first three are zeroed."""
    X = np.array(x[part], np.float64)
    B = np.array(b[part], np.float64)
    nC = op.nC
    cond = np.flatnonzero(np.asarray(g["geoPHYS_C"]).reshape(-1) != 0)
    for d in range(3):
        q = d * nC + cond
        w = op.im_t[op.cls[q], 3]
        B[q] = w * x[0][q] if part else -(w * x[1][q])
    for lst in cel_bnd[:3]:
        idx = np.asarray(lst, np.int64) - 1
        X[idx] = 0.0
        B[idx] = 0.0
    return X, B


def source_phasor(f, freq, nsamp=64):
    """(2 / N) sum f(T_n) exp(-j omega T_n), T_n = n / (N freq): the phasor a of a source a cos(omega t + phi)"""
    T = np.arange(nsamp) / (nsamp * float(freq))
    v = np.array([f(t) for t in T], np.float64)
    return (2.0 / nsamp) * np.sum(v * np.exp(-2j * np.pi * float(freq) * T))
