"""Numpy restatement of the geometric multigrid preconditioner (eddy_currents_3d_amd/csrc/ec3d_mg.hip).

Levels are oracle.poisson_csr operators of the level's grid and spacing (a rediscretisation: the device reruns the
assembly of ec3d_assemble_poisson), stored as the seven band coefficients in offset order (-z, -y, -x, diag, +x, +y,
+z).  Every elementwise operation is written in the kernels' order, so precond_apply on the device is expected to be
bit-identical to MG.apply() here (no reduction enters a V-cycle):

  GS update of a cell       t = b; t = t - c_q * x[nb_q] for q = -z, -y, -x, +x, +y, +z (0 where no neighbour); x = t / c_diag
  residual of a cell        t = b; t = t - c_q * x[nb_q] for q = -z, -y, -x, diag, +x, +y, +z
  restriction               sum of the children's residuals, k outermost, i innermost, from 0.0; times 1 / children
  prolongation              x_fine = w_fine + x_coarse[parent] (piecewise-constant injection)

Colour of cell (i, j, k) is (i + j + k) & 1 (0-based), red = 0.  One V-cycle from x = 0 on level l:
  pre   sweeps of (red, black), the first red half from x = 0 being x = b / d on red, 0 on black;
  b_{l+1} = mean of the children's b - A w; V-cycle on level l + 1;
  x = w + P x_{l+1}; post sweeps of (black, red);
  coarsest level: coarse_sweeps sweeps of (red, black, black, red) from x = 0.

`bnd` is what oracle.poisson_csr takes: a scalar for all six faces, or six values in the Fortran order of BND(3, 2),
BND(d, 1) for d = x, y, z and then BND(d, 2) (the operator uses BND(d, 2) on the first cell of axis d and BND(d, 1) on
the last; solver.assemble_poisson flattens a (3, 2) array column-major to that order).  Every level gets the same BND.

pbicgstab_gpuorder restates the outer iteration (ec3d_mg_launch_iteration) with the kernels' summation order, so a
device solve is expected to equal it bit for bit as well.
"""
from __future__ import annotations

import numpy as np

from device_sums_numpy import block_sum as _block_sums, strided as mg_scalar_sum   # the workgroup tree, k_mg_scalar's collapse

MAX_COARSE_ROWS = 4096
DEFAULT_PRE, DEFAULT_POST, DEFAULT_COARSE = 2, 2, 16


def hierarchy_dims(sdx, sdy, sdz, delta=(0.00333, 0.00333, 0.00333)):
    """Level dims and spacings: an axis halves while it is even and >= 8; stop when no axis can halve or the level
    has <= 4096 rows.  Returns (dims, deltas, ok) -- ok False when the coarsest level is over the coarse solver's cap."""
    dims = [(sdx, sdy, sdz)]
    deltas = [tuple(float(d) for d in delta)]
    while dims[-1][0] * dims[-1][1] * dims[-1][2] > MAX_COARSE_ROWS:
        d = dims[-1]
        half = [a % 2 == 0 and a >= 8 for a in d]
        if not any(half):
            break
        dims.append(tuple(a // 2 if h else a for a, h in zip(d, half)))
        deltas.append(tuple(2.0 * s if h else s for s, h in zip(deltas[-1], half)))
    last = dims[-1]
    return dims, deltas, last[0] * last[1] * last[2] <= MAX_COARSE_ROWS


def bands_of(sdx, sdy, sdz, delta, bnd=-0.95):
    """oracle.poisson_csr(sdx, sdy, sdz, delta, bnd) as a (7, n) array of band coefficients."""
    from oracle import oracle as O
    valA, irow, jcol = O.poisson_csr(sdx, sdy, sdz, delta, bnd)
    n = sdx * sdy * sdz
    rows = np.repeat(np.arange(n), np.diff(irow))
    off = (jcol - 1) - rows
    kdz = sdx * sdy
    q = np.select([off == -kdz, off == -sdx, off == -1, off == 0, off == 1, off == sdx, off == kdz],
                  [0, 1, 2, 3, 4, 5, 6], -1)
    assert (q >= 0).all()
    c = np.zeros((7, n))
    c[q, rows] = valA
    return c


class Level:
    def __init__(self, dims, delta, bnd=-0.95):  # bnd: scalar or six faces, as oracle.poisson_csr
        self.dims = dims
        self.sdx, self.sdy, self.sdz = dims
        self.n = self.sdx * self.sdy * self.sdz
        self.c = bands_of(self.sdx, self.sdy, self.sdz, delta, bnd)
        k, j, i = np.meshgrid(np.arange(self.sdz), np.arange(self.sdy), np.arange(self.sdx), indexing="ij")
        self.ijk = (i.reshape(-1), j.reshape(-1), k.reshape(-1))
        self.colour = ((i + j + k) & 1).reshape(-1)

    def neighbours(self, x):
        """x at the six neighbours (0 where there is none), in offset order -z, -y, -x, +x, +y, +z."""
        X = x.reshape(self.sdz, self.sdy, self.sdx)
        out = []
        for axis, sgn in ((0, -1), (1, -1), (2, -1), (2, 1), (1, 1), (0, 1)):
            Y = np.zeros_like(X)
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            if sgn < 0:
                dst[axis], src[axis] = slice(1, None), slice(None, -1)
            else:
                dst[axis], src[axis] = slice(None, -1), slice(1, None)
            Y[tuple(dst)] = X[tuple(src)]
            out.append(Y.reshape(-1))
        return out

    def half_sweep(self, x, b, colour):
        nb = self.neighbours(x)
        t = b.copy()
        for q, v in zip((0, 1, 2, 4, 5, 6), nb):
            t = t - self.c[q] * v
        m = self.colour == colour
        x = x.copy()
        x[m] = t[m] / self.c[3][m]
        return x

    def residual(self, x, b):
        nb = self.neighbours(x)
        t = b.copy()
        for q, v in zip((0, 1, 2), nb[:3]):
            t = t - self.c[q] * v
        t = t - self.c[3] * x
        for q, v in zip((4, 5, 6), nb[3:]):
            t = t - self.c[q] * v
        return t

    def spmv(self, x):
        """A x, rows summed in offset order from the -z term (the device's spmv_dot order)."""
        nb = self.neighbours(x)
        s = self.c[0] * nb[0]
        s = s + self.c[1] * nb[1]
        s = s + self.c[2] * nb[2]
        s = s + self.c[3] * x
        for q, v in zip((4, 5, 6), nb[3:]):
            s = s + self.c[q] * v
        return s


def restrict(fine, coarse, r):
    fx, fy, fz = (fine.sdx // coarse.sdx, fine.sdy // coarse.sdy, fine.sdz // coarse.sdz)
    R = r.reshape(fine.sdz, fine.sdy, fine.sdx)
    s = np.zeros((coarse.sdz, coarse.sdy, coarse.sdx))
    for dk in range(fz):
        for dj in range(fy):
            for di in range(fx):
                s = s + R[dk::fz, dj::fy, di::fx]
    return (s * (1.0 / (fx * fy * fz))).reshape(-1)


def prolong(fine, coarse, w, xc):
    fx, fy, fz = (fine.sdx // coarse.sdx, fine.sdy // coarse.sdy, fine.sdz // coarse.sdz)
    Xc = xc.reshape(coarse.sdz, coarse.sdy, coarse.sdx)
    P = np.repeat(np.repeat(np.repeat(Xc, fz, 0), fy, 1), fx, 2).reshape(-1)
    return w + P


class MG:
    def __init__(self, sdx, sdy, sdz, delta=(0.00333, 0.00333, 0.00333), bnd=-0.95, pre=0, post=0,
                 coarse_sweeps=0):
        dims, deltas, ok = hierarchy_dims(sdx, sdy, sdz, delta)
        if not ok:
            raise ValueError("coarsest level over the coarse solver's cap")
        self.levels = [Level(d, s, bnd) for d, s in zip(dims, deltas)]
        self.pre = pre or DEFAULT_PRE
        self.post = post or DEFAULT_POST
        self.coarse = coarse_sweeps or DEFAULT_COARSE

    def _cycle(self, l, b):
        L = self.levels[l]
        x = np.zeros(L.n)
        if l == len(self.levels) - 1:
            for _ in range(self.coarse):
                for col in (0, 1, 1, 0):
                    x = L.half_sweep(x, b, col)
            return x
        for _ in range(self.pre):
            x = L.half_sweep(x, b, 0)
            x = L.half_sweep(x, b, 1)
        C = self.levels[l + 1]
        bc = restrict(L, C, L.residual(x, b))
        xc = self._cycle(l + 1, bc)
        x = prolong(L, C, x, xc)
        for _ in range(self.post):
            x = L.half_sweep(x, b, 1)
            x = L.half_sweep(x, b, 0)
        return x

    def apply(self, r):
        return self._cycle(0, np.asarray(r, np.float64))

    def spmv(self, x):
        return self.levels[0].spmv(x)


def pbicgstab(mg, b, x0=None, tol=1e-8, itmax=200):
    """Right-preconditioned BiCGSTAB with the reference's restart rule (src/solvers.f90:24-50).  Returns (x, iter)."""
    A = mg.spmv
    x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
    r = b - A(x)
    r0 = r.copy()
    p = r.copy()
    bnorm = np.linalg.norm(b)
    it = 0
    if bnorm == 0.0:
        return x, 0
    rr0 = r @ r0
    while True:
        if it > itmax:
            return x, it
        it += 1
        ph = mg.apply(p)
        v = A(ph)
        alpha = rr0 / (r0 @ v)
        s = r - alpha * v
        if np.linalg.norm(s) / bnorm < tol:
            return x + alpha * ph, it
        sh = mg.apply(s)
        t = A(sh)
        omega = (t @ s) / (t @ t)
        x = x + alpha * ph + omega * sh
        r = s - omega * t
        if np.linalg.norm(r) / bnorm < tol:
            return x, it
        rr0_new = r @ r0
        beta = (alpha / omega) * rr0_new / rr0
        p = r + beta * (p - omega * v)
        rr0 = rr0_new
        if abs(rr0_new) / bnorm < tol:
            r0 = r.copy()
            p = r.copy()
            rr0 = r @ r0


# ---- GPU-order twin of the outer iteration ------------------------------------------------------------------------
MG_DOT_BLOCKS = 2048  # EC3D_MG_DOT_BLOCKS
EXIT_NONE, EXIT_S, EXIT_R = 0, 1, 2  # SolverState::stop_kind: 0 for the itmax exit and ||b|| = 0


def mg_partials(prod):
    """The per-workgroup partials of one reducing MG kernel (k_mg_spmv_dot, k_mg_s, k_mg_xr) over the row products
    `prod`: nb = min(2048, ceil(n / 256)) workgroups of 256 threads, thread t of workgroup k adding rows
    k*256 + t + m*nb*256 in increasing m from 0.0, then block_sum."""
    n = len(prod)
    nb = min(MG_DOT_BLOCKS, max(1, -(-n // 256)))
    T = nb * 256
    M = -(-n // T)
    P = np.zeros(M * T)
    P[:n] = prod
    P = P.reshape(M, T)
    acc = np.zeros(T)
    for m in range(M):
        acc = acc + P[m]
    return _block_sums(acc)


def mg_dot(a, b):
    """a.b as one MG reducing kernel and k_mg_scalar sum it (products a[r] * b[r])."""
    return mg_scalar_sum(mg_partials(a * b))


class Identity:
    """M = I on the operator of `level`: with it, pbicgstab_gpuorder is the reference's iteration."""

    def __init__(self, level):
        self.levels = [level]

    def apply(self, r):
        return np.array(r, np.float64, copy=True)


def pbicgstab_gpuorder(mg, b, x0, tol, itmax, setup_geom=None, hist_cap=0):
    """ec3d_mg_launch_iteration restated operation by operation, every sum in the kernels' order.

    Setup as the device's (the solve without a preconditioner's): R = b - A x0, R0 = P = R, ||b|| and R.R summed by
    the SpMV kernels' geometry setup_geom (oracle.geoms_of(solver)[1]; None: in the MG kernels' order, for a twin
    without a device).  The row sums of A x are Level.spmv's (oracle_spmv_csr's up to the sign of a zero).

    Returns (x, it, hist_s, hist_r, restarts, exit_kind): hist_* of length hist_cap, NaN where not reached;
    exit_kind EXIT_S (||S|| / ||b|| < tol: x += alpha p^ only), EXIT_R, or EXIT_NONE (itmax + 1 iterations ran, or
    ||b|| = 0: x returned unchanged with it = 0)."""
    A = mg.levels[0].spmv
    b = np.asarray(b, np.float64)
    x = np.array(x0, np.float64, copy=True)
    hs = np.full(hist_cap, np.nan)
    hr = np.full(hist_cap, np.nan)
    if setup_geom is None:
        sdot = mg_dot
    else:
        from oracle import oracle as O
        def sdot(u, v):
            return O.dot_gpuorder(setup_geom, u, v)
    R = b - A(x)
    R0 = R.copy()
    p = R.copy()
    bnorm = np.sqrt(sdot(b, b))                       # k_setup
    if bnorm == 0.0:
        return x, 0, hs, hr, 0, EXIT_NONE
    rr0 = sdot(R, R0)                                 # st->rr0[1]
    it = 0
    restarts = 0
    while True:
        if it > itmax:
            return x, it, hs, hr, restarts, EXIT_NONE
        it += 1
        ph = mg.apply(p)
        v = A(ph)                                     # k_mg_spmv_dot #1: R0.v
        alpha = rr0 / mg_dot(R0, v)                   # MG_ALPHA
        s = R - alpha * v                             # k_mg_s: S.S
        sn = np.sqrt(mg_dot(s, s))                    # MG_SEXIT
        if it - 1 < hist_cap:
            hs[it - 1] = sn
        if sn / bnorm < tol:
            x = x + alpha * ph                        # k_mg_xr, the ||S|| exit's branch
            return x, it, hs, hr, restarts, EXIT_S
        sh = mg.apply(s)
        t = A(sh)                                     # k_mg_spmv_dot #2: S.t, t.t
        omega = mg_dot(s, t) / mg_dot(t, t)           # MG_OMEGA
        x = x + alpha * ph + omega * sh               # k_mg_xr: R.R, R.R0
        R = s - omega * t
        rr = mg_dot(R, R)
        rr0_new = mg_dot(R, R0)
        rn = np.sqrt(rr)                              # MG_REXIT
        if it - 1 < hist_cap:
            hr[it - 1] = rn
        if rn / bnorm < tol:
            return x, it, hs, hr, restarts, EXIT_R
        beta = (alpha / omega) * rr0_new / rr0
        if abs(rr0_new) / bnorm < tol:                # k_mg_p: the restart R0 = R, P = R
            restarts += 1
            p = R.copy()
            R0 = R.copy()
            rr0 = rr                                  # R0 == R: the next rr0 is R.R
        else:
            p = R + beta * (p - omega * v)
            rr0 = rr0_new
