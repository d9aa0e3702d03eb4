"""numpy twin of ec3d_set_guess_history (csrc/ec3d_guess.hip): the projection onto earlier solutions in front of a solve
and the update of the stored pairs behind it, every sum in the device's order.

    dot_device(a, b)     a . b over vectors of n_pad doubles as k_guess_dots + k_guess_collapse add it
    History(depth, spmv, solve, to_dev)
        spmv(v) -> A v, solve(b, x0) -> (x, iter, hist_s, hist_r, ...) in the caller's numbering; to_dev(v) -> the vector in
        the handle's device numbering, zero padded to n_pad (the dot products are summed there: oracle.device_system)
    History.step(b, x)   one solve: returns what solve returned, with x replaced; History.info holds what
                         ec3d_get_guess_history reports (used, kept, stored, coef, res_before, res_after)
    for_handle(oracle, solver, valA, irow, jcol, depth, tol, itmax, hist_cap)   the twin of a device handle
    for_system(oracle, valA, irow, jcol, depth, tol, itmax)                    on the CPU, with oracle.bicgstab_wr

No test lives here (the name does not start with test_)."""
import numpy as np

from device_sums_numpy import THREADS, TILE, WGS, stream_dot as dot_device  # noqa: F401  (k_guess_dots + k_guess_collapse)

MIN_NEW = 1e-6                          # EC3D_GUESS_MIN_NEW
MAX_DEPTH = 8


class History:
    def __init__(self, depth, spmv, solve, to_dev):
        assert 0 <= depth <= MAX_DEPTH
        self.depth, self.spmv, self.solve, self.to_dev = depth, spmv, solve, to_dev
        self.q, self.aq = [], []                # oldest first
        self.info = dict(depth=depth, stored=0, used=0, kept=0, res_before=0.0, res_after=0.0, coef=np.zeros(0))

    def dot(self, a, b):
        return dot_device(self.to_dev(a), self.to_dev(b))

    def clear(self):
        self.q, self.aq = [], []

    def step(self, b, x):
        if self.depth == 0:
            return self.solve(b, x)
        k = len(self.q)
        x_start = np.array(x, dtype=np.float64)
        x = x_start.copy()
        zero_b = not np.any(b * b)              # B.B = 0, as the device's sum of squares has it
        coef = np.zeros(k)
        finite = True
        res_before = None
        if k:
            r = b - self.spmv(x)
            coef = np.array([self.dot(aq, r) for aq in self.aq])
            rr = self.dot(r, r)
            finite = bool(np.all(np.isfinite(coef)) and np.isfinite(rr))
            if zero_b:
                coef[:] = 0.0
            elif finite:
                for c, q in zip(coef, self.q):  # in this order, every term a rounded product and a rounded sum
                    x = x + c * q
            with np.errstate(all="ignore"):
                res_before = np.sqrt(rr) / np.sqrt(self.dot(b, b))
        with np.errstate(all="ignore"):
            res_after = np.sqrt(self.dot(b - self.spmv(x), b - self.spmv(x))) / np.sqrt(self.dot(b, b))
        out = self.solve(b, x)
        x = out[0]
        kept = 0
        if not zero_b:
            s = x - x_start
            a_s = self.spmv(s)
            n0 = n1 = None
            for p in range(2 if k else 1):
                h = [self.dot(aq, a_s) for aq in self.aq]
                if p == 0:
                    n0 = n1 = self.dot(a_s, a_s)
                finite = finite and bool(np.all(np.isfinite(h)) and np.isfinite(n0))
                if k and finite:
                    for hi, q, aq in zip(h, self.q, self.aq):
                        a_s = a_s - hi * aq
                        s = s - hi * q
                    n1 = self.dot(a_s, a_s)
            finite = finite and bool(np.isfinite(n0) and np.isfinite(n1))
            if finite and np.sqrt(n1) > MIN_NEW * np.sqrt(n0):
                inv = 1.0 / np.sqrt(n1)
                if k == self.depth:
                    self.q.pop(0)
                    self.aq.pop(0)
                self.q.append(s * inv)
                self.aq.append(a_s * inv)
                kept = 1
        if not finite:
            self.clear()
            kept = -1
        self.info = dict(depth=self.depth, stored=len(self.q), used=k, kept=kept, coef=coef,
                         res_before=res_after if res_before is None else float(res_before), res_after=float(res_after))
        return (x,) + tuple(out[1:])


def for_handle(oracle, solver, valA, irow, jcol, depth, tol, itmax, hist_cap=0, solve=None):
    """The twin of `solver` (an EC3DSolver holding this CSR system): sums in its device numbering, the solve by
    oracle.twin_solve unless `solve(b, x0)` is given (a preconditioned iteration's twin)."""
    rm = solver.row_map().astype(np.int64)
    n_pad = int(solver.geometry(0).n_pad)

    def to_dev(v):
        d = np.zeros(n_pad)
        d[rm] = v
        return d
    if solve is None:
        def solve(b, x0):
            return oracle.twin_solve(solver, valA, irow, jcol, b, x0, tol, itmax, hist_cap=hist_cap)
    return History(depth, lambda v: oracle.spmv_csr(valA, irow, jcol, v), solve, to_dev)


def for_system(oracle, valA, irow, jcol, depth, tol, itmax):
    """The algorithm alone, on the CPU: the reference's iteration (oracle.bicgstab_wr), rows in their own order."""
    n = len(irow) - 1
    n_pad = (n + TILE - 1) // TILE * TILE

    def to_dev(v):
        d = np.zeros(n_pad)
        d[:n] = v
        return d
    return History(depth, lambda v: oracle.spmv_csr(valA, irow, jcol, v),
                   lambda b, x0: oracle.bicgstab_wr(valA, irow, jcol, b, x0, tol, itmax), to_dev)
