"""Numpy restatement of the block multigrid preconditioner of the structured A-V form (EC3D_PRECOND_BLOCK_MG,
eddy_currents_3d_amd/csrc/ec3d_mg.hip, k_avmg_*).

The four blocks' band coefficients come from the system's CSR in the reference's numbering ([Ax | Ay | Az | U], U
unknown m on cell ucell[m]): bands in offset order (-z, -y, -x, diag, +x, +y, +z); couplings between blocks are left
out of M.  The three A blocks must have the same bands (src/EC3D.f90: valY = valX, valZ = valX): one hierarchy serves
them.  Every operation is written in the kernels' order, so precond_apply on the device is expected to equal
AVMG.apply() bit for bit (the only sums in M, the U projection's, are restated in the kernels' order):

  levels      level 0 is the A block's operator; an axis whose extent is > 1 is ceil-halved (aggregates of 2 cells, the
              last one 1 cell on an odd axis) until a level has <= 4096 cells
  Galerkin    coarse band q = sum of the children's couplings that cross the aggregate's face on that side (to a cell
              inside the box); diagonal = children's diagonals plus their couplings inside the aggregate; children k
              outermost, i innermost, within a child the diagonal first and then the couplings in offset order from
              0.0; times 1 / (2 * nominal children)
  V-cycle     mg_numpy's (red-black GS, pre + post sweeps, first red half from zero, residual + mean restriction,
              piecewise-constant prolongation, coarse_sweeps of (red, black, black, red) on the coarsest level), with
              the mean over the aggregate's actual children and rows without a diagonal giving 0
  U block     the right-hand side projected onto the U block's range -- b - (w.b / w.1) on every conducting component,
              w the U rows' left null vector (1/2 per axis with a missing neighbour), the sums in k_avmg_upart /
              k_avmg_umean's fixed order -- then pre + post sweeps of (red, black) from zero on the U unknowns' 7-point
              rows (a neighbour without a U unknown is 0)

spmv is the full operator (oracle.spmv_csr), so mg_numpy.pbicgstab and mg_numpy.pbicgstab_gpuorder run the
preconditioned iteration with this M unchanged.
"""
from __future__ import annotations

import numpy as np

from mg_numpy import DEFAULT_COARSE, DEFAULT_POST, DEFAULT_PRE, MAX_COARSE_ROWS, _block_sums, mg_scalar_sum

UCHUNK = 4096  # EC3D_AVMG_UCHUNK

# offset order: axis of the (z, y, x)-shaped grid and direction of band q; q = 3 is the diagonal
_AX = (0, 1, 2, None, 2, 1, 0)
_DIR = (-1, -1, -1, 0, 1, 1, 1)


def level_dims(sdx, sdy, sdz):
    dims = [(sdx, sdy, sdz)]
    while dims[-1][0] * dims[-1][1] * dims[-1][2] > MAX_COARSE_ROWS:
        dims.append(tuple((a + 1) // 2 if a > 1 else a for a in dims[-1]))
    return dims


def _offsets(sdx, sdy):
    return (-sdx * sdy, -sdx, -1, 0, 1, sdx, sdx * sdy)


def _shift(X, axis, sgn):
    """X at the neighbour along `axis` in direction sgn (0 beyond the box)."""
    Y = np.zeros_like(X)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if sgn < 0:
        dst[axis], src[axis] = slice(1, None), slice(None, -1)
    else:
        dst[axis], src[axis] = slice(None, -1), slice(1, None)
    Y[tuple(dst)] = X[tuple(src)]
    return Y


class BandLevel:
    """A 7-point operator on a grid as seven (n,) band arrays; rows without a diagonal give 0."""

    def __init__(self, dims, c):
        self.dims = tuple(int(a) for a in dims)
        self.sdx, self.sdy, self.sdz = self.dims
        self.shape = (self.sdz, self.sdy, self.sdx)
        self.n = self.sdx * self.sdy * self.sdz
        self.c = np.asarray(c, np.float64)
        k, j, i = np.meshgrid(np.arange(self.sdz), np.arange(self.sdy), np.arange(self.sdx), indexing="ij")
        self.colour = ((i + j + k) & 1).reshape(-1)
        self.live = self.c[3] != 0.0

    def neighbours(self, x):
        X = x.reshape(self.shape)
        return [_shift(X, a, s).reshape(-1) for a, s in ((0, -1), (1, -1), (2, -1), (2, 1), (1, 1), (0, 1))]

    def half_sweep(self, x, b, colour, rows=None):
        """GS update of the rows of one colour (and of `rows`, when given) from the other colour's values."""
        nb = self.neighbours(x)
        t = b.copy()
        for q, v in zip((0, 1, 2, 4, 5, 6), nb):
            t = t - self.c[q] * v
        m = self.colour == colour
        if rows is not None:
            m = m & rows
        x = x.copy()
        live = m & self.live
        x[m & ~self.live] = 0.0
        x[live] = t[live] / self.c[3][live]
        return x

    def init_red(self, b, rows=None):
        """The first red half-sweep from x = 0: b / d on red, 0 elsewhere."""
        m = (self.colour == 0) & self.live
        if rows is not None:
            m = m & rows
        x = np.zeros(self.n)
        x[m] = b[m] / self.c[3][m]
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


def _children(fine, coarse):
    """(dk, dj, di, slices of the fine grid, slices of the coarse grid) for every child position that exists."""
    f = [2 if a > 1 else 1 for a in fine.shape]
    out = []
    for dk in range(f[0]):
        for dj in range(f[1]):
            for di in range(f[2]):
                d = (dk, dj, di)
                if any(d[a] >= fine.shape[a] for a in range(3)):
                    continue
                fs = tuple(slice(d[a], None, f[a]) for a in range(3))
                cs = tuple(slice(0, len(range(d[a], fine.shape[a], f[a]))) for a in range(3))
                out.append((d, fs, cs))
    return f, out


def galerkin(fine: BandLevel, dims) -> BandLevel:
    coarse_shape = (dims[2], dims[1], dims[0])
    f, kids = _children(fine, None)
    C = [fine.c[q].reshape(fine.shape) for q in range(7)]
    idx = np.meshgrid(np.arange(fine.sdz), np.arange(fine.sdy), np.arange(fine.sdx), indexing="ij")
    D = np.zeros(coarse_shape)
    B = [np.zeros(coarse_shape) for _ in range(7)]
    for d, fs, cs in kids:
        D[cs] = D[cs] + C[3][fs]
        for q in (0, 1, 2, 4, 5, 6):
            a = _AX[q]
            pos = idx[a][fs]
            nb = pos + _DIR[q]
            inbox = (nb >= 0) & (nb < fine.shape[a])
            inside = inbox & (nb // f[a] == pos // f[a])
            cross = inbox & ~inside
            cq = C[q][fs]
            D[cs] = np.where(inside, D[cs] + cq, D[cs])
            B[q][cs] = np.where(cross, B[q][cs] + cq, B[q][cs])
    scale = 1.0 / (2.0 * f[0] * f[1] * f[2])
    c = np.stack([(D if q == 3 else B[q]).reshape(-1) * scale for q in range(7)])
    return BandLevel(dims, c)


def restrict(fine, coarse, r):
    _, kids = _children(fine, coarse)
    R = r.reshape(fine.shape)
    s = np.zeros(coarse.shape)
    cnt = np.zeros(coarse.shape)
    for _, fs, cs in kids:
        s[cs] = s[cs] + R[fs]
        cnt[cs] += 1
    return (s * (1.0 / cnt)).reshape(-1)


def prolong(fine, coarse, w, xc):
    f = [2 if a > 1 else 1 for a in fine.shape]
    Xc = xc.reshape(coarse.shape)
    P = np.repeat(np.repeat(np.repeat(Xc, f[0], 0), f[1], 1), f[2], 2)[:fine.sdz, :fine.sdy, :fine.sdx].reshape(-1)
    x = w + P
    x[~fine.live] = 0.0
    return x


def bands_from_csr(valA, irow, jcol, dims, ucell):
    """(A-block bands (7, nC) -- checked equal over the three blocks --, U bands (7, nC) on the U cells' positions,
    0 elsewhere)."""
    sdx, sdy, sdz = dims
    nC = sdx * sdy * sdz
    irow = np.asarray(irow, np.int64)
    jcol = np.asarray(jcol, np.int64) - 1
    n = len(irow) - 1
    rows = np.repeat(np.arange(n), np.diff(irow))
    offs = _offsets(sdx, sdy)
    nu = len(ucell)
    uc = np.full(n, -1, np.int64)               # cell of every unknown's column, block-relative
    uc[:3 * nC] = np.tile(np.arange(nC), 3)
    uc[3 * nC:3 * nC + nu] = ucell
    blk = np.minimum(np.arange(n) // nC, 3)
    same = blk[rows] == blk[jcol]
    off = uc[jcol] - uc[rows]
    bands = []
    for d in range(4):
        c = np.zeros((7, nC))
        m = same & (blk[rows] == d)
        for q, o in enumerate(offs):
            e = m & (off == o)
            c[q, uc[rows[e]]] = valA[e]
        bands.append(c)
    for d in (1, 2):
        if not np.array_equal(bands[0], bands[d]):
            raise ValueError("the A blocks' band coefficients differ")
    return bands[0], bands[3]


def u_components(urows, dims):
    """Conducting components of the (nC,) mask of U cells (cells joined across a face; cell = (k * sdy + j) * sdx + i),
    each as its cells in scan order, the components in order of their first cell."""
    sdx, sdy, sdz = dims
    comp = np.full(len(urows), -1, np.int64)
    comps = []
    for c0 in np.flatnonzero(urows):
        if comp[c0] >= 0:
            continue
        comp[c0] = len(comps)
        stack, cells = [int(c0)], []
        while stack:
            q = stack.pop()
            cells.append(q)
            i, j, k = q % sdx, (q // sdx) % sdy, q // (sdx * sdy)
            for ok, nb in ((k > 0, q - sdx * sdy), (j > 0, q - sdx), (i > 0, q - 1), (i + 1 < sdx, q + 1),
                           (j + 1 < sdy, q + sdx), (k + 1 < sdz, q + sdx * sdy)):
                if ok and urows[nb] and comp[nb] < 0:
                    comp[nb] = comp[c0]
                    stack.append(nb)
        comps.append(np.sort(np.array(cells, np.int64)))
    return comps


def u_weights(cu):
    """Weights of the U rows' left null vector from the U bands (7, nC): 1/2 per axis along which the cell misses a
    neighbour (a band coefficient of that axis is 0)."""
    w = np.ones(cu.shape[1])
    for lo, hi in ((2, 4), (1, 5), (0, 6)):
        w = np.where((cu[lo] == 0.0) | (cu[hi] == 0.0), w * 0.5, w)
    return w


class AVMG:
    def __init__(self, valA, irow, jcol, dims, ucell, pre=0, post=0, coarse_sweeps=0):
        self.valA, self.irow, self.jcol = valA, irow, jcol
        self.dims = tuple(int(a) for a in dims)
        self.nC = int(np.prod(self.dims))
        self.ucell = np.asarray(ucell, np.int64)
        self.n = 3 * self.nC + len(self.ucell)
        ca, cu = bands_from_csr(valA, irow, jcol, self.dims, self.ucell)
        self.levels = [BandLevel(self.dims, ca)]
        for d in level_dims(*self.dims)[1:]:
            self.levels.append(galerkin(self.levels[-1], d))
        self.ulevel = BandLevel(self.dims, cu)
        self.urows = np.zeros(self.nC, bool)
        self.urows[self.ucell] = True
        self.ucomps = u_components(self.urows, self.dims)
        self.uweight = u_weights(cu)
        self.pre = pre or DEFAULT_PRE
        self.post = post or DEFAULT_POST
        self.coarse = coarse_sweeps or DEFAULT_COARSE
        self.levels[0].spmv = self.spmv   # pbicgstab_gpuorder takes A from levels[0]

    @classmethod
    def from_golden(cls, g, **kw):
        """From a tests/golden npz of the A-V system (valA, irow, jcol, geoPHYS_C)."""
        geoC = np.asarray(g["geoPHYS_C"]).reshape(-1)
        sdz, sdy, sdx = g["geoPHYS_C"].shape
        nC = geoC.size
        q = np.flatnonzero(geoC)
        ucell = np.empty(len(q), np.int64)
        ucell[geoC[q] - 3 * nC - 1] = q
        return cls(g["valA"], g["irow"], g["jcol"], (sdx, sdy, sdz), ucell, **kw)

    @classmethod
    def from_solver(cls, s, dims, **kw):
        """From a handle holding the structured A-V form: export_csr() and row_map() (the U unknowns' cells)."""
        valA, irow, jcol = s.export_csr()
        rm = s.row_map().astype(np.int64)
        sdx, sdy, sdz = dims
        nC = sdx * sdy * sdz
        plane = sdx * sdy
        pitch = int(rm[plane] - rm[0]) if sdz > 1 else plane
        nCd = int(rm[nC] - rm[0])
        p = rm[3 * nC:] - 3 * nCd
        return cls(valA, irow, jcol, dims, (p // pitch) * plane + p % pitch, **kw)

    def _cycle(self, l, b):
        L = self.levels[l]
        if l == len(self.levels) - 1:
            x = np.zeros(L.n)
            for _ in range(self.coarse):
                for col in (0, 1, 1, 0):
                    x = L.half_sweep(x, b, col)
            return x
        x = L.init_red(b)
        x = L.half_sweep(x, b, 1)
        for _ in range(self.pre - 1):
            x = L.half_sweep(x, b, 0)
            x = L.half_sweep(x, b, 1)
        C = self.levels[l + 1]
        xc = self._cycle(l + 1, restrict(L, C, L.residual(x, b)))
        x = prolong(L, C, x, xc)
        for _ in range(self.post):
            x = L.half_sweep(x, b, 1)
            x = L.half_sweep(x, b, 0)
        return x

    def project_u(self, bu_cells):
        """bu - (w.bu / w.1) on each component (k_avmg_upart / k_avmg_umean: chunks of UCHUNK entries, thread-strided
        sums and the workgroup tree, then the chunks' partials as k_mg_scalar sums them)."""
        out = bu_cells.copy()
        for cells in self.ucomps:
            prod = self.uweight[cells] * bu_cells[cells]
            parts = []
            for lo in range(0, len(cells), UCHUNK):
                chunk = prod[lo:lo + UCHUNK]
                P = np.zeros(-(-len(chunk) // 256) * 256)
                P[:len(chunk)] = chunk
                P = P.reshape(-1, 256)
                acc = np.zeros(256)
                for m in range(P.shape[0]):
                    acc = acc + P[m]
                parts.append(float(_block_sums(acc.reshape(1, 256))[0]))
            wsum = 0.0
            for v in self.uweight[cells]:
                wsum += float(v)
            mean = mg_scalar_sum(np.array(parts)) * (1.0 / wsum)
            out[cells] = bu_cells[cells] - mean
        return out

    def apply_u(self, bu_cells):
        """The U block's sweeps on a grid-shaped vector (the U unknowns' entries, 0 elsewhere), from its right-hand
        side projected onto the U block's range."""
        U = self.ulevel
        bu_cells = self.project_u(bu_cells)
        x = U.init_red(bu_cells, self.urows)
        x = U.half_sweep(x, bu_cells, 1, self.urows)
        for _ in range(self.pre + self.post - 1):
            x = U.half_sweep(x, bu_cells, 0, self.urows)
            x = U.half_sweep(x, bu_cells, 1, self.urows)
        return x

    def apply(self, r):
        r = np.asarray(r, np.float64)
        nC = self.nC
        z = np.empty(self.n)
        for d in range(3):
            z[d * nC:(d + 1) * nC] = self._cycle(0, r[d * nC:(d + 1) * nC])
        bu = np.zeros(nC)
        bu[self.ucell] = r[3 * nC:]
        z[3 * nC:] = self.apply_u(bu)[self.ucell]
        return z

    def spmv(self, x):
        from oracle import oracle as O
        return O.spmv_csr(self.valA, self.irow, self.jcol, x)
