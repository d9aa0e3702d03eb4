"""The "same classes as the tile below" flags (csrc/ec3d_sweep_lists.hpp: ec3d_class_runs) restated in numpy, and
generated seven-band operators whose classes change along z at stated planes (tests/test_class_runs_host.py checks the
statements on the CPU; tests/test_gpu_class_runs.py runs the operators on the device).

A class is a row's seven band coefficients, bit for bit: two rows share one exactly when their coefficients are equal.
An operator here is csr_grid_generate's constant-coefficient diffusion operator (ghost-cell Dirichlet faces) with a
non-negative amount added to the DIAGONAL of chosen cells: the rows stay diagonally dominant, the classes of a plane
change exactly where the amounts do, and nowhere else -- apart from the two planes every box has: plane 1 differs from
the face plane 0 below it, and the face plane sdz-1 from the plane below it."""
from __future__ import annotations

import numpy as np

import csr_grid_generate as GG

PX, PY = 128, 4
STEP = 1.0e5     # the amount between two layers: of the order of the face coefficients 1 / h^2 = 4e4 .. 2.5e5


def class_runs(cls, planes, kdz, sdx, px=PX, py=PY):
    """flag[plane k][patch q] = 1 exactly when k > 0 and every class of the px x py patch q of plane k equals the one
    kdz rows below; behind them a plane of zeros and four more (the kernels read a step ahead, by dwords)."""
    c = np.asarray(cls).reshape(planes, kdz // sdx // py, py, sdx // px, px)
    same = (c[1:] == c[:-1]).all(axis=(2, 4))                      # [plane - 1][patch row][patch column]
    tpp = kdz // (px * py)
    flag = np.zeros(planes * tpp + tpp + 4, np.uint8)
    flag[tpp:planes * tpp] = same.reshape(-1)
    return flag


def classes_of_bands(c):
    """One id per distinct column of the (7, n) band array (compared as bit patterns)."""
    _, ids = np.unique(np.ascontiguousarray(c.T).view(np.uint64), axis=0, return_inverse=True)
    return ids.reshape(-1)


def zero_tiles(flag, planes, tpp):
    """{(plane, patch)} above plane 0 whose flag is 0."""
    return {(t // tpp, t % tpp) for t in range(tpp, planes * tpp) if not flag[t]}


# name -> (layer id per plane of a nine-plane box | None, single cells (k, j, i) that get one STEP more)
DIMS = (256, 8, 9)
OPERATORS = {
    "layers_1_2_3": ([0, 1, 2, 2, 3, 3, 3, 4, 4], ()),        # layers of 1, 1, 2, 3 and 2 planes
    "consecutive": ([0, 0, 0, 1, 2, 2, 2, 2, 2], ()),          # two changes on consecutive planes
    "inclusion": ([0] * 9, ((4, 5, 130),)),                    # one cell: patch (1, 1) of plane 4 alone differs
    "segment_edges": ([0, 0, 0, 1, 1, 2, 2, 2, 2], ()),        # with z segments of three planes: first and last plane of the second
    "last_plane": ([0] * 8 + [1], ()),
}


def changed_tiles(name, dims=DIMS):
    """{(plane, patch)} whose classes differ from the tile below, as the table above states them."""
    sdx, sdy, sdz = dims
    npx, tpp = sdx // PX, sdx * sdy // (PX * PY)
    layers, cells = OPERATORS[name]
    planes = {1, sdz - 1} | {k for k in range(1, sdz) if layers[k] != layers[k - 1]}
    out = {(k, q) for k in planes for q in range(tpp)}
    for k, j, i in cells:
        q = (j // PY) * npx + i // PX
        out |= {(k, q), (k + 1, q)}
    return out


def operator(name, dims=DIMS):
    """(valA, irow, jcol, c): the reference's 1-based CSR triple and the (7, n) band array."""
    sdx, sdy, sdz = dims
    layers, cells = OPERATORS[name]
    assert len(layers) == sdz
    c = GG._diffusion(dims, GG.kappa_of(dims, jump=False))
    c[3] += STEP * np.asarray(layers, np.float64)[:, None, None]
    for k, j, i in cells:
        c[3, k, j, i] += STEP
    c = np.ascontiguousarray(c.reshape(7, -1))
    return (*GG.bands_to_csr(dims, c), c)
