"""GPU: class bytes carried up the z-march of the dictionary form's 2-D tiles (patch_pair in csrc/ec3d_kernels.hip).

A workgroup that steps onto a tile whose 512 class bytes equal those of the tile below keeps the class pairs its threads
hold instead of loading them; which tiles those are says one flag byte per tile, made on the device from the class array
whenever one is produced (ec3d_class_runs in csrc/ec3d_sweep_lists.hpp is the rule, tests/test_class_runs_host.py pins
it on the CPU).  Nothing else changes -- same classes, same products in the same order -- so the bars are the parity
suite's: A*x equals the oracle's CSR row sums bit for bit, and every solve (both exits, the itmax exit, bench-style
ec3d_iterate calls) equals the oracle's GPU-order twin bit for bit: x, iter and the residual history.

Grids: 128 x 4 x 5 and 128 x 8 x 6 (one patch / two patch rows per plane; fewer than the eight planes the z-march asks
for, so the flags are made but the kernels that read them do not run), 256 x 8 x 9 and 128 x 4 x 9 (2 x 2 patches / one
patch per plane, z-march on 2-D tiles: the carried classes at work).  EC3D_PATCH=1 throughout, over EC3D_FUSE23 / EC3D_FUSE51
in {0, 2}, EC3D_K4S in {0, 2} and EC3D_XDEFER in {1, 4}."""
import itertools

import numpy as np
import pytest

import class_runs_numpy as R

pytestmark = pytest.mark.gpu

GRIDS = [(128, 4, 5), (128, 8, 6), (256, 8, 9), (128, 4, 9)]
KNOBS = list(itertools.product(("0", "2"), ("0", "2"), ("1", "4")))      # fuse, k4s, xdefer
knobs = pytest.mark.parametrize("fuse, k4s, xdefer", KNOBS, ids=[f"fuse{f}-k4s{k}-xd{x}" for f, k, x in KNOBS])
grid_id = lambda g: "x".join(map(str, g))


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()  # raises if the HIP extension is missing: no fallback
    return E


def set_knobs(monkeypatch, fuse="0", k4s="0", xdefer="1"):
    monkeypatch.setenv("EC3D_PATCH", "1")
    monkeypatch.setenv("EC3D_FUSE23", fuse)
    monkeypatch.setenv("EC3D_FUSE51", fuse)
    monkeypatch.setenv("EC3D_K4S", k4s)
    monkeypatch.setenv("EC3D_XDEFER", xdefer)


_systems = {}


def system(oracle, key, dims):
    """(valA, irow, jcol, class ids per row, b, x0) of "poisson" or of an operator of class_runs_numpy: made once."""
    if (key, dims) not in _systems:
        if key == "poisson":
            import csr_grid_generate as GG
            valA, irow, jcol, c = GG.case("poisson", dims)
        else:
            valA, irow, jcol, c = R.operator(key, dims)
        n = dims[0] * dims[1] * dims[2]
        rng = np.random.Generator(np.random.PCG64(77 + n))
        out = (valA, irow, jcol, R.classes_of_bands(c), rng.standard_normal(n), rng.standard_normal(n))
        for a in out:
            a.setflags(write=False)
        _systems[(key, dims)] = out
    return _systems[(key, dims)]


def host_flags(ids, dims):
    sdx, sdy, sdz = dims
    return R.class_runs(ids, sdz, sdx * sdy, sdx)[:sdz * sdx * sdy // 512]


def check_flags_and_geometry(s, ids, dims):
    """(a) the device's flags are the host rule's on the matrix's classes; the 2-D tiles run from eight planes on."""
    sdx, sdy, sdz = dims
    g = s.geometry(1)
    marching = sdz >= 8
    assert (g.patch_x, g.patch_y, g.patch_sdx) == ((128, 4, sdx) if marching else (0, 0, 0))
    flags = s.class_runs()
    assert flags.dtype == np.uint8 and np.array_equal(flags, host_flags(ids, dims))
    return flags


def check_bits(oracle, s, valA, irow, jcol, b, x0):
    """(b) / (c): SpMV against the CSR row sums, solves against the GPU-order twin, bit for bit."""
    n = len(b)
    assert np.array_equal(s.spmv(x0), oracle.spmv_csr(valA, irow, jcol, x0))
    assert np.array_equal(s.spmv(b), oracle.spmv_csr(valA, irow, jcol, b))
    x, it, hist = s.solve(b, x0, 1e-10, 5000, hist_cap=64)
    xo, ito, hs, hr = oracle.twin_solve(s, valA, irow, jcol, b, x0, 1e-10, 5000, hist_cap=64)
    m = min(it, 64)
    assert it == ito and np.array_equal(x, xo) and it > 6
    assert np.array_equal(hist[:m, 0], hs[:m]) and np.array_equal(hist[:m - 1, 1], hr[:m - 1])
    # both exits: a tolerance just above ||S_k|| / ||b|| or ||R_k|| / ||b|| ends the solve at an iteration <= k
    bnorm = float(np.linalg.norm(b))
    kinds = set()
    for k in range(1, 7):
        for col in (0, 1):
            tol = float(hist[k - 1, col]) / bnorm * (1 + 1e-9)
            xe, ite, _ = s.solve(b, x0, tol, 5000)
            xeo, iteo, hse, _ = oracle.twin_solve(s, valA, irow, jcol, b, x0, tol, 5000, hist_cap=16)
            assert ite == iteo and np.array_equal(xe, xeo), (k, col)
            kinds.add("S" if hse[ite - 1] / bnorm < tol else "R")
    assert kinds == {"S", "R"}
    for itmax in (0, 1, 4, 5):                         # src/solvers.f90:25-29
        xm, itm, _ = s.solve(b, x0, 1e-30, itmax)
        xmo, itmo, _, _ = oracle.twin_solve(s, valA, irow, jcol, b, x0, 1e-30, itmax)
        assert itm == itmo == itmax + 1 and np.array_equal(xm, xmo), itmax
    # bench steps (exits and restart disabled): calls of 5 and 3 iterations leave the X of 8 iterations
    s.upload("B", b)
    s.upload("X", x0)
    s.iterate_begin()
    s.iterate(1, 5)
    s.iterate(6, 3)
    s.synchronize()
    xi = s.download("X")
    xr, itr, _ = s.solve(b, x0, 0.0, 7)
    xro, itro, _, _ = oracle.twin_solve(s, valA, irow, jcol, b, x0, 0.0, 7)
    assert itr == itro == 8 and np.array_equal(xi, xr) and np.array_equal(xr, xro)


@knobs
@pytest.mark.parametrize("dims", GRIDS, ids=grid_id)
def test_poisson_cube_flags_and_bits(E, oracle, monkeypatch, dims, fuse, k4s, xdefer):
    """(a), (b): the natively assembled operator.  Its classes are the 27 positions in the box: every plane strictly
    inside repeats the one below, plane 1 (above the face plane) and the last plane do not."""
    set_knobs(monkeypatch, fuse, k4s, xdefer)
    sdx, sdy, sdz = dims
    valA, irow, jcol, ids, b, x0 = system(oracle, "poisson", dims)
    tpp = sdx * sdy // 512
    with E.EC3DSolver() as s:
        s.assemble_poisson(sdx, sdy, sdz)
        flags = check_flags_and_geometry(s, ids, dims)
        assert R.zero_tiles(np.append(flags, 0), sdz, tpp) == {(k, q) for k in (1, sdz - 1) for q in range(tpp)}
        check_bits(oracle, s, valA, irow, jcol, b, x0)


@knobs
@pytest.mark.parametrize("name", sorted(R.OPERATORS))
def test_csr_operators_whose_classes_change_along_z(E, oracle, monkeypatch, name, fuse, k4s, xdefer):
    """(c): seven-band operators brought as CSR (ec3d_set_matrix_csr ends in the dictionary form): layers of one, two
    and three planes, two changes on consecutive planes, one cell so that exactly one tile of a plane differs, a change
    on the first and on the last plane of a z segment (24 workgroups: three segments of three planes), a change on the
    last plane.  The flags are zero exactly where class_runs_numpy states the changes."""
    set_knobs(monkeypatch, fuse, k4s, xdefer)
    dims = R.DIMS
    sdx, sdy, sdz = dims
    valA, irow, jcol, ids, b, x0 = system(oracle, name, dims)
    tpp = sdx * sdy // 512
    with E.EC3DSolver(nblk=24 if name == "segment_edges" else None) as s:
        s.set_matrix_csr(valA, irow, jcol)
        assert s.info.dict_classes == ids.max() + 1 and s.info.tail_rows == 0
        if name == "segment_edges":
            assert s.geometry(1).nblk == 24 and s.geometry(1).zm_pps == 3      # planes 3 and 5: first and last of [3, 6)
        flags = check_flags_and_geometry(s, ids, dims)
        assert R.zero_tiles(np.append(flags, 0), sdz, tpp) == R.changed_tiles(name)
        check_bits(oracle, s, valA, irow, jcol, b, x0)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("dims", GRIDS + [(128, 8, 30)], ids=grid_id)
def test_z_slabs_on_one_card_equal_the_undivided_handle(E, oracle, monkeypatch, dims, world):
    """(d): the same operator cut into two and three z-slabs on one card (every slab carries flags of its own held
    planes): A*x is the undivided handle's bit for bit; on the grid whose slabs march (128 x 8 x 30) the three-launch
    solve is the slab twin's."""
    set_knobs(monkeypatch, "2", "2", "4")
    sdx, sdy, sdz = dims
    valA, irow, jcol, ids, b, x0 = system(oracle, "poisson", dims)
    with E.EC3DSolver() as s:
        s.assemble_poisson(sdx, sdy, sdz)
        y0, y1 = s.spmv(x0), s.spmv(b)
    assert np.array_equal(y0, oracle.spmv_csr(valA, irow, jcol, x0))
    with E.EC3DMulti(world, devices=[0] * world) as m:
        m.assemble_poisson(sdx, sdy, sdz)
        assert np.array_equal(m.spmv(x0), y0) and np.array_equal(m.spmv(b), y1)
        if sdz >= 30:
            views = [m.slab(r) for r in range(world)]
            assert all(v.geometry(1).patch_x == 128 and len(v.class_runs()) > 0 for v, _, _ in views)
            x, it = m.solve(b, x0, 1e-8, 5000)
            slabs = [(v, k0 * sdx * sdy, k1 * sdx * sdy) for v, k0, k1 in views]
            xo, ito, _, _, _ = oracle.twin_solve_slabs(slabs, m.plan()[0], valA, irow, jcol, b, x0, 1e-8, 5000)
            assert it == ito and np.array_equal(x, xo)


def test_a_new_matrix_on_the_same_handle_gets_new_flags(E, oracle, monkeypatch):
    """(e): the flags belong to the class array they were made from.  One handle takes the Poisson operator, then a CSR
    operator with other classes on the same grid, then one on another grid, then the Poisson operator again: after
    every step the flags are that matrix's and A*x is its CSR row sum, bit for bit."""
    set_knobs(monkeypatch, "2", "2", "4")
    dims = R.DIMS
    steps = [("poisson", dims), ("layers_1_2_3", dims), ("inclusion", dims), ("poisson", (128, 4, 9)), ("consecutive", dims),
             ("poisson", dims)]
    with E.EC3DSolver() as s:
        seen = []
        for key, d in steps:
            valA, irow, jcol, ids, b, x0 = system(oracle, key, d)
            if key == "poisson":
                s.assemble_poisson(*d)
            else:
                s.set_matrix_csr(valA, irow, jcol)
            flags = check_flags_and_geometry(s, ids, d)
            seen.append(flags.tobytes())
            assert np.array_equal(s.spmv(x0), oracle.spmv_csr(valA, irow, jcol, x0))
            x, it, _ = s.solve(b, x0, 1e-10, 9)
            xo, ito, _, _ = oracle.twin_solve(s, valA, irow, jcol, b, x0, 1e-10, 9)
            assert it == ito and np.array_equal(x, xo)
        assert seen[0] == seen[5] and len({seen[0], seen[1], seen[2], seen[4]}) == 4


@pytest.mark.parametrize("fuse, k4s, xdefer", [("0", "0", "1"), ("2", "2", "4")], ids=["five-launches", "three-launches"])
@pytest.mark.parametrize("name", sorted(R.OPERATORS))
def test_one_segment_of_nine_planes(E, oracle, monkeypatch, name, fuse, k4s, xdefer):
    """Eight workgroups: every column is ONE z segment, so a workgroup carries its classes over all nine planes and
    meets every change of the operator in the middle of its march."""
    set_knobs(monkeypatch, fuse, k4s, xdefer)
    dims = R.DIMS
    valA, irow, jcol, ids, b, x0 = system(oracle, name, dims)
    with E.EC3DSolver(nblk=8) as s:
        s.set_matrix_csr(valA, irow, jcol)
        assert s.geometry(1).nblk == 8 and s.geometry(1).zm_pps == dims[2]
        check_flags_and_geometry(s, ids, dims)
        assert np.array_equal(s.spmv(x0), oracle.spmv_csr(valA, irow, jcol, x0))
        x, it, hist = s.solve(b, x0, 1e-10, 5000, hist_cap=64)
        xo, ito, hs, hr = oracle.twin_solve(s, valA, irow, jcol, b, x0, 1e-10, 5000, hist_cap=64)
        m = min(it, 64)
        assert it == ito and np.array_equal(x, xo)
        assert np.array_equal(hist[:m, 0], hs[:m]) and np.array_equal(hist[:m - 1, 1], hr[:m - 1])
