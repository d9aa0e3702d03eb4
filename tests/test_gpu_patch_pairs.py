"""GPU: paired patch columns of the dictionary form's 2-D tiles (patch_pair with eight patch rows, csrc/ec3d_kernels.hip).

With EC3D_PATCH=2 a launch whose grid allows it (ec3d_patch_pairs_ok in csrc/ec3d_sweep_lists.hpp;
tests/test_patch_pairs_host.py pins the rule on the CPU) runs half as many workgroups of 512 threads, each hosting two
y-adjacent workgroups of the unpaired launch, whose common boundary rows travel through LDS.  Every product, its operands
and the order of every sum are those of the unpaired launch, so the bar is exact: whatever a handle returns under
EC3D_PATCH=2 equals, bit for bit, what it returns under EC3D_PATCH=1 (the kernels from before the pairing), and the solves
equal the oracle's GPU-order twin.

Grids.  The rule wants every XCD label's run of columns to hold an even number of whole patch rows, so of the grids
  128 x 8 x 9, 256 x 16 x 9, 128 x 12 x 9      are REFUSED (two, eight and three columns: a run holds at most one patch) --
                                              the handle must say 4 patch rows and run as under EC3D_PATCH=1;
  128 x 64 x 9 at 48 workgroups               pairs: 16 columns, runs of one pair, three segments of three planes;
  256 x 64 x 9 at 96 workgroups               pairs: 32 columns, two patches per patch row;
  128 x 64 x 24 at 48 workgroups              pairs: three segments of eight planes per column.
(With the workgroups the library picks itself the small grids get four segments for nine planes -- unequal, refused --
so the pairing cases name their count.)  CSR operators on 128 x 64 x 9 whose classes change along z in ONE column of a
pair: the two halves of a workgroup then take different "same classes as below" decisions in the same step."""
import itertools
import struct

import numpy as np
import pytest

import class_runs_numpy as R
import guard_zones as Z

pytestmark = pytest.mark.gpu

# name -> (dims, workgroups asked for, pairs?)
GRIDS = {
    "128x8x9": ((128, 8, 9), None, False),
    "256x16x9": ((256, 16, 9), None, False),
    "128x12x9": ((128, 12, 9), None, False),
    "128x64x9": ((128, 64, 9), 48, True),
    "256x64x9": ((256, 64, 9), 96, True),
    "128x64x24-three-segments": ((128, 64, 24), 48, True),
}
POLICY = {"cached": {}, "nontemporal": {"EC3D_NT": "1", "EC3D_KEEP": "0"}}
KNOBS = list(itertools.product(("0", "2"), ("0", "2"), ("1", "4"), sorted(POLICY)))      # fuse, k4s, xdefer, cache policy
knobs = pytest.mark.parametrize("fuse, k4s, xdefer, policy", KNOBS, ids=[f"fuse{f}-k4s{k}-xd{x}-{p}" for f, k, x, p in KNOBS])
ENV = ("EC3D_PATCH", "EC3D_FUSE23", "EC3D_FUSE51", "EC3D_K4S", "EC3D_XDEFER", "EC3D_NT", "EC3D_KEEP")
CSR_DIMS = (128, 64, 9)
# single cells (k, j, i) whose diagonal gets one STEP more: patch row 1 (upper half of the pair of patch rows 0, 1) at
# plane 4, patch row 4 (lower half of the pair 4, 5) at plane 6
CSR_CELLS = ((4, 5, 10), (6, 17, 3))


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()  # raises if the HIP extension is missing: no fallback
    return E


def set_env(monkeypatch, patch, fuse="0", k4s="0", xdefer="1", policy="cached"):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EC3D_PATCH", patch)
    monkeypatch.setenv("EC3D_FUSE23", fuse)
    monkeypatch.setenv("EC3D_FUSE51", fuse)
    monkeypatch.setenv("EC3D_K4S", k4s)
    monkeypatch.setenv("EC3D_XDEFER", xdefer)
    for k, v in POLICY[policy].items():
        monkeypatch.setenv(k, v)


_systems = {}


def system(key, dims):
    """dict(valA, irow, jcol, b, x0, build): the Poisson cube ("poisson") or the CSR operator with CSR_CELLS; made once."""
    if (key, dims) not in _systems:
        import csr_grid_generate as GG
        if key == "poisson":
            valA, irow, jcol, c = GG.case("poisson", dims)
            build = lambda s: s.assemble_poisson(*dims)
        else:
            c = GG._diffusion(dims, GG.kappa_of(dims, jump=False))
            for k, j, i in CSR_CELLS:
                c[3, k, j, i] += R.STEP
            c = np.ascontiguousarray(c.reshape(7, -1))
            valA, irow, jcol = GG.bands_to_csr(dims, c)
            build = lambda s: s.set_matrix_csr(valA, irow, jcol)
        n = dims[0] * dims[1] * dims[2]
        rng = np.random.Generator(np.random.PCG64(91 + n))
        sy = dict(valA=valA, irow=irow, jcol=jcol, b=rng.standard_normal(n), x0=rng.standard_normal(n), build=build,
                  ids=R.classes_of_bands(c), dims=dims)
        for a in (sy["b"], sy["x0"]):
            a.setflags(write=False)
        _systems[(key, dims)] = sy
    return _systems[(key, dims)]


def bits(v):
    """A value that compares equal exactly when every bit does (NaNs included)."""
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, (tuple, list)):
        return tuple(bits(e) for e in v)
    assert isinstance(v, int), type(v)
    return v


def resident(s, sy, steps):
    s.upload("B", sy["b"])
    s.upload("X", sy["x0"])
    s.iterate_begin()
    for first, count in steps:
        s.iterate(first, count)
    s.synchronize()
    return s.download("X")


def tolerances(sy, hist):
    """A tolerance just above ||S_k|| / ||b|| and one just above ||R_k|| / ||b|| for k = 1 .. 8: the exits at every position
    of two X groups of four."""
    bnorm = float(np.linalg.norm(sy["b"]))
    return [float(hist[k - 1, col]) / bnorm * (1 + 1e-9) for k in range(1, 9) for col in (0, 1)]


def results(s, sy, tols):
    """Everything a case compares, in call order: [(label, value)]."""
    b, x0 = sy["b"], sy["x0"]
    out = [("spmv x0", s.spmv(x0)), ("spmv b", s.spmv(b))]
    s.upload("B", b)
    s.upload("X", x0)
    out.append(("true_residual", s.true_residual()))
    out.append(("24 iterations", resident(s, sy, [(1, 5), (6, 19)])))
    out.append(("converged solve", s.solve(b, x0, 1e-10, 5000, hist_cap=64)))
    for j, tol in enumerate(tols):
        out.append((f"exit {j // 2 + 1} {'SR'[j % 2]}", s.solve(b, x0, tol, 5000, hist_cap=16)))
    # the restart rule |R.R0| / ||b|| < tol (src/solvers.f90:47-49) fires when b is tiny: R.R0 scales with its square
    out.append(("restart", (s.solve(1e-8 * b, 0.0 * x0, 1e-4, 200, hist_cap=16), s.restart_count())))
    return out


def exits_seen(sy, res, tols):
    """{"S", "R"} over the exit solves of `res`."""
    bnorm = float(np.linalg.norm(sy["b"]))
    kinds = set()
    for (_, (_, it, hist)), tol in zip([r for r in res if r[0].startswith("exit")], tols):
        kinds.add("S" if hist[it - 1, 0] / bnorm < tol else "R")
    return kinds


def run(E, sy, nblk, tols=None):
    """(patch rows of the five launch kinds, reduction geometry, class-run flags, results, tolerances of the exit solves)"""
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        rows = [s.patch_rows(k) for k in range(5)]
        if tols is None:
            _, _, hist = s.solve(sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
            tols = tolerances(sy, hist)
        res = results(s, sy, tols)
        geom = (s.geometry(1).nblk, s.geometry(1).zm_pps, s.geometry(1).patch_x, s.geometry(1).patch_y)
        flags = s.class_runs()
    return rows, geom, flags, res, tols


def check_twin(E, oracle, sy, nblk, res):
    """The converged solve, the restart solve and the 24 iterations against the GPU-order twin of the same handle."""
    got = dict(res)
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        a = (sy["valA"], sy["irow"], sy["jcol"])
        xo, ito, hs, hr = oracle.twin_solve(s, *a, sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
        x, it, hist = got["converged solve"]
        m = min(it, 64)
        assert it == ito and it > 8 and np.array_equal(x, xo)
        assert np.array_equal(hist[:m, 0], hs[:m]) and np.array_equal(hist[:m - 1, 1], hr[:m - 1])
        xo, ito, _, _ = oracle.twin_solve(s, *a, sy["b"], sy["x0"], 0.0, 23)
        assert ito == 24 and np.array_equal(got["24 iterations"], xo)
        (x, it, _), restarts = got["restart"]
        xo, ito, _, _ = oracle.twin_solve(s, *a, 1e-8 * sy["b"], 0.0 * sy["x0"], 1e-4, 200)
        assert it == ito and np.array_equal(x, xo) and restarts == oracle.last_restart_count() > 0


def compare(E, oracle, monkeypatch, sy, nblk, paired, knob):
    set_env(monkeypatch, "1", *knob)
    rows1, geom1, flags1, res1, tols = run(E, sy, nblk)
    assert rows1 == [4] * 5 and geom1[2:] == (128, 4)
    set_env(monkeypatch, "2", *knob)
    rows2, geom2, flags2, res2, _ = run(E, sy, nblk, tols)
    # the handle says what it runs; the reduction geometry, the flags and with them the twin see nothing new
    assert rows2 == ([8] * 5 if paired else [4] * 5) and geom2 == geom1 and np.array_equal(flags1, flags2)
    for (label, a), (_, c) in zip(res1, res2):
        assert bits(a) == bits(c), f"{label}: EC3D_PATCH=2 differs from EC3D_PATCH=1"
    assert exits_seen(sy, res2, tols) == {"S", "R"}
    check_twin(E, oracle, sy, nblk, res2)
    return flags2


@knobs
@pytest.mark.parametrize("grid", sorted(g for g, (_, _, paired) in GRIDS.items() if paired))
def test_paired_columns_equal_unpaired_ones_and_the_twin(E, oracle, monkeypatch, grid, fuse, k4s, xdefer, policy):
    dims, nblk, paired = GRIDS[grid]
    compare(E, oracle, monkeypatch, system("poisson", dims), nblk, paired, (fuse, k4s, xdefer, policy))


@pytest.mark.parametrize("fuse, k4s, xdefer, policy", [("0", "0", "1", "cached"), ("2", "2", "4", "nontemporal")],
                         ids=["five-launches", "three-launches"])
@pytest.mark.parametrize("grid", sorted(g for g, (_, _, paired) in GRIDS.items() if not paired))
def test_a_refused_grid_runs_unpaired(E, oracle, monkeypatch, grid, fuse, k4s, xdefer, policy):
    """EC3D_PATCH=2 on a grid the rule refuses: four patch rows in every kind, and the bits of EC3D_PATCH=1."""
    dims, nblk, paired = GRIDS[grid]
    compare(E, oracle, monkeypatch, system("poisson", dims), nblk, paired, (fuse, k4s, xdefer, policy))


@knobs
@pytest.mark.parametrize("nblk", [48, 16], ids=["three-segments", "one-segment"])
def test_classes_that_change_in_one_column_of_a_pair(E, oracle, monkeypatch, nblk, fuse, k4s, xdefer, policy):
    """One half of a workgroup loads its class pair at planes 4 and 5 (6 and 7) while the other half keeps its own."""
    sy = system("csr", CSR_DIMS)
    flags = compare(E, oracle, monkeypatch, sy, nblk, True, (fuse, k4s, xdefer, policy))
    sdx, sdy, sdz = CSR_DIMS
    tpp = sdx * sdy // 512
    want = {(k, q) for k in (1, sdz - 1) for q in range(tpp)} | {(4, 1), (5, 1), (6, 4), (7, 4)}
    assert R.zero_tiles(np.append(flags, 0), sdz, tpp) == want


def test_a_new_matrix_on_the_same_handle(E, oracle, monkeypatch):
    """Re-assembly: a grid that pairs, one that does not, the CSR operator, the first again -- the handle reports the rows of
    the matrix it holds and A*x is that matrix's CSR row sum."""
    set_env(monkeypatch, "2", "2", "2", "4")
    steps = [("poisson", (128, 64, 9), 8), ("poisson", (128, 8, 9), 4), ("csr", CSR_DIMS, 8), ("poisson", (256, 64, 9), 8),
             ("poisson", (128, 64, 9), 8)]
    ys = []
    with E.EC3DSolver(nblk=16) as s:       # (16 workgroups asked for: every column of the grids that pair is one segment of nine planes)
        for key, dims, rows in steps:
            sy = system(key, dims)
            sy["build"](s)
            assert (s.geometry(1).zm_pps == 9 or rows == 4) and [s.patch_rows(k) for k in range(5)] == [rows] * 5, (key, dims)
            y = s.spmv(sy["x0"])
            assert np.array_equal(y, oracle.spmv_csr(sy["valA"], sy["irow"], sy["jcol"], sy["x0"]))
            x, it, _ = s.solve(sy["b"], sy["x0"], 1e-10, 9)
            xo, ito, _, _ = oracle.twin_solve(s, sy["valA"], sy["irow"], sy["jcol"], sy["b"], sy["x0"], 1e-10, 9)
            assert it == ito and np.array_equal(x, xo)
            ys.append(y.tobytes())
    assert ys[0] == ys[4]


@pytest.mark.parametrize("fuse, k4s, xdefer", [("0", "0", "1"), ("2", "2", "4")], ids=["five-launches", "three-launches"])
def test_guard_zones_stay_clean_and_a_nan_solve_leaves_nothing(E, monkeypatch, fuse, k4s, xdefer):
    """The vectors of a paired handle between their guard zones (ghost rows, rows n .. n_pad, the ring buffers) after
    every call, and after a solve whose right-hand side holds a NaN: the next solve is the fresh handle's, bit for bit."""
    dims, nblk, _ = GRIDS["128x64x9"]
    sy = system("poisson", dims)
    set_env(monkeypatch, "2", fuse, k4s, xdefer)
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        assert s.patch_rows(0) == 8
        z = Z.zones(s.vector_layout())
        Z.assert_clean(s, z, "fresh")
        first = s.solve(sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
        Z.assert_clean(s, z, "after the first solve")
        for m in range(0, 9):
            s.solve(sy["b"], sy["x0"], 1e-30, m)
            Z.assert_clean(s, z, f"stopped at itmax {m}")
        bad = np.array(sy["b"])
        bad[len(bad) // 3] = np.nan
        s.solve(bad, sy["x0"], 1e-10, 12)
        Z.assert_clean(s, z, "after the NaN solve")
        again = s.solve(sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
        assert bits(again) == bits(first)
    if fuse == "0":        # caller-owned memory between NaN canaries (adopted vectors run the five launches)
        with Z.adopted(E, sy["build"], nblk=nblk) as a:
            assert a.s.patch_rows(4) == 8 and a.s.fusion() == (0, 0)
            za = Z.zones(a.s.vector_layout())
            got = a.s.solve(sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
            Z.assert_clean(a, za, "adopted: after the solve")
            assert bits(got) == bits(first)
            a.s.spmv(sy["x0"])
            Z.assert_clean(a, za, "adopted: after spmv")


def test_the_cube_of_512_pairs_and_leaves_the_same_x(E, monkeypatch):
    """The headline handle as the library sets it up: x after 16 iterations equals that of EC3D_PATCH=1, all rows; and
    with EC3D_PATCH=2 every launch kind of the cube pairs (512 columns in runs of 64 = 16 patch rows, two segments of 256)."""
    from bench import bar_rhs
    N = 512
    b, x0 = bar_rhs(N), np.zeros(N ** 3)
    out = {}
    for patch in ("1", None, "2"):
        monkeypatch.delenv("EC3D_PATCH", raising=False)
        if patch:
            monkeypatch.setenv("EC3D_PATCH", patch)
        with E.EC3DSolver() as s:
            s.assemble_poisson(N, N, N)
            rows = [s.patch_rows(k) for k in range(5)]
            assert s.geometry(1).nblk == 1024 and s.fusion() == (1, 1)
            assert rows == {"1": [4] * 5, "2": [8] * 5}.get(patch, rows) and set(rows) <= {4, 8}
            x, it, _ = s.solve(b, x0, 1e-300, 15)
            assert it == 16
            out[patch] = x
    assert np.array_equal(out[None], out["1"]) and np.array_equal(out["2"], out["1"])
