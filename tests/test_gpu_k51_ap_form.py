"""GPU: K5 inside K1 with the old AP formed on the patch (patch_pair_apc, csrc/ec3d_kernels.hip; EC3D_K51_AP).

k51_p_spmv_dot forms P_new = R + beta*(P_old - omega*AP_old) where the stencil of AP_new = A P_new needs it.  The stored AP_old
is patch_sums over the values that are P_old now, so with EC3D_K51_AP=1 the kernel sums it again for the cells of its own
patch -- from P_old pairs it carries up the march, lane shuffles and a second LDS exchange -- and loads it only on the rim
rows, the edge cells and in a segment's first step.  Same products, same operands, same order: the bar is exact.  Whatever a
handle returns under EC3D_K51_AP=1 equals, bit for bit, what it returns under EC3D_K51_AP=0 (the kernel that loads AP_old
everywhere), and the solves equal the oracle's GPU-order twin.  The fused forms are forced (EC3D_FUSE23=2 EC3D_FUSE51=2):
the grids here are far below the size at which a handle picks them itself.

Grids (those of tests/test_gpu_patch_pairs.py, so that both the paired and the unpaired instance run):
  128 x 64 x 9 at 48 workgroups, 256 x 64 x 9 at 96, 128 x 64 x 24 at 48    pair under EC3D_PATCH=2; three segments per column
  128 x 8 x 9, 128 x 12 x 9                                                pairing refused: the unpaired instance
  128 x 64 x 10 at 48 workgroups (segments of 4, 4, 2 planes)              the last segment's first step: the plane two above
  128 x 64 x 13 at 64 workgroups (segments of 4, 4, 4, 1)                  is the ghost plane / the plane above is
  128 x 8 x 2, 128 x 8 x 3, 128 x 64 x 2                                    grids of two and three planes: the library marches in z
                                                                           from eight planes on, so these have no 2-D tiles and
                                                                           no K5 inside K1 -- the knob must change nothing and the
                                                                           handle must say 0 (two planes: a diffusion operator
                                                                           supplied as CSR; the Poisson assembly wants three)
  a CSR operator on 128 x 64 x 9 whose classes change inside one column    steps that load the class pair of the plane above"""
import struct

import numpy as np
import pytest

import class_runs_numpy as R
import guard_zones as Z

pytestmark = pytest.mark.gpu

# name -> (dims, workgroups asked for)
GRIDS = {
    "128x64x9": ((128, 64, 9), 48),
    "256x64x9": ((256, 64, 9), 96),
    "128x64x24-three-segments": ((128, 64, 24), 48),
    "128x8x9": ((128, 8, 9), None),
    "128x12x9": ((128, 12, 9), None),
    "128x64x10-last-segment-of-two": ((128, 64, 10), 48),
    "128x64x13-last-segment-of-one": ((128, 64, 13), 64),
    "128x8x2": ((128, 8, 2), None),
    "128x8x3": ((128, 8, 3), None),
    "128x64x2": ((128, 64, 2), 16),
}
PAIRING = {"128x64x9", "256x64x9", "128x64x24-three-segments"}      # eight patch rows under EC3D_PATCH=2
POLICY = {"cached": {}, "nontemporal": {"EC3D_NT": "1", "EC3D_KEEP": "0"}}
ENV = ("EC3D_PATCH", "EC3D_FUSE23", "EC3D_FUSE51", "EC3D_K4S", "EC3D_XDEFER", "EC3D_NT", "EC3D_KEEP", "EC3D_K51_AP")
CSR_DIMS = (128, 64, 9)
CSR_CELLS = ((4, 5, 10), (6, 17, 3))     # single cells (k, j, i) whose diagonal gets one STEP more


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()  # raises if the HIP extension is missing: no fallback
    return E


def set_env(monkeypatch, ap, patch=None, policy="cached", k4s="2", xdefer="4", fuse="2"):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if ap is not None:
        monkeypatch.setenv("EC3D_K51_AP", ap)
    if patch is not None:
        monkeypatch.setenv("EC3D_PATCH", patch)
    monkeypatch.setenv("EC3D_FUSE23", fuse)
    monkeypatch.setenv("EC3D_FUSE51", fuse)
    monkeypatch.setenv("EC3D_K4S", k4s)
    monkeypatch.setenv("EC3D_XDEFER", xdefer)
    for k, v in POLICY[policy].items():
        monkeypatch.setenv(k, v)


_systems = {}


def system(key, dims):
    """dict(valA, irow, jcol, b, x0, build): the Poisson cube ("poisson"; at least three planes) or a CSR operator; made once."""
    if (key, dims) not in _systems:
        import csr_grid_generate as GG
        if key == "poisson":
            valA, irow, jcol, c = GG.case("poisson", dims)
            build = lambda s: s.assemble_poisson(*dims)
        else:                     # a diffusion operator supplied as CSR ("csr": with CSR_CELLS; "diffusion": as it is)
            c = GG._diffusion(dims, GG.kappa_of(dims, jump=False))
            for k, j, i in CSR_CELLS if key == "csr" else ():
                c[3, k, j, i] += R.STEP
            c = np.ascontiguousarray(c.reshape(7, -1))
            valA, irow, jcol = GG.bands_to_csr(dims, c)
            build = lambda s: s.set_matrix_csr(valA, irow, jcol)
        n = dims[0] * dims[1] * dims[2]
        rng = np.random.Generator(np.random.PCG64(17 + n))
        sy = dict(valA=valA, irow=irow, jcol=jcol, b=rng.standard_normal(n), x0=rng.standard_normal(n), build=build, dims=dims)
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


def tolerances(sy, hist):
    """A tolerance just above ||S_k|| / ||b|| and one just above ||R_k|| / ||b|| for k = 1 .. 8 (as many as the solve made)."""
    bnorm = float(np.linalg.norm(sy["b"]))
    return [float(hist[k - 1, col]) / bnorm * (1 + 1e-9) for k in range(1, min(8, len(hist)) + 1) for col in (0, 1)]


def results(s, sy, tols):
    """Everything a case compares, in call order: [(label, value)]."""
    b, x0 = sy["b"], sy["x0"]
    out = []
    s.upload("B", b)
    s.upload("X", x0)
    s.iterate_begin()
    for first, count in ((1, 1), (2, 1), (3, 22)):
        s.iterate(first, count)
        s.synchronize()
        out.append((f"P AP R X after {first + count - 1} iterations", [s.download(v) for v in ("P", "AP", "R", "X")]))
    out.append(("converged solve", s.solve(b, x0, 1e-10, 5000, hist_cap=64)))
    for j, tol in enumerate(tols):
        out.append((f"exit {j // 2 + 1} {'SR'[j % 2]}", s.solve(b, x0, tol, 5000, hist_cap=16)))
    # the restart rule |R.R0| / ||b|| < tol (src/solvers.f90:47-49) fires when b is tiny: R.R0 scales with its square
    out.append(("restart", (s.solve(1e-8 * b, 0.0 * x0, 1e-4, 200, hist_cap=16), s.restart_count())))
    bad = np.array(b)
    bad[len(bad) // 3] = np.nan
    out.append(("NaN right-hand side", s.solve(bad, x0, 1e-10, 12, hist_cap=16)))
    out.append(("the solve again, behind the NaN one", s.solve(b, x0, 1e-10, 5000, hist_cap=64)))
    return out


def run(E, sy, nblk, tols=None):
    """(what the handle says it runs, results, the tolerances of the exit solves)"""
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        says = (s.k51_ap_form(), s.patch_rows(2), s.fusion(), s.geometry(1).nblk, s.geometry(1).zm_pps)
        z = Z.zones(s.vector_layout())
        Z.assert_clean(s, z, "fresh")
        if tols is None:
            _, _, hist = s.solve(sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
            tols = tolerances(sy, hist)
        res = results(s, sy, tols)
        Z.assert_clean(s, z, "after every call")
    return says, res, tols


def check_twin(E, oracle, sy, nblk, res):
    """The converged solve, the restart solve and the 24 iterations against the GPU-order twin of the same handle."""
    got = dict(res)
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        a = (sy["valA"], sy["irow"], sy["jcol"])
        xo, ito, hs, hr = oracle.twin_solve(s, *a, sy["b"], sy["x0"], 1e-10, 5000, hist_cap=64)
        x, it, hist = got["converged solve"]
        m = min(it, 64)
        assert it == ito and np.array_equal(x, xo)
        assert np.array_equal(hist[:m, 0], hs[:m]) and np.array_equal(hist[:m - 1, 1], hr[:m - 1])
        assert bits(got["the solve again, behind the NaN one"]) == bits(got["converged solve"])
        xo, ito, _, _ = oracle.twin_solve(s, *a, sy["b"], sy["x0"], 0.0, 23)
        assert ito == 24 and np.array_equal(got["P AP R X after 24 iterations"][3], xo)
        (x, it, _), restarts = got["restart"]
        xo, ito, _, _ = oracle.twin_solve(s, *a, 1e-8 * sy["b"], 0.0 * sy["x0"], 1e-4, 200)
        assert it == ito and np.array_equal(x, xo) and restarts == oracle.last_restart_count() > 0


def compare(E, oracle, monkeypatch, sy, nblk, rows, **knob):
    set_env(monkeypatch, "0", **knob)
    says0, res0, tols = run(E, sy, nblk)
    set_env(monkeypatch, "1", **knob)
    says1, res1, _ = run(E, sy, nblk, tols)
    # the handle says what the knob asked for; rows per workgroup, fusions, workgroups and segments are those of the loading form
    marching = sy["dims"][2] >= 8          # (fewer planes: no z-march, no 2-D tiles, five launches)
    assert says0[0] == 0 and says1[0] == (1 if marching else 0) and says0[1:] == says1[1:]
    assert says1[2] == ((1, 1) if marching else (0, 0)) and (says1[1] > 0) == marching
    assert rows is None or says1[1] == rows
    for (label, a), (_, c) in zip(res0, res1):
        assert bits(a) == bits(c), f"{label}: EC3D_K51_AP=1 differs from EC3D_K51_AP=0"
    x, it, _ = dict(res1)["NaN right-hand side"]
    assert np.isnan(x).any() or it < 12          # (the NaN reaches x, or the solve stopped on it: either way as with =0, above)
    check_twin(E, oracle, sy, nblk, res1)


@pytest.mark.parametrize("policy", sorted(POLICY))
@pytest.mark.parametrize("patch", [None, "2"], ids=["patch-default", "patch2"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_formed_ap_equals_loaded_ap_and_the_twin(E, oracle, monkeypatch, grid, patch, policy):
    dims, nblk = GRIDS[grid]
    rows = 8 if patch == "2" and grid in PAIRING else 4 if grid in PAIRING or (patch is None and dims[2] >= 8) else None
    compare(E, oracle, monkeypatch, system("poisson" if dims[2] > 2 else "diffusion", dims), nblk, rows, patch=patch, policy=policy)


@pytest.mark.parametrize("patch", [None, "2"], ids=["patch-default", "patch2"])
@pytest.mark.parametrize("grid", ["128x64x9", "128x8x3"])
def test_with_k4_as_a_vector_kernel_and_x_updated_every_iteration(E, oracle, monkeypatch, grid, patch):
    dims, nblk = GRIDS[grid]
    compare(E, oracle, monkeypatch, system("poisson", dims), nblk, None, patch=patch, k4s="0", xdefer="1")


@pytest.mark.parametrize("policy", sorted(POLICY))
@pytest.mark.parametrize("patch", [None, "2"], ids=["patch-default", "patch2"])
@pytest.mark.parametrize("nblk", [48, 16], ids=["three-segments", "one-segment"])
def test_classes_that_change_inside_one_column(E, oracle, monkeypatch, nblk, patch, policy):
    """cls_same = 0 on the tiles of planes 4, 5 (column 1) and 6, 7 (column 4): there the class pair of the plane above is
    loaded a step early, and in a pair only one half of the workgroup loads."""
    sy = system("csr", CSR_DIMS)
    compare(E, oracle, monkeypatch, sy, nblk, 8 if patch == "2" else 4, patch=patch, policy=policy)
    set_env(monkeypatch, "1", patch=patch, policy=policy)
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        sdx, sdy, sdz = CSR_DIMS
        tpp = sdx * sdy // 512
        want = {(k, q) for k in (1, sdz - 1) for q in range(tpp)} | {(4, 1), (5, 1), (6, 4), (7, 4)}
        assert R.zero_tiles(np.append(s.class_runs(), 0), sdz, tpp) == want


def test_a_new_matrix_on_the_same_handle(E, oracle, monkeypatch):
    """Re-assembly: the handle reports the form of the matrix it holds and solves that matrix as the twin does."""
    set_env(monkeypatch, "1", patch="2")
    steps = [("poisson", (128, 64, 9), 8), ("poisson", (128, 8, 9), 4), ("csr", CSR_DIMS, 8), ("poisson", (128, 8, 3), 0),
             ("poisson", (128, 64, 9), 8)]
    xs = []
    with E.EC3DSolver(nblk=16) as s:
        for key, dims, rows in steps:
            sy = system(key, dims)
            sy["build"](s)
            assert s.k51_ap_form() == (rows > 0) and s.patch_rows(2) == rows and s.fusion() == ((1, 1) if rows else (0, 0)), (key, dims)
            x, it, _ = s.solve(sy["b"], sy["x0"], 1e-10, 9)
            xo, ito, _, _ = oracle.twin_solve(s, sy["valA"], sy["irow"], sy["jcol"], sy["b"], sy["x0"], 1e-10, 9)
            assert it == ito and np.array_equal(x, xo), (key, dims)
            xs.append(x.tobytes())
    assert xs[0] == xs[4]


def test_handles_without_the_instance_report_the_loading_form(E, monkeypatch):
    """EC3D_K51_AP=1 asks; the five-launch iteration, adopted vectors, plain DIA, z-slabs and the structured A-V form have
    no computing instance and say so."""
    import av_cut_sweep as CS
    dims, nblk = GRIDS["128x64x9"]
    sy = system("poisson", dims)
    set_env(monkeypatch, "1", fuse="0", k4s="0", xdefer="1")
    with E.EC3DSolver(nblk=nblk) as s:                           # five launches
        sy["build"](s)
        assert s.fusion() == (0, 0) and s.k51_ap_form() == 0
    set_env(monkeypatch, "1")
    with E.EC3DSolver(nblk=nblk) as s:                           # the same handle with the three launches: 1; unset: 0
        sy["build"](s)
        assert s.fusion() == (1, 1) and s.k51_ap_form() == 1
    set_env(monkeypatch, None)
    with E.EC3DSolver(nblk=nblk) as s:
        sy["build"](s)
        assert s.fusion() == (1, 1) and s.k51_ap_form() == 0
    set_env(monkeypatch, "1")
    with Z.adopted(E, sy["build"], nblk=nblk) as a:              # caller-owned vectors: no K5 inside K1
        assert a.s.fusion()[1] == 0 and a.s.k51_ap_form() == 0
        za = Z.zones(a.s.vector_layout())
        a.s.solve(sy["b"], sy["x0"], 1e-10, 12)
        Z.assert_clean(a, za, "adopted: after the solve")
    with E.EC3DSolver(nblk=nblk, dictionary=False) as s:        # plain DIA bands: 2-D tiles need the dictionary form
        sy["build"](s)
        assert s.info.dict_classes == 0 and s.k51_ap_form() == 0
    with E.EC3DMulti(2, devices=[0, 0]) as m:                    # z-slabs
        m.assemble_poisson(128, 8, 24)
        for r in range(2):
            assert m.slab(r)[0].k51_ap_form() == 0
    monkeypatch.setenv("EC3D_PITCH", "2")
    with E.EC3DMulti(nranks=1, structured=True) as m:            # the structured A-V form
        m.assemble(*CS.member(16, 6, 3))
        assert m.slab(0)[0].k51_ap_form() == 0
