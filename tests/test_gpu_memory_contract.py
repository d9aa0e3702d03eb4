"""GPU: the memory contract of the work vectors, in every kernel form.

Every work vector is [ghost | n_pad | ghost] doubles, zero filled, and the kernels store to rows [0, n) only
(csrc/ec3d_context.hip ec3d_prepare_vectors, csrc/ec3d_kernels.hip store2 / EC3D_MASK2 / row_owned).  The ghosts and the rows
behind n are READ -- multiplied by a zero coefficient, asked for as "the row beside the plane above" -- so a stray finite
value there changes nothing until an Inf meets it.  The parity tests compare the rows of a vector with a twin's; these
look at everything else (tests/guard_zones.py):

(a) a handle that works on caller-owned memory (ec3d_adopt_vectors) between two NaN canaries: after EVERY call the canaries
    are intact, every zone of every vector is zero bytes, and the result is the plain handle's bit for bit; where n < n_pad,
    once more with a finite mark in rows [n, n_pad), which has to come back intact (a stray +0.0 would not show on zeros);
(b) the fused forms, which need the library's own spare buffers: the same zones of the library's block and of every ring
    buffer a stop at itmax = 0 .. 8 hands out, read back through hipMemcpy;
(c) z-slabs on one card: outer ghosts and everything behind the halo planes zero, an interior halo plane of P the
    neighbour's owned plane bit for bit;
(d) a handle has no memory of a solve whose scalars went NaN or Inf: the next clean solve on it -- ec3d_solve, upload +
    ec3d_solve_resident, rhs_step -> solve -> post_update -- is a fresh handle's bit for bit and leaves the zones clean;
(e) a new matrix on the same handle: clean zones and a fresh handle's bits after every step;
(f) the lists below hold what they are meant to hold.

Every assertion is exact: bytes are zero, bits are equal, a canary is intact."""
import itertools
import struct

import numpy as np
import pytest

import av_grids as AGR
import class_runs_numpy as R
import csr_generate as G
import guard_zones as Z
from conftest import load_golden

pytestmark = pytest.mark.gpu

KNOBS = ("EC3D_PATCH", "EC3D_FUSE23", "EC3D_FUSE51", "EC3D_K4S", "EC3D_XDEFER", "EC3D_XASYNC", "EC3D_NT", "EC3D_KEEP",
         "EC3D_PITCH", "EC3D_SAV_PATCH", "EC3D_SAV_IL", "EC3D_NBLK_SPMV")
AV = {"g2": "g2_conducting_hole_16x15x14", "g3": "g3_moving_coil_18x16x12", "g8a": "g8a_two_plates_18x16x16"}
PITCH = {"auto": {}, "pitched": {"EC3D_PITCH": "2"}}
# the interleaved z-march as tests/test_gpu_interleaved.py forces it (it needs tile-aligned planes: pitched only)
SAV_FORM = {"linear": {"EC3D_SAV_PATCH": "0"}, "patch": {"EC3D_SAV_PATCH": "2"},
            "interleaved": {"EC3D_SAV_IL": "2", "EC3D_PITCH": "2", "EC3D_SAV_PATCH": "0", "EC3D_NT": "1"}}
PATCH = {"EC3D_PATCH": "1"}
LINEAR = {"EC3D_PATCH": "0"}       # 2-D tiles are the default of a dictionary-form grid that marches

# (a): id -> (kind, what, environment, handle arguments)
ADOPTED = {
    "poisson-3x3x3": ("poisson", (3, 3, 3), {}, {}),
    "poisson-17x9x5": ("poisson", (17, 9, 5), {}, {}),                     # n = 765: 259 padding rows
    "poisson-128x4x5": ("poisson", (128, 4, 5), {}, {}),                   # no z-march
    "poisson-128x4x9-patch": ("poisson", (128, 4, 9), PATCH, {}),          # 2-D tiles, carried classes
    "poisson-256x8x9-patch": ("poisson", (256, 8, 9), PATCH, {}),
    "poisson-128x12x10-linear": ("poisson", (128, 12, 10), LINEAR, {}),    # linear z-march
    "bands-128x12x10": ("poisson", (128, 12, 10), LINEAR, {"dictionary": False}),
    "poisson-128x12x10-linear-nt1-keep0": ("poisson", (128, 12, 10), {**LINEAR, "EC3D_NT": "1", "EC3D_KEEP": "0"}, {}),
    "poisson-128x12x10-linear-nt1-keep43": ("poisson", (128, 12, 10), {**LINEAR, "EC3D_NT": "1", "EC3D_KEEP": "43"}, {}),
    "csr-nb3": ("csr", "nb3", {}, {}),                                     # N0 = 1537: 511 padding rows
    "csr-long_row": ("csr", "long_row", {}, {}),                           # a tail: not a stencil
    "operator-layers_1_2_3": ("operator", "layers_1_2_3", PATCH, {}),
    "operator-inclusion": ("operator", "inclusion", PATCH, {}),
}
for _g, _p, _f in itertools.product(AV, PITCH, SAV_FORM):
    if _f != "interleaved" or _p == "pitched":
        ADOPTED[f"{_g}-{_p}-{_f}"] = ("av", _g, {**PITCH[_p], **SAV_FORM[_f]}, {})
# the interleaved march on three columns: planes of 1200 cells in 1536 rows (tests/av_grids.py S3), tiles that start
# mid-row, 336 padding rows behind every plane in the third; eight workgroups asked for, so segments start inside the conductor
ADOPTED["grid-S3-pitched-interleaved"] = ("avgrid", "S3", {**SAV_FORM["interleaved"], "EC3D_NBLK_SPMV": "8"}, {})

# (b): the forms that need the spare pair and the rings
OWNED_GRIDS = [(256, 8, 9), (128, 12, 10)]
OWNED_KNOBS = list(itertools.product(("0", "2"), ("0", "2"), ("1", "3", "4"), (None, "2", "3")))   # fuse, k4s, xdefer, xasync
OWNED = {f"poisson-{'x'.join(map(str, d))}-fuse{f}-k4s{k}-xd{x}-xa{a}":
         ("poisson", d, {**PATCH, "EC3D_FUSE23": f, "EC3D_FUSE51": f, "EC3D_K4S": k, "EC3D_XDEFER": x,
                         **({} if a is None else {"EC3D_XASYNC": a})}, {})
         for d in OWNED_GRIDS for f, k, x, a in OWNED_KNOBS}
PATCH_FUSED = {"EC3D_SAV_PATCH": "2", "EC3D_FUSE23": "2", "EC3D_FUSE51": "2"}      # conftest's sav_tiles = patch-fused
for _g, _p in itertools.product(("g2", "g3"), PITCH):
    OWNED[f"{_g}-{_p}-patch-fused"] = ("av", _g, {**PITCH[_p], **PATCH_FUSED}, {})
RING_STOPS = range(0, 9)          # itmax = 0 .. 8: two groups of EC3D_XDEFER = 4, the deepest rings there are

THREE_LAUNCH = {**PATCH, "EC3D_FUSE23": "2", "EC3D_FUSE51": "2", "EC3D_K4S": "2", "EC3D_XDEFER": "4"}
# (d)
BAD_SOLVE = {
    "poisson-17x9x5": ("poisson", (17, 9, 5), {}, {}),
    "csr-nb3": ("csr", "nb3", {}, {}),
    "g2-auto": ("av", "g2", {}, {}),
    "g2-pitched": ("av", "g2", PITCH["pitched"], {}),
    "g8a-pitched": ("av", "g8a", PITCH["pitched"], {}),
    "poisson-256x8x9-three-launch-xd4": ("poisson", (256, 8, 9), THREE_LAUNCH, {}),
    # 336 rows of padding behind every plane of the third column, which a NaN solve leaves as 0 + NaN * 0
    "grid-S3-pitched-interleaved": ADOPTED["grid-S3-pitched-interleaved"],
}
BAD_KINDS = ("nan", "overflow")
# (e)
NEW_MATRIX = [("poisson", (256, 8, 9), PATCH, {}), ("csr", "nb3", PATCH, {}), ("av", "g2", {**PATCH, **PITCH["pitched"]}, {}),
              ("poisson", (128, 4, 9), PATCH, {}), ("poisson", (128, 4, 9), PATCH, {"nblk": 8})]


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()  # raises if the HIP extension is missing: no fallback
    return E


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in KNOBS
        monkeypatch.setenv(k, v)


# ---- systems: made once, read-only ------------------------------------------------------------------------------------
_systems = {}


def system(kind, what):
    """dict(build(s), n, b, x0, itmax, plane (cells of an xy plane, A-V only), g (the captured case, A-V only))."""
    if (kind, what) not in _systems:
        if kind == "poisson":
            n = what[0] * what[1] * what[2]
            sy = dict(build=lambda s: s.assemble_poisson(*what), n=n, itmax=5000)
        elif kind == "av":
            g = load_golden(AV[what])
            sdz, sdy, sdx = g["geoPHYS"].shape
            sy = dict(build=lambda s: s.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"],
                                                 float(g["dt"])),
                      n=len(g["irow"]) - 1, itmax=400, plane=sdx * sdy, cells=sdx * sdy * sdz, g=g,
                      b=np.array(g["b0"]), x0=np.array(g["xin0"]))
        elif kind == "avgrid":
            args = AGR.system(what)
            sdx, sdy, sdz = AGR.GRIDS[what]["dims"]
            sy = dict(build=lambda s: s.assemble(*args), n=3 * sdx * sdy * sdz + int(np.count_nonzero(args[1])), itmax=400,
                      plane=sdx * sdy, cells=sdx * sdy * sdz)
        else:
            valA, irow, jcol = G.case(what)[:3] if kind == "csr" else R.operator(what, R.DIMS)[:3]
            sy = dict(build=lambda s: s.set_matrix_csr(valA, irow, jcol), n=len(irow) - 1, itmax=5000)
        if "b" not in sy:
            rng = np.random.Generator(np.random.PCG64(77 + sy["n"]))
            sy["b"], sy["x0"] = rng.standard_normal(sy["n"]), rng.standard_normal(sy["n"])
        sy["b"].setflags(write=False)
        sy["x0"].setflags(write=False)
        _systems[(kind, what)] = sy
    return _systems[(kind, what)]


def bits(v):
    """A value that compares equal exactly when every bit does (NaNs included)."""
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, (tuple, list)):
        return tuple(bits(e) for e in v)
    if isinstance(v, dict):
        return tuple((k, bits(e)) for k, e in sorted(v.items()))
    assert v is None or isinstance(v, (int, str)), type(v)
    return v


def exit_tolerances(s, sy, hist, it):
    """One tolerance that ends the solve at the S exit and one that ends it at the R exit, picked as
    tests/test_gpu_class_runs.py check_bits does: just above ||S_k|| / ||b|| or ||R_k|| / ||b|| of an early iteration."""
    bnorm = float(np.linalg.norm(sy["b"]))
    found = {}
    for k in range(1, min(it, 13)):
        for col in (0, 1):
            if not np.isfinite(hist[k - 1, col]) or hist[k - 1, col] <= 0.0:
                continue
            tol = float(hist[k - 1, col]) / bnorm * (1 + 1e-9)
            _, ite, he = s.solve(sy["b"], sy["x0"], tol, sy["itmax"], hist_cap=16)
            if ite <= 16 and ite <= sy["itmax"]:
                found.setdefault("S" if he[ite - 1, 0] / bnorm < tol else "R", tol)
        if len(found) == 2:
            break
    assert set(found) == {"S", "R"}, found
    return found


def resident_x(s, sy, steps):
    s.upload("B", sy["b"])
    s.upload("X", sy["x0"])
    s.iterate_begin()
    for first, count in steps:
        s.iterate(first, count)
    s.synchronize()
    return s.download("X")


def calls(sy, tols):
    """[(label, f(handle) -> result)]: what (a) and (b) run in turn."""
    b, x0, itmax = sy["b"], sy["x0"], sy["itmax"]
    out = [("spmv x0", lambda s: s.spmv(x0)), ("spmv b", lambda s: s.spmv(b)),
           ("solve 1e-10", lambda s: s.solve(b, x0, 1e-10, itmax, hist_cap=64)),
           ("S exit", lambda s: s.solve(b, x0, tols["S"], itmax, hist_cap=16)),
           ("R exit", lambda s: s.solve(b, x0, tols["R"], itmax, hist_cap=16))]
    for m in (0, 1, 4):
        out.append((f"itmax {m}", lambda s, m=m: s.solve(b, x0, 1e-30, m)))
    out.append(("iterate(1, 5) + iterate(6, 3)", lambda s: resident_x(s, sy, [(1, 5), (6, 3)])))
    out.append(("true_residual", lambda s: s.true_residual()))
    if "g" in sy:      # the time loop's field work on the resident vectors
        g = sy["g"]
        idx = np.arange(1, 3 * sy["cells"] + 1, 97, dtype=np.int32)
        val = np.linspace(-1.0, 1.0, len(idx))

        def both(s):
            return s.download("B"), s.download("X")

        def load(s):
            s.upload("B", g["b0"])
            s.upload("X", g["xout0"])
            return both(s)
        out += [("upload b0, xout0", load),
                ("post_update", lambda s: (s.post_update(), both(s))[1]),
                ("rhs_step moving=0", lambda s: (s.rhs_step(idx, val, moving=False), both(s))[1]),
                ("rhs_step moving=1", lambda s: (s.rhs_step(idx, val, moving=True), both(s))[1]),
                ("vtk_fields", lambda s: s.vtk_fields(g["delta"], sy["cells"], True)),
                ("domain_integrals", lambda s: s.domain_integrals(g["delta"]))]
    return out


def zones_of(s, sy):
    return Z.zones(s.vector_layout(), Z.pitch_info(s, sy["plane"]) if "plane" in sy else None)


def check_form(s, kind, what, env):
    """The case reaches the form it is listed for."""
    g = s.geometry(1)
    if kind in ("poisson", "operator"):
        sdx, sdy, sdz = what if kind == "poisson" else R.DIMS
        marching = sdz >= 8 and (sdx * sdy) % 512 == 0          # the z-march asks for eight planes of whole tiles
        assert (g.zm_tpp > 0) == marching
        patches = marching and env.get("EC3D_PATCH") == "1" and s.info.dict_classes > 0
        assert env.get("EC3D_PATCH") in ("0", "1") or not marching          # every marching case says which tiles it means
        assert (g.patch_x, g.patch_y) == ((128, 4) if patches else (0, 0))
    if kind in ("av", "avgrid"):
        pi = Z.pitch_info(s, system(kind, what)["plane"])
        assert pi is not None and len(pi["hidden"]) > 0                      # the structured form
        if env.get("EC3D_PITCH") == "2":
            assert pi["pitch"] % 512 == 0 and pi["pitch"] > pi["plane"]
        else:
            assert pi["pitch"] == pi["plane"]
        # the 2-D tiles of the structured kernels (and with them the fused launches) need tile-aligned planes
        patches = env.get("EC3D_SAV_PATCH") == "2" and env.get("EC3D_PITCH") == "2"
        assert (g.patch_x > 0 and g.patch_y > 0) if patches else (g.patch_x, g.patch_y) == (0, 0)
        if not patches:
            assert s.fusion() == (0, 0)
        if env.get("EC3D_SAV_IL") == "2":
            assert g.ulist_n == 0 and len(s.ulist()) > 0                     # the U tiles are inside the march
        if kind == "avgrid":
            assert g.zm_tpp == 3 and pi["pitch"] == 1536 and pi["plane"] == 1200 and s.n == system(kind, what)["n"]
            assert [int(t) for t in s.ulist()] == AGR.u_tiles(what)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(ADOPTED))
def test_adopted_vectors_between_canaries(E, monkeypatch, case):
    kind, what, env, args = ADOPTED[case]
    set_env(monkeypatch, env)
    sy = system(kind, what)
    with E.EC3DSolver(**args) as plain:
        sy["build"](plain)
        check_form(plain, kind, what, env)
        _, it, hist = plain.solve(sy["b"], sy["x0"], 1e-10, sy["itmax"], hist_cap=64)
        todo = calls(sy, exit_tolerances(plain, sy, hist, it))
        want = [bits(f(plain)) for _, f in todo]
    with Z.adopted(E, sy["build"], **args) as a:
        s = a.s
        # adopted vectors get no spare pair: five launches, X updated in every iteration
        assert s.fusion() == (0, 0) and s.x_interval() == 1
        z = zones_of(s, sy)
        assert z["rows n..n_pad"].size == a.layout["n_pad"] - a.layout["n"]
        Z.assert_clean(a, z, f"{case}: after ec3d_adopt_vectors")
        for (label, f), w in zip(todo, want):
            got = bits(f(s))
            Z.assert_clean(a, z, f"{case}: after {label}")
            assert got == w, f"{case}: {label} differs from the plain handle"
        padded = a.layout["n_pad"] > a.layout["n"]
    if padded:
        # "rows >= n are never stored": a stray store of the +0.0 a kernel computes there cannot be told from untouched
        # zeros, so once more with a finite mark in rows [n, n_pad) of every vector.  No kernel stores there, the rows
        # beside them see them through a zero coefficient and the dot products leave them out: the marks are intact and
        # the results the same bits.
        with Z.adopted(E, sy["build"], mark_padding=True, **args) as a:
            for (label, f), w in zip(todo, want):
                got = bits(f(a.s))
                Z.assert_clean(a, z, f"{case}: marked padding rows: after {label}")
                assert got == w, f"{case}: marked padding rows: {label} differs from the plain handle"


# ---- (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(OWNED))
def test_library_owned_vectors_and_rings(E, monkeypatch, case):
    kind, what, env, args = OWNED[case]
    set_env(monkeypatch, env)
    sy = system(kind, what)
    with E.EC3DSolver(**args) as s:
        sy["build"](s)
        check_form(s, kind, what, env)
        fuse = 1 if env["EC3D_FUSE23"] == "2" and s.geometry(1).patch_x > 0 else 0      # (check_form: which cases have 2-D tiles)
        assert s.fusion() == (fuse, fuse), case
        if "EC3D_XDEFER" in env:
            assert s.x_interval() == int(env["EC3D_XDEFER"]), case
        z = zones_of(s, sy)
        Z.assert_clean(s, z, f"{case}: fresh")
        _, it, hist = s.solve(sy["b"], sy["x0"], 1e-10, sy["itmax"], hist_cap=64)
        Z.assert_clean(s, z, f"{case}: after the first solve")
        for label, f in calls(sy, exit_tolerances(s, sy, hist, it)):
            f(s)
            Z.assert_clean(s, z, f"{case}: after {label}")
        seen = set()
        for m in RING_STOPS:
            s.solve(sy["b"], sy["x0"], 1e-30, m)
            seen |= {name.split("@")[1] for name in Z.rings(s)}
            Z.assert_clean(s, z, f"{case}: stopped at itmax {m}")
        # every buffer ec3d_spare_pair lays out has been handed out at one stop or another: the second AP (K5 inside K1), the
        # P ring (either) and the S ring (deferred X update) of D buffers, 2 D when the groups of X updates run on a second
        # stream (EC3D_XASYNC=2); the buffer among the eight vectors is one of each ring
        D = s.x_interval()
        cap = 2 * D if D > 1 and env.get("EC3D_XASYNC") == "2" else D
        want = (max(2, cap) - 1 if fuse or D > 1 else 0) + (1 if fuse else 0) + (cap - 1 if D > 1 else 0)
        assert len(seen) == want, (case, sorted(seen), want)


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def bad_rhs(sy, kind):
    b = np.array(sy["b"])
    if kind == "nan":
        b[sy["n"] // 3] = np.nan
    else:                       # ||b||^2 overflows
        b[:] = 0.0
        b[sy["n"] // 3] = 1e308
    return b


def routes(sy):
    """{name: f(handle) -> result}: the ways a clean system reaches a handle."""
    b, x0, itmax = sy["b"], sy["x0"], sy["itmax"]

    def resident(s):
        s.upload("B", b)
        s.upload("X", x0)
        it, hist = s.solve_resident(1e-10, itmax, hist_cap=64)
        return it, hist, s.download("X"), s.true_residual()
    out = {"solve": lambda s: s.solve(b, x0, 1e-10, itmax, hist_cap=64), "upload + solve_resident": resident}
    if "g" in sy:
        g = sy["g"]
        idx = np.arange(1, 3 * sy["cells"] + 1, 97, dtype=np.int32)
        val = np.linspace(-1.0, 1.0, len(idx))

        def time_step(s):
            s.upload("B", g["b0"])
            s.upload("X", g["xout0"])
            s.post_update()
            s.rhs_step(idx, val, moving=False)
            it, hist = s.solve_resident(float(g["tol"]), int(g["itmax"]), hist_cap=64)
            s.post_update()
            return it, hist, s.download("X"), s.download("B"), s.vtk_fields(g["delta"], sy["cells"], True)
        out["rhs_step -> solve -> post_update"] = time_step
    return out


@pytest.mark.parametrize("bad", BAD_KINDS)
@pytest.mark.parametrize("case", sorted(BAD_SOLVE))
def test_a_handle_has_no_memory_of_a_bad_solve(E, monkeypatch, case, bad):
    kind, what, env, args = BAD_SOLVE[case]
    set_env(monkeypatch, env)
    sy = system(kind, what)
    todo = routes(sy)
    want = {}
    for name, f in todo.items():            # a fresh handle each
        with E.EC3DSolver(**args) as s:
            sy["build"](s)
            check_form(s, kind, what, env)
            want[name] = bits(f(s))
    bb = bad_rhs(sy, bad)
    with E.EC3DSolver(**args) as s:
        sy["build"](s)
        z = zones_of(s, sy)
        for name, f in todo.items():
            x, it, _ = s.solve(bb, np.zeros(sy["n"]), 1e-6, 7)
            assert not np.isfinite(x).all(), f"{case}: the {bad} solve stayed finite"
            got = bits(f(s))
            assert got == want[name], f"{case}: {name} after a {bad} solve differs from a fresh handle"
            Z.assert_clean(s, z, f"{case}: {name} after a {bad} solve")


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def slab_blocks(m, world):
    """Per slab: (view, k0, k1, layout, the eight vectors as [8, len] bit patterns, the vector it hands out as P now)."""
    m.synchronize()
    out = []
    for r in range(world):
        v, k0, k1 = m.slab(r)
        lay = v.vector_layout()
        ln = 2 * lay["ghost"] + lay["n_pad"]
        p = v.device_vector("P")[0]
        out.append(dict(view=v, k0=k0, k1=k1, lay=lay, vec=Z.owned_block(v)[1], P=Z.peek(p - 8 * lay["ghost"], ln)))
    return out


def check_grid_slabs(slabs, kdz, where, exchanged=True):
    """Slabs of a single-component grid: the halo planes are the kdz rows below row 0 and the kdz rows from row n on
    (ec3d_multi.hip: recv_lo = [-kdz, 0), recv_hi = [n, n + kdz)).  Rows [n, n_pad) are never stored by a kernel, but on a
    slab with an upper neighbour they overlap that halo plane (csrc/ec3d_kernels.hip, above store2): there they hold what
    the exchange put there, like the rest of the plane; everything else around the rows is zero bytes."""
    world = len(slabs)
    for r, s in enumerate(slabs):
        g, n, n_pad = s["lay"]["ghost"], s["lay"]["n"], s["lay"]["n_pad"]
        assert s["lay"]["halo"] == kdz <= g and n == (s["k1"] - s["k0"]) * kdz
        lo = 0 if r == 0 else kdz                       # rows of the lower / upper ghost the exchange may fill
        hi = 0 if r == world - 1 else kdz
        z = {"lower ghost": np.arange(0, g - lo, dtype=np.int64),
             "behind the upper halo plane": np.arange(g + n + hi, g + n_pad + g, dtype=np.int64)}
        if hi == 0:
            assert np.array_equal(z["behind the upper halo plane"][:n_pad - n], np.arange(g + n, g + n_pad))   # rows n..n_pad
        found = Z.findings(s["vec"], z) + Z.findings([s["P"]], z, names=("P as handed out",))
        assert not found, f"{where}: slab {r}:\n  " + "\n  ".join(found)
        # an interior ghost plane of P holds the neighbour's owned plane, bit for bit
        if r > 0:
            below = slabs[r - 1]
            gb, nb = below["lay"]["ghost"], below["lay"]["n"]
            assert np.array_equal(s["P"][g - kdz:g], below["P"][gb + nb - kdz:gb + nb]), f"{where}: slab {r}: lower halo of P"
        if r < world - 1:
            above = slabs[r + 1]
            ga = above["lay"]["ghost"]
            assert np.array_equal(s["P"][g + n:g + n + kdz], above["P"][ga:ga + kdz]), f"{where}: slab {r}: upper halo of P"
            assert np.any(s["P"][g + n:g + n + kdz] != 0) == exchanged, f"{where}: slab {r}: the upper halo of P"


GRID_SLABS = {"24x24x24": ((24, 24, 24), {}), "128x8x30-three-launch": ((128, 8, 30), THREE_LAUNCH)}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", sorted(GRID_SLABS))
def test_z_slabs_of_a_grid_on_one_card(E, monkeypatch, case, world):
    dims, env = GRID_SLABS[case]
    set_env(monkeypatch, env)
    sy = system("poisson", dims)
    kdz = dims[0] * dims[1]
    with E.EC3DSolver() as s:
        s.assemble_poisson(*dims)
        y = s.spmv(sy["x0"])
    with E.EC3DMulti(world, devices=[0] * world) as m:
        m.assemble_poisson(*dims)
        views = [m.slab(r)[0] for r in range(world)]
        if env:
            assert m.plan()[0] in (3, 4) and all(v.geometry(1).patch_x == 128 for v in views)      # marching slabs, three launches
        else:
            assert m.plan()[0] == 0 or all(v.geometry(1).patch_x == 0 for v in views)
        check_grid_slabs(slab_blocks(m, world), kdz, f"{case}: fresh", exchanged=False)
        assert np.array_equal(m.spmv(sy["x0"]), y)
        check_grid_slabs(slab_blocks(m, world), kdz, f"{case}: after spmv")
        x, it = m.solve(sy["b"], sy["x0"], 1e-8, 5000)
        assert it <= 5000 and np.isfinite(x).all()
        check_grid_slabs(slab_blocks(m, world), kdz, f"{case}: after a solve")


@pytest.mark.parametrize("world", [2, 3])
def test_z_slabs_of_the_av_system_on_one_card(E, monkeypatch, world):
    """g2 as A-V slabs: a slab holds its owned planes and two halo planes per interior side INSIDE its rows (extended
    grid), so both ghosts and rows [n, n_pad) are zero on every slab.  Of the three A blocks ONE plane per side travels --
    the 7-point stencil and the U rows read A one plane away (ec3d_multi.hip av_layout) -- and holds the neighbour's
    owned plane of P bit for bit."""
    set_env(monkeypatch, {})
    sy = system("av", "g2")
    g = sy["g"]
    sdz, plane, H, T = g["geoPHYS"].shape[0], sy["plane"], 2, 1         # planes held / travelling per interior side
    with E.EC3DMulti(world, devices=[0] * world) as m:
        m.assemble(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))

        def check(where):
            slabs = slab_blocks(m, world)
            for r, s in enumerate(slabs):
                z = Z.zones(s["lay"])
                found = Z.findings(s["vec"], z) + Z.findings([s["P"]], z, names=("P as handed out",))
                assert not found, f"{where}: slab {r}:\n  " + "\n  ".join(found)
                e0, e1 = max(0, s["k0"] - H), min(sdz, s["k1"] + H)
                pi = Z.pitch_info(s["view"], plane)
                s["pitch"] = pi["pitch"] if pi else plane
                s["block"] = s["pitch"] * (e1 - e0)
                s["e0"] = e0
                assert s["lay"]["n"] >= 3 * s["block"]

            def planes(s, d, k_lo, k_hi):       # rows of planes [k_lo, k_hi) (global numbering) of component d, payload only
                rows = [s["lay"]["ghost"] + d * s["block"] + (k - s["e0"]) * s["pitch"] + np.arange(plane) for k in range(k_lo, k_hi)]
                return s["P"][np.concatenate(rows)]
            for r in range(1, world):
                lower, upper = slabs[r - 1], slabs[r]
                cut = upper["k0"]
                assert lower["k1"] == cut
                for d in range(3):
                    assert np.array_equal(planes(upper, d, cut - T, cut), planes(lower, d, cut - T, cut)), (where, r, d, "lower halo")
                    assert np.array_equal(planes(lower, d, cut, cut + T), planes(upper, d, cut, cut + T)), (where, r, d, "upper halo")
                assert any(np.any(planes(upper, d, cut - T, cut) != 0) for d in range(3)), (where, r)
        rng = np.random.Generator(np.random.PCG64(5))
        xs = rng.standard_normal(sy["n"])
        with E.EC3DSolver() as s:
            sy["build"](s)
            y = s.spmv(xs)
        assert np.array_equal(m.spmv(xs), y)
        check("after spmv")
        x, it = m.solve(sy["b"], sy["x0"], float(g["tol"]), int(g["itmax"]))
        assert it <= int(g["itmax"]) and np.isfinite(x).all()
        check("after a solve")


def test_the_staged_driver_uploads_over_what_a_bad_solve_left(E, monkeypatch):
    """dist.py HipAVSlabOps.set_vector scatters the unknowns into torch-owned vectors: the rows that hold no unknown are
    zero afterwards, whatever they held (a NaN here, put by the test)."""
    from eddy_currents_3d_amd.dist import HipAVSlabOps
    set_env(monkeypatch, PITCH["pitched"])
    g = system("av", "g2")["g"]
    sdz = g["geoPHYS"].shape[0]
    ops = HipAVSlabOps(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]), 0, sdz, 1,
                       structured=True)
    try:
        assert ops.structured and ops.n_ref == len(g["b0"])
        pi = Z.pitch_info(ops.local, 16 * 15)
        hidden = pi["hidden"]
        assert pi["pitch"] == 512 and np.array_equal(hidden, np.setdiff1d(np.arange(ops.n), ops._rm.cpu().numpy()))
        gaps = hidden[hidden % 512 >= 16 * 15]
        assert len(gaps) > 0 and len(hidden) > len(gaps)          # rows between pitched planes, and empty U slots
        b = ops._base("X")
        with ops.context():
            ops.store[b + int(gaps[0])] = float("nan")
            ops.store[b + int(hidden[-1])] = float("inf")
        ops.set_vector("X", g["xout0"])
        with ops.context():
            rows = ops.store[b:b + ops.n].cpu().numpy()
        assert not rows[hidden].view(np.uint64).any()
        assert np.array_equal(ops.get_vector("X"), g["xout0"])
    finally:
        ops.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------
def test_a_new_matrix_on_the_same_handle(E, monkeypatch):
    with E.EC3DSolver() as s:
        for step, (kind, what, env, args) in enumerate(NEW_MATRIX):
            set_env(monkeypatch, env)
            sy = system(kind, what)
            if "nblk" in args:
                s.set_workgroups(args["nblk"])          # the matrix of the step before stays
            else:
                sy["build"](s)
            with E.EC3DSolver(**args) as fresh:
                sy["build"](fresh)
                want = bits(fresh.solve(sy["b"], sy["x0"], 1e-10, sy["itmax"], hist_cap=64))
                assert fresh.geometry(1).nblk == s.geometry(1).nblk and fresh.vector_layout() == s.vector_layout()
            z = zones_of(s, sy)
            Z.assert_clean(s, z, f"step {step}: fresh")
            assert bits(s.solve(sy["b"], sy["x0"], 1e-10, sy["itmax"], hist_cap=64)) == want, f"step {step}"
            Z.assert_clean(s, z, f"step {step}: after the solve")
        assert s.geometry(1).nblk == 8


# ---- the check itself --------------------------------------------------------------------------------------------------
def test_the_check_sees_a_negative_zero_and_a_touched_canary(E, monkeypatch):
    """A mark of the smallest kind, put by the test itself INSIDE the block it looks at, is reported; taken out, the block
    is clean again."""
    set_env(monkeypatch, {})
    sy = system("poisson", (17, 9, 5))
    with E.EC3DSolver() as s:
        sy["build"](s)
        lay = s.vector_layout()
        z = zones_of(s, sy)
        s.solve(sy["b"], sy["x0"], 1e-10, 50)
        Z.assert_clean(s, z, "before the mark")
        at = s.device_vector("S")[0] + 8 * lay["n"]                 # row n of S: the first padding row
        Z.poke(at, [-0.0])
        with pytest.raises(AssertionError, match=r"S: rows n\.\.n_pad: 1 of 259 not zero bytes.*0x8000000000000000"):
            Z.assert_clean(s, z, "marked")
        Z.poke(at, [0.0])
        Z.assert_clean(s, z, "after the mark")
    with Z.adopted(E, sy["build"]) as a:
        z = zones_of(a.s, sy)
        Z.assert_clean(a, z, "before the mark")
        with a.torch.cuda.stream(a.stream):
            a.store[a.margin - 1] = 0.0                              # the last double of the lower margin
        with pytest.raises(AssertionError, match="lower margin: 1 doubles overwritten"):
            Z.assert_clean(a, z, "marked")
        with a.torch.cuda.stream(a.stream):
            a.store[a.margin + Z.NVEC * a.len - 1] = 1e-300          # the last double of AS's upper ghost
        with pytest.raises(AssertionError, match="AS: upper ghost: 1 of"):
            Z.assert_clean(a, z, "marked")


# ---- (f) ---------------------------------------------------------------------------------------------------------------
def test_the_lists_hold_what_they_are_meant_to():
    dims = {c[1] for c in ADOPTED.values() if c[0] == "poisson"}
    assert dims == {(3, 3, 3), (17, 9, 5), (128, 4, 5), (128, 4, 9), (256, 8, 9), (128, 12, 10)}
    assert 17 * 9 * 5 == 765 and Z.round_up(765, 512) - 765 == 259
    assert ADOPTED["poisson-128x4x9-patch"][2] == ADOPTED["poisson-256x8x9-patch"][2] == {"EC3D_PATCH": "1"}
    assert ADOPTED["bands-128x12x10"][3] == {"dictionary": False} and ADOPTED["poisson-128x12x10-linear"][2] == LINEAR
    assert {c[2].get("EC3D_KEEP") for c in ADOPTED.values() if c[2].get("EC3D_NT") == "1" and c[0] == "poisson"} == {"0", "43"}
    assert G.N0 == 1537 and Z.round_up(G.N0, 512) - G.N0 == 511
    csr = [c[1] for c in ADOPTED.values() if c[0] == "csr"]
    assert len(csr) == 2 and all(G.case(c)[3]["n"] == G.N0 for c in csr)
    assert any(G.case(c)[3]["tail_rows"] > 0 for c in csr)                       # one is no stencil
    ops = [c[1] for c in ADOPTED.values() if c[0] == "operator"]
    assert len(ops) == 2 and set(ops) <= set(R.OPERATORS)
    av = {k: c[2] for k, c in ADOPTED.items() if c[0] == "av"}
    for g in ("g2", "g3", "g8a"):
        for p in ("auto", "pitched"):
            assert av[f"{g}-{p}-linear"].get("EC3D_SAV_PATCH") == "0" and av[f"{g}-{p}-patch"].get("EC3D_SAV_PATCH") == "2"
            assert (av[f"{g}-{p}-linear"].get("EC3D_PITCH") == "2") == (p == "pitched")
        assert av[f"{g}-pitched-interleaved"]["EC3D_SAV_IL"] == "2"
    assert len(av) == 15
    grid = {k: c for k, c in ADOPTED.items() if c[0] == "avgrid"}
    assert set(grid) == {"grid-S3-pitched-interleaved"} and grid["grid-S3-pitched-interleaved"][1] == "S3"
    assert grid["grid-S3-pitched-interleaved"][2] == {**SAV_FORM["interleaved"], "EC3D_NBLK_SPMV": "8"}
    assert AGR.GRIDS["S3"]["dims"] == (40, 30, 33) and AGR.pitch_of("S3") == 1536 and AGR.GRIDS["S3"]["pitched"]
    assert {"spmv x0", "spmv b", "solve 1e-10", "S exit", "R exit", "itmax 4", "true_residual"} <= \
        {label for label, _ in calls(system("avgrid", "S3"), {"S": 0.0, "R": 0.0})}
    labels = [label for label, _ in calls(system("av", "g2"), {"S": 0.0, "R": 0.0})]
    assert labels[:2] == ["spmv x0", "spmv b"] and {"solve 1e-10", "S exit", "R exit", "itmax 0", "itmax 1", "itmax 4",
                                                    "iterate(1, 5) + iterate(6, 3)", "true_residual", "rhs_step moving=0",
                                                    "rhs_step moving=1", "post_update", "vtk_fields",
                                                    "domain_integrals"} <= set(labels)
    # (b)
    po = [c for c in OWNED.values() if c[0] == "poisson"]
    assert {c[1] for c in po} == {(256, 8, 9), (128, 12, 10)} and len(po) == 2 * 2 * 2 * 3 * 3
    assert all(c[2]["EC3D_FUSE23"] == c[2]["EC3D_FUSE51"] for c in po)
    assert {(c[2]["EC3D_FUSE23"], c[2]["EC3D_K4S"], c[2]["EC3D_XDEFER"], c[2].get("EC3D_XASYNC")) for c in po} == \
        set(itertools.product(("0", "2"), ("0", "2"), ("1", "3", "4"), (None, "2", "3")))
    assert {k for k, c in OWNED.items() if c[0] == "av"} == {f"{g}-{p}-patch-fused" for g in ("g2", "g3")
                                                             for p in ("auto", "pitched")}
    assert list(RING_STOPS) == list(range(9))
    # (c)
    assert {c[0] for c in GRID_SLABS.values()} == {(24, 24, 24), (128, 8, 30)}
    assert GRID_SLABS["24x24x24"][1] == {} and GRID_SLABS["128x8x30-three-launch"][1] == THREE_LAUNCH
    assert THREE_LAUNCH == {"EC3D_PATCH": "1", "EC3D_FUSE23": "2", "EC3D_FUSE51": "2", "EC3D_K4S": "2", "EC3D_XDEFER": "4"}
    assert (24 * 24 * 12) % 512 != 0          # a slab of the plain plan whose rows [n, n_pad) overlap the upper halo plane
    # (d), (e)
    assert set(BAD_SOLVE) == {"poisson-17x9x5", "csr-nb3", "g2-auto", "g2-pitched", "g8a-pitched",
                              "poisson-256x8x9-three-launch-xd4", "grid-S3-pitched-interleaved"}
    assert BAD_SOLVE["grid-S3-pitched-interleaved"] is ADOPTED["grid-S3-pitched-interleaved"]
    assert BAD_SOLVE["poisson-256x8x9-three-launch-xd4"][2]["EC3D_XDEFER"] == "4" and BAD_KINDS == ("nan", "overflow")
    assert set(routes(system("av", "g2"))) == {"solve", "upload + solve_resident", "rhs_step -> solve -> post_update"}
    assert [(c[0], c[1]) for c in NEW_MATRIX] == [("poisson", (256, 8, 9)), ("csr", "nb3"), ("av", "g2"),
                                                  ("poisson", (128, 4, 9)), ("poisson", (128, 4, 9))]
    assert NEW_MATRIX[2][2]["EC3D_PITCH"] == "2" and NEW_MATRIX[4][3] == {"nblk": 8}
