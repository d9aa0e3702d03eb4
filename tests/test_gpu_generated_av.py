"""A-V assembly and the per-step field kernels on generated geometries (tests/av_generate.py: 80 seeds of 0 .. 4
conducting domains, unions of boxes with holes, six independent boundary values, anisotropic spacing, per-domain
velocities; directed defects and near-face blocks) and on the captures g9a / g9b, against the oracle's assembly
(oracle.gen_sparse_matrix), the numpy restatements of the per-step vectors (tests/multidomain_numpy.py) and of the
field file's vectors (tests/fields_numpy.py), and the GPU-order twin of the solver; all of them pinned on the host by
tests/test_generated_av_host.py.  Every comparison is bit for bit unless it names the reference's x (10 tol).

Nothing is skipped or filtered inside a test: the lists below are made at import from the committed seed list by the
oracle alone, and tests/test_generated_av_host.py asserts how many of each kind they hold."""
import re

import numpy as np
import pytest

import av_generate as AG
import avmg_numpy as AV
import fields_numpy as FN
import multidomain_numpy as MD
from conftest import load_golden
from mg_numpy import hierarchy_dims
from oracle import oracle as O
from test_generated_av_host import DEFECT_CODES, G9, captured_field_files, model_of, oracle_code

pytestmark = pytest.mark.gpu

MEMBERS = {seed: AG.generate(seed) for seed in AG.CORPUS}
CODES = {seed: oracle_code(O, a) for seed, a in MEMBERS.items()}
ACCEPTED = [s for s in AG.CORPUS if CODES[s] == 0]
NDOM = {s: len(MD.conductors(MEMBERS[s][0], MEMBERS[s][1])) for s in ACCEPTED}
SCAN = {s: MD.structured_applies(MEMBERS[s][0], MEMBERS[s][1]) for s in ACCEPTED}
ONE_DOMAIN = [s for s in ACCEPTED if NDOM[s] == 1]
SOLVE = ([s for s in ACCEPTED if SCAN[s] and NDOM[s] == 1][:2] + [s for s in ACCEPTED if SCAN[s] and NDOM[s] > 1][:2] +
         [s for s in ACCEPTED if not SCAN[s]][:4])      # 4 in the structured form, 4 on bands + tail
BLOCK_MG = sorted((s for s in ACCEPTED if SCAN[s] and 1 <= NDOM[s] <= 4 and
                   hierarchy_dims(*MEMBERS[s][0].shape[::-1], MEMBERS[s][4])[2]),
                  key=lambda s: -MEMBERS[s][0].size)[:4]
FORMS = (True, False)                 # EC3DSolver(structured=...): the default, and bands + tail


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    return E


_cache = {}


def matrix_of(seed):
    if ("m", seed) not in _cache:
        _cache["m", seed] = O.gen_sparse_matrix(*MEMBERS[seed])
    return _cache["m", seed]


def state_of(seed):
    """Random X, B and sources in non-conducting cells, and what the restatements make of them: a dict with X0, B0,
    idx, val, post = (B, X) after post_update, and rhs[(moving, rule)] = B after rhs_step from the post-updated
    state."""
    if ("s", seed) in _cache:
        return _cache["s", seed]
    geo, geoC, valPHYS, BND, delta, dt = MEMBERS[seed]
    m = matrix_of(seed)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    N = geo.size
    X0, B0 = rng.standard_normal(m["n"]), rng.standard_normal(m["n"])
    doms = MD.conductors(geo, geoC)
    if doms:        # a state the reference's loop can be in: nothing ever writes the U rows of Jaf past max siznod,
        B0[3 * N + max(len(c) for _, c in doms):] = 0.0      # they keep their initial 0 (src/EC3D.f90:374-392)
    air = np.flatnonzero(geoC.reshape(-1) == 0)
    cells = rng.choice(air, min(12, len(air)), replace=False)
    idx = (rng.integers(0, 3, len(cells)) * N + cells + 1).astype(np.int32)
    val = rng.standard_normal(len(idx))
    bp, xp = MD.post_update(geo, geoC, valPHYS, dt, geo.shape, B0, X0)
    rhs = {}
    for rule in (("reference", "all") if NDOM[seed] > 1 else ("reference",)):
        for moving in (False, True):
            rhs[moving, rule] = MD.rhs_step(m["irow"], m["jcol"], m["valA"], geo, geoC, valPHYS, dt, geo.shape, bp, xp,
                                            idx, val, moving, rule=rule)
    st = dict(X0=X0, B0=B0, idx=idx, val=val, post=(bp, xp), rhs=rhs, fields=FN.fields(geoC, delta, xp, bp))
    _cache["s", seed] = st
    return st


def check_matrix(s, m, D, scan, structured):
    """The handle's operator against the oracle's: CSR, nnz, the six cel_bnd lists, three products; the storage form."""
    va, ir, jc = s.export_csr()
    assert np.array_equal(ir, m["irow"]) and np.array_equal(jc, m["jcol"]) and np.array_equal(va, m["valA"])
    mi = s.info
    assert mi.nnz == len(m["jcol"]) and mi.n == len(m["irow"]) - 1
    for got, want in zip(s.cel_bnd(), m["cel_bnd"]):
        assert np.array_equal(got, want)
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(3):
        x = rng.standard_normal(s.n)
        assert np.array_equal(s.spmv(x), O.spmv_csr(m["valA"], m["irow"], m["jcol"], x))
    if structured and scan:      # (no conductor: the 9 coupled classes of one unused domain are still there)
        assert mi.tail_rows == 0 and mi.dict_classes == 55 + 9 * max(D, 1)
    elif D:
        assert mi.tail_rows > 0


def same_fields(got, want):
    for key in ("A", "eddy", "source", "B"):
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            assert np.asarray(got[key], np.float32).tobytes() == want[key].tobytes(), key


def captured_matrix(g):
    m = O.gen_sparse_matrix(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"]))
    assert np.array_equal(m["valA"], g["valA"]) and np.array_equal(m["jcol"], g["jcol"])
    return m


def args_of(g):
    return g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], g["BND"], g["delta"], float(g["dt"])


# ---------------------------------------------------------------------------------------------- verdict
@pytest.mark.parametrize("seed", AG.CORPUS)
def test_device_assembles_exactly_what_the_oracle_assembles(E, seed):
    """Both storage forms.  A refused member may hold several defects: the device keeps the largest code any cell
    raises, the reference stops at the first defect in scan order, so the two codes need not be equal -- only the
    refusal is required, with one of the reference's three codes."""
    for structured in FORMS:
        with E.EC3DSolver(structured=structured) as s:
            if CODES[seed] == 0:
                s.assemble(*MEMBERS[seed])
                assert s.n == matrix_of(seed)["n"]
            else:
                with pytest.raises(E.EC3DError) as err:
                    s.assemble(*MEMBERS[seed])
                assert err.value.status in (1, 2, 3)


@pytest.mark.parametrize("kind", AG.DEFECTS)
def test_single_defect_is_refused_with_the_oracles_code(E, kind):
    """One defect: the device's code is the oracle's.  The refused handle then assembles a legal geometry correctly."""
    legal = AG.near_face("y", "p")
    m = O.gen_sparse_matrix(*legal)
    for structured in FORMS:
        with E.EC3DSolver(structured=structured) as s:
            with pytest.raises(E.EC3DError) as err:
                s.assemble(*AG.single_defect(kind))
            assert err.value.status == DEFECT_CODES[kind] == oracle_code(O, AG.single_defect(kind))
            s.assemble(*legal)
            check_matrix(s, m, 1, True, structured)


# ----------------------------------------------------------------------------------------------- matrix
@pytest.mark.parametrize("seed", ACCEPTED)
def test_matrix_equals_the_oracles(E, plane_pitch, seed):
    for structured in FORMS:
        with E.EC3DSolver(structured=structured) as s:
            s.assemble(*MEMBERS[seed])
            check_matrix(s, matrix_of(seed), NDOM[seed], SCAN[seed], structured)


@pytest.mark.parametrize("side", "mp")
@pytest.mark.parametrize("axis", "xyz")
def test_near_face_matrix_equals_the_oracles(E, plane_pitch, axis, side):
    args = AG.near_face(axis, side)
    m = O.gen_sparse_matrix(*args)
    for structured in FORMS:
        with E.EC3DSolver(structured=structured) as s:
            s.assemble(*args)
            check_matrix(s, m, 1, True, structured)


@pytest.mark.parametrize("case", sorted(G9))
def test_captured_matrix(E, plane_pitch, case):
    g = load_golden(G9[case])
    m = captured_matrix(g)
    for structured in FORMS:
        with E.EC3DSolver(structured=structured) as s:
            s.assemble(*args_of(g))
            check_matrix(s, m, 2 if case == "g9a" else 1, True, structured)


# ------------------------------------------------------------------------------------- per-step vectors
@pytest.mark.parametrize("seed", ACCEPTED)
def test_step_vectors_and_fields_equal_the_restatements(E, plane_pitch, seed):
    """post_update, rhs_step (static and moving sources, both U-row rules where there are several domains) and the
    field vectors after the post-update -- ec3d_vtk_fields and the begin / wait path in both byte orders."""
    geo, geoC, valPHYS, BND, delta, dt = MEMBERS[seed]
    st = state_of(seed)
    bp, xp = st["post"]
    N = geo.size
    for structured in FORMS:
        with E.EC3DSolver(structured=structured) as s:
            s.assemble(*MEMBERS[seed])
            s.upload("B", st["B0"])
            s.upload("X", st["X0"])
            s.post_update()
            assert np.array_equal(s.download("B"), bp) and np.array_equal(s.download("X"), xp)
            same_fields(s.vtk_fields(delta, N, NDOM[seed] > 0), st["fields"])
            for big in (True, False):
                f = s.vtk_fields_wait(s.vtk_fields_begin(delta, big_endian=big), big_endian=big)
                assert all(v is None or v.dtype == np.dtype(">f4" if big else "<f4") for v in f.values())
                same_fields({k: (None if v is None else v.astype(np.float32)) for k, v in f.items()}, st["fields"])
            for (moving, rule), want in st["rhs"].items():
                s.set_u_rhs(rule)
                s.upload("B", bp)
                s.upload("X", xp)
                s.rhs_step(st["idx"], st["val"], moving=moving)
                assert np.array_equal(s.download("B"), want), (moving, rule)
                assert np.array_equal(s.download("X"), xp)


@pytest.mark.parametrize("case", sorted(G9))
def test_every_captured_step(E, oracle, plane_pitch, case):
    """As test_gpu_multidomain.test_every_captured_step does for g8: from the captured previous step the device's
    post_update and rhs_step give the captured x_in and b bit for bit, the solve equals the GPU-order twin bit for
    bit, takes the reference's iteration count and lands within 10 tol of its x; the last field file the reference
    wrote is reproduced byte for byte from its step's state."""
    from eddy_currents_3d_amd import host, vxc
    from eddy_currents_3d_amd.vtk import field_vtk_bytes
    g = load_golden(G9[case])
    tol, itmax = float(g["tol"]), int(g["itmax"])
    model = model_of(g)
    prog = host.SourceProgram(model, vxc.domain_tables(model))
    sdz, sdy, sdx = g["vox"].shape
    dt = float(g["dt"])
    files = dict(captured_field_files(g))
    T = 0.0
    with E.EC3DSolver() as s:
        s.assemble(*args_of(g))
        n = s.n
        s.upload("B", np.zeros(n))
        s.upload("X", np.zeros(n))
        for k in range(len(g["iters"])):
            idx, val, moving = prog.step(T)
            s.rhs_step(idx, val, moving=moving)
            b = s.download("B")
            assert np.array_equal(b, g[f"b{k}"]), f"step {k}"
            x0 = s.download("X")
            assert np.array_equal(x0, g[f"xin{k}"]), f"step {k}"
            it, _ = s.solve_resident(tol, itmax)
            x = s.download("X")
            xt, itt, _, _ = oracle.twin_solve(s, g["valA"], g["irow"], g["jcol"], b, x0, tol, itmax)
            xr = g[f"xout{k}"]
            print(f"{case} step {k}: {it} iterations; x vs the reference's "
                  f"{np.linalg.norm(x - xr) / np.linalg.norm(xr):.2e}")
            assert it == itt == int(g["iters"][k]) and np.array_equal(x, xt), f"step {k}"
            assert np.linalg.norm(x - xr) <= 10 * tol * np.linalg.norm(xr)
            s.upload("B", g[f"b{k}"])           # the reference's own state from here on
            s.upload("X", xr)
            s.post_update()
            bp, xp = MD.post_update(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, g["vox"].shape, g[f"b{k}"], xr)
            assert np.array_equal(s.download("B"), bp) and np.array_equal(s.download("X"), xp)
            if k in files:
                f = s.vtk_fields(g["delta"], sdx * sdy * sdz, True)
                assert field_vtk_bytes(sdx, sdy, sdz, g["delta"], f) == files[k]
                f = s.vtk_fields_wait(s.vtk_fields_begin(g["delta"]))
                assert field_vtk_bytes(sdx, sdy, sdz, g["delta"], f) == files[k]
            T = T + dt
        assert files


# ------------------------------------------------------------------------------------------------ slabs
def _slab_case(key):
    if key == "g9b":
        g = load_golden(G9["g9b"])
        args = args_of(g)
        m = captured_matrix(g)
    else:
        args, m = MEMBERS[key], matrix_of(key)
    return args, m


def _slab_state(key, args, m):
    if key != "g9b":
        st = state_of(key)
        return st
    if ("s", key) in _cache:
        return _cache["s", key]
    geo, geoC, valPHYS, BND, delta, dt = args
    rng = np.random.Generator(np.random.PCG64(99))
    X0, B0 = rng.standard_normal(m["n"]), rng.standard_normal(m["n"])
    air = np.flatnonzero(geoC.reshape(-1) == 0)
    cells = rng.choice(air, 12, replace=False)
    idx = (rng.integers(0, 3, 12) * geo.size + cells + 1).astype(np.int32)
    val = rng.standard_normal(12)
    bp, xp = MD.post_update(geo, geoC, valPHYS, dt, geo.shape, B0, X0)
    rhs = {(mv, "reference"): MD.rhs_step(m["irow"], m["jcol"], m["valA"], geo, geoC, valPHYS, dt, geo.shape, bp, xp,
                                          idx, val, mv) for mv in (False, True)}
    _cache["s", key] = dict(X0=X0, B0=B0, idx=idx, val=val, post=(bp, xp), rhs=rhs,
                            fields=FN.fields(geoC, delta, xp, bp))
    return _cache["s", key]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("key", ONE_DOMAIN + ["g9b"])
def test_slabs_equal_the_undivided_results(E, key, world):
    """z-slabs of a one-domain model, all on this GPU, structured and not: the slabs' SpMV gives the rows of the global
    operator (EC3DMulti.spmv), and post_update, rhs_step and vtk_fields on HipAVSlabOps / InProcessSlabs give what
    the undivided handle gives -- the restatements' vectors, which test_step_vectors_and_fields_equal_the_restatements
    holds the undivided handle to."""
    from eddy_currents_3d_amd.dist import HipAVSlabOps, InProcessSlabs, slab_bounds
    args, m = _slab_case(key)
    st = _slab_state(key, args, m)
    geo, geoC, valPHYS, BND, delta, dt = args
    sdz = geo.shape[0]
    n = m["n"]
    bp, xp = st["post"]
    rng = np.random.Generator(np.random.PCG64(17))
    for structured in FORMS:
        with E.EC3DMulti(world, devices=[0] * world, structured=structured) as mu:
            mu.assemble(*args)
            assert mu.n == n
            for _ in range(2):
                x = rng.standard_normal(n)
                assert np.array_equal(mu.spmv(x), O.spmv_csr(m["valA"], m["irow"], m["jcol"], x))
        ops = []
        try:
            for r in range(world):
                k0, k1 = slab_bounds(sdz, r, world)
                ops.append(HipAVSlabOps(geo, geoC, valPHYS, BND, delta, dt, k0, k1, world, structured=structured))
                assert ops[-1].structured == structured
            drv = InProcessSlabs(ops)
            for o in ops:
                o.set_vector_global("B", st["B0"])
                o.set_vector_global("X", st["X0"])
            drv.post_update()
            assert np.array_equal(drv.vector("B", n), bp) and np.array_equal(drv.vector("X", n), xp)
            same_fields(drv.vtk_fields(delta, True), st["fields"])
            for moving in (False, True):
                for o in ops:
                    o.set_vector_global("B", bp)
                    o.set_vector_global("X", xp)
                drv.rhs_step(st["idx"], st["val"], moving=moving)
                assert np.array_equal(drv.vector("B", n), st["rhs"][moving, "reference"]), moving
        finally:
            for o in ops:
                o.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("structured", FORMS)
def test_multi_solves_g9b_in_the_references_iteration_counts(E, world, structured):
    g = load_golden(G9["g9b"])
    tol, itmax = float(g["tol"]), int(g["itmax"])
    with E.EC3DMulti(world, devices=[0] * world, structured=structured) as mu:
        mu.assemble(*args_of(g))
        for k in range(len(g["iters"])):
            x, it = mu.solve(g[f"b{k}"], g[f"xin{k}"], tol, itmax)
            xr = g[f"xout{k}"]
            print(f"g9b in {world} slabs, step {k}: {it} iterations, reference {int(g['iters'][k])}; x vs the "
                  f"reference's {np.linalg.norm(x - xr) / np.linalg.norm(xr):.2e}")
            assert it == int(g["iters"][k])
            assert np.linalg.norm(x - xr) <= 10 * tol * np.linalg.norm(xr)


# ------------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("key", sorted(G9) + SOLVE)
def test_twelve_iterations_equal_the_twin(E, oracle, sav_tiles, plane_pitch, key):
    """12 iterations from a random right-hand side (tol = 1e-30, itmax = 11): x, the iteration count and the residual
    history equal the GPU-order twin's bit for bit, under every tile shape of the structured kernels and both
    pitches.  g9a and g9b also run their captured steps: the reference's iteration count, x within 10 tol."""
    if key in G9:
        g = load_golden(G9[key])
        args, m = args_of(g), captured_matrix(g)
    else:
        g, args, m = None, MEMBERS[key], matrix_of(key)
    b = np.random.Generator(np.random.PCG64(23)).standard_normal(m["n"])
    with E.EC3DSolver() as s:
        s.assemble(*args)
        x, it, hist = s.solve(b, np.zeros(m["n"]), 1e-30, 11, hist_cap=16)
        xt, itt, hs, hr = oracle.twin_solve(s, m["valA"], m["irow"], m["jcol"], b, np.zeros(m["n"]), 1e-30, 11,
                                            hist_cap=16)
        assert it == itt == 12 and np.array_equal(x, xt)
        assert np.array_equal(hist[:, 0], hs, equal_nan=True) and np.array_equal(hist[:, 1], hr, equal_nan=True)
        if g is not None:
            tol, itmax = float(g["tol"]), int(g["itmax"])
            for k in range(len(g["iters"])):
                x, it, _ = s.solve(g[f"b{k}"], g[f"xin{k}"], tol, itmax)
                xr = g[f"xout{k}"]
                assert it == int(g["iters"][k])
                assert np.linalg.norm(x - xr) <= 10 * tol * np.linalg.norm(xr)


# ------------------------------------------------------------------------------------- block multigrid
@pytest.mark.timeout(600)
@pytest.mark.parametrize("key", sorted(G9) + BLOCK_MG)
def test_block_mg_equals_its_twin(E, key):
    args = args_of(load_golden(G9[key])) if key in G9 else MEMBERS[key]
    sdz, sdy, sdx = args[0].shape
    rng = np.random.Generator(np.random.PCG64(3))
    with E.EC3DSolver() as s:
        s.assemble(*args)
        s.set_preconditioner("block-mg")
        twin = AV.AVMG.from_solver(s, (sdx, sdy, sdz))
        for _ in range(2):
            r = rng.standard_normal(s.n)
            assert np.array_equal(s.precond_apply(r), twin.apply(r))


def test_the_lists_hold_what_the_issue_asks():
    assert len(SOLVE) == 8 and len(BLOCK_MG) == 4 and len(ONE_DOMAIN) >= 5
    assert re.fullmatch(r"g9b_.*", G9["g9b"])
