"""z-slabs of the A-V system with the cut swept across a conductor (tests/av_cut_sweep.py: one plate, every position
of a cut from four planes under it to four over it, two-plane slabs, ranks without a conducting cell), one slab per
rank, all on device 0.  tests/test_av_cut_sweep_host.py asserts on the host that the family holds every situation.

Every comparison is bit for bit; the one bound is 5 tol on the true residual of a converged solve.

1. the operator: EC3DMulti.spmv == oracle.spmv_csr on the oracle's matrix (src/EC3D.f90:465-1049), both storage forms,
   both plane pitches, and through set_matrix_csr where the library cuts the CSR triple;
2. the time loop through the in-library driver (ec3d_multi_post_update / _rhs_step / _vtk_fields) and, at world 4,
   through the staged driver of dist.py, against the numpy restatements;
3. EC3D_AV_SEND_EMPTY_U = 0 against 1: the same bits everywhere, and the U planes of a cut travel in a direction exactly
   when the two planes on the sending side hold a conducting cell;
4. solves against oracle.twin_solve_av_slabs, the multi-rank GPU-order twin: x, the iteration count and every slab's
   restart count, on plans 0, 2 and 5 -- the in-library driver and the staged driver (each against a twin made from its
   own handles);
5. the one-process-per-GPU driver over the loopback transport, against the one-process handle.

Slabs keep no residual history (hist_cap), so none is compared."""
import numpy as np
import pytest

import av_cut_sweep as CS
import fields_numpy as FN
import multidomain_numpy as MD
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORMS = (True, False)                   # EC3DMulti(structured=...): the structured form, and bands + tail
KNOBS = ("EC3D_SLAB_FSPLIT", "EC3D_SLAB_PLAN", "EC3D_NT", "EC3D_KEEP", "EC3D_FUSE23", "EC3D_FUSE51", "EC3D_PATCH", "EC3D_NBLK",
         "EC3D_NBLK_SPMV", "EC3D_VEC_DEPTH", "EC3D_XCD_MAP", "EC3D_ZMARCH", "EC3D_XDEFER", "EC3D_XD_OFF_DEPTH", "EC3D_XD_ON_DEPTH",
         "EC3D_K4S", "EC3D_SLAB_FUSE", "EC3D_SLAB_XDEFER", "EC3D_XASYNC", "EC3D_XASYNC_WGS", "EC3D_XASYNC_PRIO",
         "EC3D_AV_SEND_EMPTY_U")
ALL = list(CS.MEMBERS)
TWIN_CASES = [(k, 2) for k in CS.THIN_PLATE] + [(k, 3) for k in CS.THICK_PLATE] + [(k, 4) for k in CS.THIN_SLABS]
# (plan asked for, plane pitch)
SLOTS = ("BB", "RR_INIT", "D1", "SS", "D2", "D3", "RR", "RR0N")       # P_* of csrc/ec3d_internal.hpp: a rank's eight sums
COMBOS = [(2, "auto"), (2, "pitched"), (5, "pitched"), (0, "auto")]


def case_id(c):
    return f"{CS.key_id(c[0])}-w{c[1]}"


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def set_knobs(monkeypatch, pitch=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("EC3D_" + k, str(v))
    if pitch == "pitched":
        monkeypatch.setenv("EC3D_PITCH", "2")
    elif pitch == "auto":
        monkeypatch.delenv("EC3D_PITCH", raising=False)


_cache = {}


def args_of(key):
    if ("a", key) not in _cache:
        _cache["a", key] = CS.member(*key)
    return _cache["a", key]


def matrix_of(key):
    if ("m", key) not in _cache:
        _cache["m", key] = O.gen_sparse_matrix(*args_of(key))
    return _cache["m", key]


def with_situation(name, world=2, keys=CS.THIN_PLATE):
    """The first member of `keys` whose cut at `world` is in the situation `name`."""
    for k in keys:
        if name in CS.situations(CS.per_plane(args_of(k)[1]), k[0], world):
            return k
    raise AssertionError(name)


def in_air(world=2):
    """A thin-plate member whose cut at world 2 is further than two planes from the plate: the upper rank's extended slab
    holds no conducting cell (its compact U block has length 0)."""
    for k in CS.THIN_PLATE:
        s = CS.situations(CS.per_plane(args_of(k)[1]), k[0], world)
        if "rank's extended slab holds no conductor below" in s and not any(x.startswith("cut") for x in s):
            return k
    raise AssertionError("no member with the cut in air")


def state_of(key):
    """Random X, B and sources in air cells -- among them one on each of the two planes on each side of every cut of every
    world the member runs at -- and what the restatements make of them (as tests/test_gpu_generated_av.py's state_of)."""
    if ("s", key) in _cache:
        return _cache["s", key]
    geo, geoC, valPHYS, BND, delta, dt = args_of(key)
    m = matrix_of(key)
    sdz, sdy, sdx = geo.shape
    N = geo.size
    rng = np.random.Generator(np.random.PCG64(4000 + 100 * key[0] + 10 * key[1] + key[2]))
    X0, B0 = rng.standard_normal(m["n"]), rng.standard_normal(m["n"])
    flat = geoC.reshape(-1)
    near = sorted({p for w in CS.MEMBERS[key] for c in CS.cuts(sdz, w) for p in (c - 2, c - 1, c, c + 1)})
    cells = [p * sdx * sdy + (5 + p % 2) * sdx + (p % 2) for p in near]      # x = 0 or 1: beside the plate, in air
    air = np.setdiff1d(np.flatnonzero(flat == 0), cells)
    cells = np.concatenate([cells, rng.choice(air, 8, replace=False)]).astype(np.int64)
    assert np.all(flat[cells] == 0) and len(set(cells // (sdx * sdy))) >= len(near)
    idx = ((np.arange(len(cells)) % 3) * N + cells + 1).astype(np.int32)
    val = rng.standard_normal(len(idx))
    bp, xp = MD.post_update(geo, geoC, valPHYS, dt, geo.shape, B0, X0)
    rhs = {mv: MD.rhs_step(m["irow"], m["jcol"], m["valA"], geo, geoC, valPHYS, dt, geo.shape, bp, xp, idx, val, mv)
           for mv in (False, True)}
    st = dict(X0=X0, B0=B0, idx=idx, val=val, post=(bp, xp), rhs=rhs, fields=FN.fields(geoC, delta, xp, bp))
    _cache["s", key] = st
    return st


def same_fields(got, want):
    for k in ("A", "eddy", "source", "B"):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            assert np.asarray(got[k], np.float32).tobytes() == want[k].tobytes(), k


def joined(parts, big):
    assert all(v is None or all(a.dtype == np.dtype(">f4" if big else "<f4") for a in v) for v in parts.values())
    return {k: (None if v is None else np.concatenate(v).astype(np.float32)) for k, v in parts.items()}


def slabs_of(m):
    return [m.slab(r) for r in range(m.nranks)]


def restarts_of(m):
    return [m.slab(r)[0].restart_count() for r in range(m.nranks)]


def random_system(key, seed):
    m = matrix_of(key)
    rng = np.random.Generator(np.random.PCG64(seed))
    return m, rng.standard_normal(m["n"]), rng.standard_normal(m["n"])


# --------------------------------------------------------------------------------------------- 1. operator
@pytest.mark.parametrize("key", ALL, ids=CS.key_id)
def test_operator_equals_the_oracles(E, monkeypatch, plane_pitch, key):
    """A x over the slabs == the oracle's CSR row sums, at every world of the member: natively assembled in both storage
    forms ("auto": the kernels mask the rows outside the owned index ranges; "pitched": they sweep the owned tiles only),
    and cut out of the oracle's CSR triple wherever probe_csr_multi says the library cuts it."""
    set_knobs(monkeypatch)
    m = matrix_of(key)
    rng = np.random.Generator(np.random.PCG64(17))
    xs = [rng.standard_normal(m["n"]) for _ in range(2)]
    want = [O.spmv_csr(m["valA"], m["irow"], m["jcol"], x) for x in xs]
    for world in CS.MEMBERS[key]:
        for structured in FORMS:
            with E.EC3DMulti(world, devices=[0] * world, structured=structured) as mu:
                mu.assemble(*args_of(key))
                assert mu.n == m["n"]
                for x, y in zip(xs, want):
                    assert np.array_equal(mu.spmv(x), y), (world, structured)
        cuts_it, why = E.probe_csr_multi(m["valA"], m["irow"], m["jcol"], world)
        assert cuts_it, why                                   # (every member is a one-domain plate: all of them are cut)
        with E.EC3DMulti(world, devices=[0] * world) as mu:
            mu.set_matrix_csr(m["valA"], m["irow"], m["jcol"])
            assert mu.n == m["n"]
            for x, y in zip(xs, want):
                assert np.array_equal(mu.spmv(x), y), (world, "csr")


# -------------------------------------------------------------------------------- 2. time-loop vectors, fields
@pytest.mark.parametrize("key", ALL, ids=CS.key_id)
def test_time_loop_vectors_and_fields_in_the_library(E, monkeypatch, plane_pitch, key):
    """src/EC3D.f90:412-433 (post-update), :277-404 (right-hand side, static and moving sources) and the four point vectors
    of field_N.vtk on the slabs of the multi handle == the numpy restatements on the undivided system."""
    set_knobs(monkeypatch)
    geo, geoC, valPHYS, BND, delta, dt = args_of(key)
    st = state_of(key)
    bp, xp = st["post"]
    for world in CS.MEMBERS[key]:
        for structured in FORMS:
            with E.EC3DMulti(world, devices=[0] * world, structured=structured) as mu:
                mu.assemble(*args_of(key))
                mu.upload("B", st["B0"])
                mu.upload("X", st["X0"])
                mu.post_update()
                assert np.array_equal(mu.download("B"), bp) and np.array_equal(mu.download("X"), xp), (world, structured)
                same_fields(mu.vtk_fields(delta, geo.size, True), st["fields"])
                for big in (True, False):
                    parts = mu.vtk_fields_wait(mu.vtk_fields_begin(delta, big_endian=big), big_endian=big)
                    assert all(len(v) == world for v in parts.values())
                    same_fields(joined(parts, big), st["fields"])
                for moving in (False, True):
                    mu.upload("B", bp)
                    mu.upload("X", xp)
                    mu.rhs_step(st["idx"], st["val"], moving=moving)
                    assert np.array_equal(mu.download("B"), st["rhs"][moving]), (world, structured, moving)
                    assert np.array_equal(mu.download("X"), xp)


@pytest.mark.parametrize("key", ALL, ids=CS.key_id)
def test_time_loop_vectors_and_fields_on_the_staged_driver(E, monkeypatch, key):
    """The same through HipAVSlabOps / InProcessSlabs at world 4 (tests/test_gpu_generated_av.py runs worlds 2 and 3):
    four planes per rank on the 16-plane grid, two on the 8-plane one."""
    from eddy_currents_3d_amd.dist import HipAVSlabOps, InProcessSlabs, slab_bounds
    set_knobs(monkeypatch, pitch="auto")
    geo, geoC, valPHYS, BND, delta, dt = args_of(key)
    n = matrix_of(key)["n"]
    st = state_of(key)
    bp, xp = st["post"]
    world = 4
    for structured in FORMS:
        ops = []
        try:
            for r in range(world):
                k0, k1 = slab_bounds(geo.shape[0], r, world)
                ops.append(HipAVSlabOps(geo, geoC, valPHYS, BND, delta, dt, k0, k1, world, structured=structured))
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
                assert np.array_equal(drv.vector("B", n), st["rhs"][moving]), (structured, moving)
                assert np.array_equal(drv.vector("X", n), xp)
        finally:
            for o in ops:
                o.close()


@pytest.mark.parametrize("zi", CS.TWO_DOMAIN)
def test_slabs_still_refuse_a_plate_of_two_domains(E, monkeypatch, zi):
    """The plate split into two domains with the interface on the cut, one plane below and one above: the per-step
    kernels of a slab refuse several domains (tests/test_gpu_multidomain.py).  The day that is lifted this test fails:
    then give these members to every test of this file."""
    set_knobs(monkeypatch)
    args = CS.two_domain(zi)
    m = O.gen_sparse_matrix(*args)
    with E.EC3DMulti(2, devices=[0, 0]) as mu:
        mu.assemble(*args)
        mu.upload("B", np.zeros(m["n"]))
        mu.upload("X", np.zeros(m["n"]))
        with pytest.raises(E.EC3DError) as e:
            mu.rhs_step(np.zeros(0, np.int32), np.zeros(0))
        assert e.value.status == 5
        with pytest.raises(E.EC3DError) as e:
            mu.post_update()
        assert e.value.status == 5


# --------------------------------------------------------------------------------------- 3. the U-plane rule
def expected_halo_rows(per, sdz, world, kdz, send_empty):
    """[(sent, received)] per rank of the structured form: one plane of each A block per neighbour, and the two U planes
    next to the cut when they travel -- always, or (send_empty False) when the two planes on the sending side hold a
    conducting cell."""
    out = []
    for r in range(world):
        k0, k1 = CS.slab_bounds(sdz, r, world)
        sent = recv = 0
        if r > 0:
            sent += 3 * kdz + (2 * kdz if send_empty or per[k0:k0 + 2].sum() > 0 else 0)
            recv += 3 * kdz + (2 * kdz if send_empty or per[k0 - 2:k0].sum() > 0 else 0)
        if r < world - 1:
            sent += 3 * kdz + (2 * kdz if send_empty or per[k1 - 2:k1].sum() > 0 else 0)
            recv += 3 * kdz + (2 * kdz if send_empty or per[k1:k1 + 2].sum() > 0 else 0)
        out.append((sent, recv))
    return out


@pytest.mark.parametrize("plan", [2, 5])
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("key", CS.THIN_PLATE, ids=CS.key_id)
def test_empty_u_planes_stay_at_home_without_changing_a_bit(E, monkeypatch, key, world, plan):
    """EC3D_AV_SEND_EMPTY_U=0 claims that the ghost rows it no longer fills are exactly zero in every vector: A x, the
    per-step vectors and 24 iterations are the same bits as with every U plane sent, while the exchange shrinks exactly
    where the rule says."""
    geo, geoC, valPHYS, BND, delta, dt = args_of(key)
    sdz, kdz = geo.shape[0], geo.shape[1] * geo.shape[2]
    per = CS.per_plane(geoC)
    st = state_of(key)
    bp, xp = st["post"]
    m, b, x0 = random_system(key, 31)
    out = {}
    for send in ("1", "0"):
        set_knobs(monkeypatch, pitch="pitched" if plan == 5 else "auto", SLAB_PLAN=plan, AV_SEND_EMPTY_U=send)
        with E.EC3DMulti(world, devices=[0] * world, structured=True) as mu:
            mu.assemble(*args_of(key))
            assert mu.plan()[0] == plan
            rows = [mu.halo_rows(r) for r in range(world)]
            assert rows == expected_halo_rows(per, sdz, world, kdz, send == "1")
            assert sum(s for s, _ in rows) == sum(r for _, r in rows)
            got = [mu.spmv(x0)]
            mu.upload("B", st["B0"])
            mu.upload("X", st["X0"])
            mu.post_update()
            got += [mu.download("B"), mu.download("X")]
            for moving in (False, True):
                mu.upload("B", bp)
                mu.upload("X", xp)
                mu.rhs_step(st["idx"], st["val"], moving=moving)
                got.append(mu.download("B"))
            x, it = mu.solve(b, x0, 1e-30, 23)
            assert it == 24
            out[send] = got + [x]
    assert np.array_equal(out["1"][0], O.spmv_csr(m["valA"], m["irow"], m["jcol"], x0))
    assert len(out["0"]) == len(out["1"]) == 6
    for a, c in zip(out["0"], out["1"]):
        assert np.array_equal(a, c)


# ------------------------------------------------------------------------------------ 4. solves against the twin
@pytest.mark.parametrize("plan, pitch", COMBOS, ids=[f"plan{p}-{q}" for p, q in COMBOS])
@pytest.mark.parametrize("structured", FORMS, ids=["structured", "bands+tail"])
@pytest.mark.parametrize("case", TWIN_CASES, ids=case_id)
def test_24_iterations_equal_the_twin(E, monkeypatch, case, structured, plan, pitch):
    """24 iterations from a random b and x0 (tol 1e-30, itmax 23): x, the count and every slab's restart count are the
    multi-rank GPU-order twin's.  A slab too thin for a split launch runs the whole kernel inside the job's plan, and the
    twin follows what each view reports."""
    key, world = case
    set_knobs(monkeypatch, pitch=pitch, SLAB_PLAN=plan)
    m, b, x0 = random_system(key, 23)
    with E.EC3DMulti(world, devices=[0] * world, structured=structured) as mu:
        mu.assemble(*args_of(key))
        assert mu.plan()[0] == plan
        sl = slabs_of(mu)
        if plan == 5:   # K1 / K3 split where a slab of the structured form owns two boundary planes per cut and two more
            assert [v.can_overlap() for v, _, _ in sl] == [structured and k1 - k0 >= 6 for _, k0, k1 in sl]
        x, it = mu.solve(b, x0, 1e-30, 23)
        rs = restarts_of(mu)
        xt, itt, _, _, rst = O.twin_solve_av_slabs(sl, args_of(key)[1], plan, m["valA"], m["irow"], m["jcol"], b, x0, 1e-30, 23)
    assert it == itt == 24
    assert np.array_equal(x, xt)
    assert rs == [rst] * world


CONVERGED = [("cut one plane inside a face below", lambda: with_situation("cut one plane inside a face below")),   # the bottom face
             ("cut one plane inside a face above", lambda: with_situation("cut one plane inside a face above")),   # the top face
             ("cut in air", in_air)]


@pytest.mark.parametrize("plan, pitch", [(2, "auto"), (5, "pitched")], ids=["plan2-auto", "plan5-pitched"])
@pytest.mark.parametrize("structured", FORMS, ids=["structured", "bands+tail"])
@pytest.mark.parametrize("name, pick", CONVERGED, ids=[c[0].replace(" ", "-") for c in CONVERGED])
def test_converged_solves_equal_the_twin(E, monkeypatch, name, pick, structured, plan, pitch):
    """b = A x*, tol 1e-9, two slabs: both exits of src/solvers.f90:34 / :43 available; then a warm second solve from the
    result.  The true residual (computed on the device) is within 5 tol."""
    key, world, tol, itmax = pick(), 2, 1e-9, 5000
    set_knobs(monkeypatch, pitch=pitch, SLAB_PLAN=plan)
    m = matrix_of(key)
    xstar = np.random.Generator(np.random.PCG64(41)).standard_normal(m["n"])
    b = O.spmv_csr(m["valA"], m["irow"], m["jcol"], xstar)
    x0 = np.zeros(m["n"])
    with E.EC3DMulti(world, devices=[0] * world, structured=structured) as mu:
        mu.assemble(*args_of(key))
        assert mu.plan()[0] == plan
        sl = slabs_of(mu)
        x, it = mu.solve(b, x0, tol, itmax)
        rs = restarts_of(mu)
        rel, _ = mu.true_residual()
        x2, it2 = mu.solve(b, x, tol, itmax)
        rs2 = restarts_of(mu)
        tw = lambda start: O.twin_solve_av_slabs(sl, args_of(key)[1], plan, m["valA"], m["irow"], m["jcol"], b, start, tol, itmax)
        xt, itt, _, _, rst = tw(x0)
        xt2, itt2, _, _, rst2 = tw(xt)
    print(f"{name}, {CS.key_id(key)}: {it} iterations (twin {itt}), restarts {rs} (twin {rst}), true residual {rel:.2e}; "
          f"warm {it2} (twin {itt2})")
    assert it == itt <= itmax and np.array_equal(x, xt) and rs == [rst] * world
    assert rel < 5 * tol
    assert it2 == itt2 and np.array_equal(x2, xt2) and rs2 == [rst2] * world


@pytest.mark.parametrize("structured", FORMS, ids=["structured", "bands+tail"])
@pytest.mark.parametrize("key", CS.THIN_PLATE, ids=CS.key_id)
def test_staged_driver_equals_the_twin(E, monkeypatch, key, structured):
    """The staged driver of dist.py (HipAVSlabOps / InProcessSlabs, K2 / K5 boundary rows first: the order of plan 2) on two
    slabs against a twin made from ITS handles -- so the in-library driver and the staged one, which tests/test_gpu_multi.py
    holds to each other, are each held to the restatement."""
    from eddy_currents_3d_amd.dist import HipAVSlabOps, InProcessSlabs, slab_bounds
    set_knobs(monkeypatch, pitch="auto")
    world = 2
    geo, geoC, valPHYS, BND, delta, dt = args_of(key)
    m, b, x0 = random_system(key, 23)
    ops = []
    try:
        for r in range(world):
            k0, k1 = slab_bounds(geo.shape[0], r, world)
            ops.append(HipAVSlabOps(geo, geoC, valPHYS, BND, delta, dt, k0, k1, world, structured=structured))
            ops[-1].set_vector_global("B", b)
            ops[-1].set_vector_global("X", x0)
        drv = InProcessSlabs(ops, vsplit=True)
        it = drv.solve(1e-30, 23)
        x = drv.x(m["n"])
        rs = [o.local.restart_count() for o in ops]
        drv._sync()
        slots = [o.lsum.cpu().numpy().copy() for o in ops]
        sl = [(o.local, o.k0, o.k1) for o in ops]
        sums = {}
        xt, itt, _, _, rst = O.twin_solve_av_slabs(sl, geoC, 2, m["valA"], m["irow"], m["jcol"], b, x0, 1e-30, 23, sums=sums)
    finally:
        for o in ops:
            o.close()
    assert it == itt == 24
    assert np.array_equal(x, xt)
    assert rs == [rst] * world
    for q, name in enumerate(SLOTS):
        assert [float(s[q]) for s in slots] == sums[name], name


# ----------------------------------------------------------------------------------- 5. rank driver, loopback
@pytest.mark.parametrize("structured", FORMS, ids=["structured", "bands+tail"])
@pytest.mark.parametrize("name", ["cut one plane inside a face below", "cut one plane inside a face above"],
                         ids=["inside-bottom-face", "inside-top-face"])
def test_rank_job_over_loopback_equals_the_one_process_handle(E, monkeypatch, name, structured):
    """Two ranks of the one-process-per-GPU driver (ec3d_multi_create_rank) over the loopback transport, the cut one plane
    inside a face: A x and 24 iterations on plan 2 are the one-process handle's bits."""
    import test_gpu_rank_loopback as LB
    set_knobs(monkeypatch, pitch="auto")
    LB.set_knobs(monkeypatch, SLAB_PLAN=2)
    key, world = with_situation(name), 2
    m, b, x0 = random_system(key, 23)
    with E.EC3DMulti(world, devices=[0] * world, structured=structured) as one:
        one.assemble(*args_of(key))
        want_plan = one.plan()
        assert want_plan[0] == 2
        y_one = one.spmv(x0)
        x_one, it_one = one.solve(b, x0, 1e-30, 23)
        cuts = [one.slab(r)[1:] for r in range(world)]
    assert np.array_equal(y_one, O.spmv_csr(m["valA"], m["irow"], m["jcol"], x0))

    def body(mu, r):
        mu.assemble(*args_of(key))
        assert mu.n == m["n"] and mu.slab(0)[1:] == cuts[r] and mu.plan() == want_plan
        y = mu.spmv(x0)
        x, it = mu.solve(b, x0, 1e-30, 23)
        return x, it, y

    got = LB.run_ranks(E, world, body, structured=structured)
    assert [g[1] for g in got] == [it_one] * world == [24] * world
    assert np.array_equal(LB.merge(x0, [g[0] for g in got]), x_one)
    assert np.array_equal(LB.merge(np.zeros(m["n"]), [g[2] for g in got]), y_one)
