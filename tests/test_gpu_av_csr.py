"""The CSR route of the structured A-V kernels -- ec3d_set_matrix_csr / sprsbcgstabwr_ through the recogniser
(csrc/ec3d_sav_csr.cpp) -- on the corpus of tests/av_csr_generate.py: the reference's matrices of 0 .. 4 conducting
domains, one-edit mutations of them, and "saturated" matrices that fill every slot the recogniser admits (wrap slots,
all five U slots of an A row, all nine A slots of a U row, conductors on box faces and in the first and last plane),
which ec3d_assemble never builds.  tests/test_av_csr_host.py pins the corpus and the recogniser's decisions on the host.

Every comparison is bit for bit -- A*x against the oracle's CSR row sums (src/solvers.f90:54-61), twelve iterations
against the GPU-order twin -- except the slabs' x, held to the 1e-12 of tests/test_gpu_multi.py (slab dot products sum
in another order).  Vectors are finite: the structured kernels skip coupling slots whose coefficient is 0.0.

Nothing is skipped or filtered inside a test: the parameter lists are made at import from the corpus, and
test_every_form_ran_on_every_family asserts what they hold."""
import numpy as np
import pytest

import av_csr_generate as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILE = 512
CORPUS = G.corpus(O)
BY_NAME = {m.name: m for m in CORPUS}
KNOBS = ("EC3D_PITCH", "EC3D_SAV_PATCH", "EC3D_SAV_PATCH_PX", "EC3D_SAV_IL", "EC3D_FUSE23", "EC3D_FUSE51", "EC3D_NT",
         "EC3D_KEEP", "EC3D_NBLK", "EC3D_NBLK_SPMV", "EC3D_NBLK_SPMV_PLAIN", "EC3D_ZMARCH")
# form: the knobs that force it (tests/test_gpu_parity.py, tests/test_gpu_interleaved.py)
FORMS = {
    "linear": {},
    "z-march": {"EC3D_PITCH": "2", "EC3D_SAV_PATCH": "0"},
    "2-D tiles": {"EC3D_PITCH": "2", "EC3D_SAV_PATCH": "2"},
    "2-D tiles fused": {"EC3D_PITCH": "2", "EC3D_SAV_PATCH": "2", "EC3D_FUSE23": "2", "EC3D_FUSE51": "2"},
    "interleaved": {"EC3D_PITCH": "2", "EC3D_SAV_PATCH": "0", "EC3D_SAV_IL": "2"},
}
NBLK = (None, 3, 40)
NT = ("0", "1")


def aligned(m):
    """Does the library align this member's planes to tiles by itself?  (ec3d_ctx::pitch: then the default form is a
    z-march, not linear tiles.)"""
    sdx, sdy, sdz = m.dims
    plane = sdx * sdy
    return (-(-plane // TILE) * TILE - plane) * 16 <= plane and sdz >= 8


def _form_members(form):
    """Members a form runs on: recognised under the form's pitch, with a conductor (the interleaved march shows in the
    U tiles), an even sdx where the form is 2-D tiles (ec3d_pick_patch_shape), the smallest first."""
    pitched = form != "linear"
    tiles2d = form.startswith("2-D")
    ok = [m for m in CORPUS if m.expect[pitched] and m.n_cond > 0 and not (tiles2d and m.dims[0] % 2) and
          (pitched or not aligned(m))]
    gen = sorted((m for m in ok if m.family == "generated" and not m.name.startswith("near")), key=lambda m: m.n)
    pick = [m for m in gen if m.D == 1][:2] + [m for m in gen if m.D >= 2][:2] + [m for m in gen if m.D >= 3][:1]
    pick += [m for m in ok if m.family == "mutated"]
    pick += [m for m in ok if m.family == "saturated"]
    return list(dict.fromkeys(m.name for m in pick))


FORM_CASES = [(form, name) for form in FORMS for name in _form_members(form)]
GEN2 = sorted((m for m in CORPUS if m.family == "generated" and m.expect[0] and m.D >= 2), key=lambda m: m.n)
SLAB_CASES = [GEN2[1].name, GEN2[3].name, "sat_odd_two_boxes_11x9x10_none"]       # seed30, seed49: see the test
REFUSED = "sat_interior_12x10x9_all"


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


@pytest.fixture
def knobs(monkeypatch):
    """set(form, nblk, nt): the environment of one launch form, everything else unset."""
    def set_(form="linear", nblk=None, nt=None, pitch=None):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in FORMS[form].items():
            monkeypatch.setenv(k, v)
        if pitch == "pitched":
            monkeypatch.setenv("EC3D_PITCH", "2")
        if nblk is not None:
            monkeypatch.setenv("EC3D_NBLK_SPMV", str(nblk))
            if form == "linear":                   # (without a z-march the SpMV kernels take their grid from this one)
                monkeypatch.setenv("EC3D_NBLK_SPMV_PLAIN", str(nblk))
        if nt is not None:
            monkeypatch.setenv("EC3D_NT", nt)
    return set_


_want = {}


def product(m, key, x):
    """oracle.spmv_csr, computed once per (member, vector)."""
    if (m.name, key) not in _want:
        _want[m.name, key] = O.spmv_csr(m.valA, m.irow, m.jcol, x)
    return _want[m.name, key]


def vectors(m):
    """(key, x): a standard normal vector and one whose entries span 1e-100 .. 1e+100."""
    rng = np.random.Generator(np.random.PCG64(11))
    x = rng.standard_normal(m.n)
    return [("normal", x), ("wide", rng.standard_normal(m.n) * 10.0 ** rng.uniform(-100.0, 100.0, m.n))]


def without_zeros(m):
    """The member's CSR with the explicitly stored zeros removed, stored order kept."""
    keep = m.valA != 0.0
    r, _ = G._rows(m.irow, m.jcol)
    irow = np.concatenate([[1], 1 + np.cumsum(np.bincount(r[keep], minlength=m.n))]).astype(np.int32)
    return m.valA[keep], irow, m.jcol[keep]


def unit_rows(m, rm):
    """Rows whose unit vectors are multiplied: the first and the last, both sides of every block boundary, both sides of
    the first and the last tile edge in the device numbering `rm` (ec3d_get_row_map)."""
    nC = int(np.prod(m.dims))
    rows = {0, m.n - 1}
    for b in (nC, 2 * nC, 3 * nC):
        rows |= {b - 1, min(b, m.n - 1)}
    for rem in (TILE - 1, 0):
        at = np.flatnonzero((rm % TILE == rem) & (rm >= TILE - 1))
        if len(at):
            rows |= {int(at[0]), int(at[-1])}
    return sorted(rows)


# ------------------------------------------------------------------------------------- storage and product
@pytest.mark.parametrize("name", list(BY_NAME))
def test_stored_as_probed_and_multiplies_like_the_oracle(E, knobs, plane_pitch, name):
    """ec3d_set_matrix_csr stores what ec3d_probe_csr said -- the structured form with the probe's classes, or bands +
    tail -- and either way ec3d_export_csr gives the input back without the zeros it stored (neither form holds them),
    and A*x is the oracle's for a normal vector, a vector spanning 200 decades and unit vectors at the rows where a
    kernel changes block or tile."""
    m = BY_NAME[name]
    knobs(pitch=plane_pitch)
    p = E.probe_csr(*m.csr)
    assert bool(p.structured) == m.expect[plane_pitch == "pitched"]
    with E.EC3DSolver() as s:
        s.set_matrix_csr(*m.csr)
        mi = s.info
        assert mi.n == m.n and mi.nnz == len(m.valA)
        if p.structured:
            assert mi.tail_rows == 0 and mi.dict_classes == p.classes
            assert len(s.ulist()) > 0 or m.n_cond == 0
        else:
            assert mi.tail_rows > 0                             # (every refused member has a conductor)
        rm = s.row_map().astype(np.int64)
        assert np.all(np.diff(rm) > 0) and (p.structured or np.array_equal(rm, np.arange(m.n)))
        va, ir, jc = s.export_csr()
        wa, wi, wj = without_zeros(m)
        assert np.array_equal(ir, wi) and np.array_equal(jc, wj) and va.tobytes() == wa.tobytes()
        for key, x in vectors(m):
            assert np.array_equal(s.spmv(x), product(m, key, x)), key
        for r in unit_rows(m, rm):
            e = np.zeros(m.n)
            e[r] = 1.0
            assert np.array_equal(s.spmv(e), O.spmv_csr(m.valA, m.irow, m.jcol, e)), r


# --------------------------------------------------------------------------------------- every launch form
def check_form(s, form, m):
    """From the handle's own account: which form the SpMV kernels run in."""
    sdx, sdy, sdz = m.dims
    tpp = -(-sdx * sdy // TILE)
    g = s.geometry(1)
    ul = s.ulist()
    assert s.info.tail_rows == 0 and (len(ul) > 0 or form.startswith("2-D"))
    if form == "linear":
        assert g.zm_tpp == 0 and g.patch_x == 0 and g.ulist_n == len(ul) and s.fusion() == (0, 0)
    elif form == "z-march":
        assert g.zm_tpp == tpp and g.patch_x == 0 and g.ulist_n == len(ul) and s.fusion() == (0, 0)
    elif form == "interleaved":
        assert g.zm_tpp == tpp and g.patch_x == 0 and g.ulist_n == 0 and s.fusion() == (0, 0)
        off, tiles = s.visit_order(1)
        assert np.array_equal(np.sort(tiles), np.sort(np.concatenate([np.arange(g.ntiles_front), ul])))
    else:
        assert g.patch_x > 0 and g.patch_y == TILE // g.patch_x and g.patch_sdx == sdx and g.patch_sdy == sdy
        assert g.zm_tpp == (sdx // g.patch_x) * -(-sdy // g.patch_y)
        assert s.fusion() == ((1, 1) if form == "2-D tiles fused" else (0, 0))


@pytest.mark.parametrize("form,name", FORM_CASES)
def test_every_form_multiplies_and_iterates_like_the_twin(E, oracle, knobs, form, name):
    """Under the form's knobs, with 3, 40 and the library's own count of workgroups and both cache policies: the handle
    says the form ran, A*x is the oracle's, and twelve iterations (tol 1e-30, itmax 11, b = standard_normal(PCG64(23)),
    x0 = 0) give the twin's x, iteration count and both history columns."""
    m = BY_NAME[name]
    (key, x), _ = vectors(m)
    b = np.random.Generator(np.random.PCG64(23)).standard_normal(m.n)
    for nblk in NBLK:
        for nt in NT:
            knobs(form, nblk, nt)
            with E.EC3DSolver() as s:
                s.set_matrix_csr(*m.csr)
                check_form(s, form, m)
                assert np.array_equal(s.spmv(x), product(m, key, x)), (nblk, nt)
                xs, it, hist = s.solve(b, np.zeros(m.n), 1e-30, 11, hist_cap=16)
                xt, itt, hs, hr = oracle.twin_solve(s, m.valA, m.irow, m.jcol, b, np.zeros(m.n), 1e-30, 11, hist_cap=16)
                assert it == itt == 12 and np.array_equal(xs, xt), (nblk, nt)
                assert np.array_equal(hist[:, 0], hs, equal_nan=True) and np.array_equal(hist[:, 1], hr, equal_nan=True)
                if m.family == "saturated":
                    assert np.all(np.isfinite(xs))


def test_every_form_ran_on_every_family():
    for form in FORMS:
        ms = [BY_NAME[n] for f, n in FORM_CASES if f == form]
        gen = [m for m in ms if m.family == "generated"]
        mut = [m for m in ms if m.family == "mutated"]
        sat = [m for m in ms if m.family == "saturated"]
        assert len(gen) >= 4 and sum(m.D >= 2 for m in gen) >= 2, form
        assert len(mut) >= 2 and any(m.mutation == "wrap_x" for m in mut), form
        assert len(sat) >= 2 and any(m.wrap == "x" for m in sat), form
        assert any(m.extra["boxes"][0][0] == (0, m.dims[0]) for m in sat), form      # a conductor on the x faces
        print(f"{form}: {len(gen)} generated, {len(mut)} mutated, {len(sat)} saturated")
    assert any(BY_NAME[n].wrap == "all" for f, n in FORM_CASES if f == "linear")
    assert any(BY_NAME[n].mutation == "wrap_plane" for f, n in FORM_CASES if f == "linear")
    assert [BY_NAME[n].D >= 2 for n in SLAB_CASES] == [True, True, True] and BY_NAME[SLAB_CASES[2]].wrap == "none"


# --------------------------------------------------------------------------------------------------- slabs
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", SLAB_CASES)
def test_slabs_multiply_and_solve_like_the_undivided_handle(E, knobs, plane_pitch, name, world):
    """z-slabs cut out of the recognised form (ec3d_sav_slice), all on this GPU: A*x is the oracle's bit for bit; the
    solve takes the undivided handle's iteration count and gives its x to 1e-12.  The saturated member is solved to
    1e-10 (nine iterations on the host).  On the reference's matrices a random right-hand side does not converge (the
    oracle's solver runs to itmax on the host), so they take this file's twelve iterations, from two members whose x
    moved by less than 1e-13 on the host when every sum was reordered by a random permutation of the unknowns."""
    m = BY_NAME[name]
    knobs(pitch=plane_pitch)
    assert E.probe_csr_multi(*m.csr, world)[0]
    b = np.random.Generator(np.random.PCG64(23)).standard_normal(m.n)
    tol, itmax = (1e-10, 100) if m.family == "saturated" else (1e-30, 11)
    with E.EC3DSolver() as s:
        s.set_matrix_csr(*m.csr)
        x1, it1, _ = s.solve(b, np.zeros(m.n), tol, itmax)
    with E.EC3DMulti(world, devices=[0] * world) as mu:
        mu.set_matrix_csr(*m.csr)
        assert mu.n == m.n
        for key, x in vectors(m):
            assert np.array_equal(mu.spmv(x), product(m, key, x)), key
        xs, its = mu.solve(b, np.zeros(m.n), tol, itmax)
    rel = np.linalg.norm(xs - x1) / np.linalg.norm(x1)
    print(f"{name} in {world} slabs: {its} iterations (undivided {it1}), x differs by {rel:.2e}")
    assert its == it1 and (it1 == 12 or 1 < it1 < 100)
    assert rel <= 1e-12


def test_a_system_without_conductor_is_cut_as_one_operator(E, knobs, oracle):
    """Seven planes cannot give four A-V slabs of two planes; without a conductor the matrix is one 7-point operator on
    21 planes, and that is what the library cuts (tests/test_av_csr_host.py states the rule)."""
    m = next(m for m in CORPUS if m.family == "generated" and m.n_cond == 0 and m.dims[2] == 7)
    knobs()
    assert E.probe_csr(*m.csr).structured and E.probe_csr_multi(*m.csr, 4)[0]
    with E.EC3DMulti(4, devices=[0] * 4) as mu:
        mu.set_matrix_csr(*m.csr)
        for key, x in vectors(m):
            assert np.array_equal(mu.spmv(x), product(m, key, x)), key


def test_coupling_across_z_faces_is_refused_and_the_handle_lives_on(E, knobs):
    bad, good = BY_NAME[REFUSED], BY_NAME["sat_interior_12x10x9_none"]
    knobs()
    assert not E.probe_csr_multi(*bad.csr, 2)[0]
    with E.EC3DMulti(2, devices=[0, 0]) as mu:
        with pytest.raises(E.EC3DError, match="couples across"):
            mu.set_matrix_csr(*bad.csr)
        mu.set_matrix_csr(*good.csr)
        (key, x), _ = vectors(good)
        assert np.array_equal(mu.spmv(x), product(good, key, x))


# ------------------------------------------------------------------------------------------------- drop-in
@pytest.mark.parametrize("name", [GEN2[0].name, "sat_fills_xy_16x8x10_x"])
def test_drop_in_symbol_equals_the_handle(E, knobs, name):
    """sprsbcgstabwr_ itself: x and the iteration count of ec3d_set_matrix_csr + ec3d_solve, bit for bit."""
    m = BY_NAME[name]
    knobs()
    b = np.random.Generator(np.random.PCG64(23)).standard_normal(m.n)
    with E.EC3DSolver() as s:
        s.set_matrix_csr(*m.csr)
        xh, ith, _ = s.solve(b, np.zeros(m.n), 1e-30, 11)
    try:
        x = np.zeros(m.n)
        it = E.sprsBCGstabWR(m.valA, m.irow, m.jcol, m.n, b, x, 1e-30, 11)
        assert it == ith == 12 and np.array_equal(x, xh)
    finally:
        E.load_library().ec3d_invalidate()
