"""ec3d_set_matrix_csr / sprsbcgstabwr_ on matrices that are not grid stencils (tests/csr_generate.py: 1 .. 16 bands,
a 27-point stencil cut to 16, the 40 % threshold, the row sample, seven bands that are no 7-point grid -- among them
matrices with the grid's offsets and nonzero coefficients in every wrap slot --, tail shapes, tiny sizes), against

* the restatement of the split rule (tests/bands_tail_numpy.py) for the storage form,
* the oracle's stored-order row sum (oracle.spmv_csr, src/solvers.f90:54-61) bit for bit, and, independently of the
  oracle's C code, the row sum in np.longdouble within the sequential-summation bound
  gamma_k sum_j |a_ij x_j|, gamma_k = k u / (1 - k u), u = 2^-53, k = the row's length (derived, not measured; the
  reference's own rounding, k 2^-63 relative, and one subnormal spacing per operation for products that underflow
  are added to it),
* the GPU-order twin of the solver bit for bit and the reference's own order within 10 tol (SURVEY's bar).

tests/test_generated_csr_host.py pins the corpus and the restatement on the host.  Every test prints the format and
the launch form that ran."""
import numpy as np
import pytest

import bands_tail_numpy as BT
import csr_generate as G
from eddy_currents_3d_amd.solver import PRECOND_E_MATRIX
from test_generated_csr_host import ITMAX, TOL, form_of, rhs_of

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TINY = np.longdouble(2.0) ** -1074


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def describe(s):
    """Which kernels serve the handle's matrix (fmt_of in csrc/ec3d_kernels.hip goes by the same two numbers) and on
    which launch form."""
    mi, g = s.info, s.geometry(1)
    fmt = (f"DICT7 ({mi.dict_classes} classes)" if mi.dict_classes else "DIA7") if mi.nbands == 7 else f"generic, {mi.nbands} bands"
    form = (f"z-march ({g.zm_tpp} tiles per plane)" if g.zm_tpp else "linear tiles") + \
           (f", {g.patch_x} x {g.patch_y} patches" if g.patch_x else "") + f", {g.nblk} workgroups"
    return f"{fmt} + {mi.tail_rows} tail rows; {form}"


def vectors(n, few_units=False):
    """(label, x): standard normal, entries spanning 1e+-100, unit vectors at rows 0, n - 1 and both sides of every
    tile boundary (of the first and the last boundary only where the matrix has thousands of tiles)."""
    rng = np.random.Generator(np.random.PCG64(11))
    out = [("normal", rng.standard_normal(n)),
           ("1e+-100", rng.choice((-1.0, 1.0), n) * 10.0 ** rng.uniform(-100.0, 100.0, n))]
    edges = list(range(512, n, 512))
    if few_units and len(edges) > 2:
        edges = [edges[0], edges[-1]]
    for r in sorted({0, n - 1} | {e - 1 for e in edges} | set(edges)):
        e = np.zeros(n)
        e[r] = 1.0
        out.append((f"unit {r}", e))
    return out


def check_product(s, O, valA, irow, jcol, label, x, bound=True):
    y = s.spmv(x)
    assert np.all(np.isfinite(y)), label
    assert np.array_equal(y, O.spmv_csr(valA, irow, jcol, x)), label
    if bound:
        yl, mag, k = BT.product_of_csr(valA, irow, jcol, x)
        k = k.astype(np.longdouble)
        limit = (k * U / (1 - k * U) + k * np.longdouble(2.0) ** -63) * mag + k * TINY
        err = np.abs(y.astype(np.longdouble) - yl)
        assert np.all(err <= limit), (label, float((err / np.maximum(limit, TINY)).max()))
    return y


def formats_of(intent):
    return (False, True) if intent["dict"] else (False,)


# ------------------------------------------------------------------------------------------ form and product
@pytest.mark.parametrize("name", G.CASES)
def test_form_and_product(E, oracle, name):
    valA, irow, jcol, intent = G.case(name)
    f = form_of(name)
    big = name == "sampling"
    for dictionary in formats_of(intent):
        with E.EC3DSolver() as s:
            s.set_format(dictionary)
            s.set_matrix_csr(valA, irow, jcol)
            mi = s.info
            print(f"{name}, dictionary {'on' if dictionary else 'off'}: {describe(s)}")
            assert (mi.n, mi.n_pad, mi.nnz, mi.nbands) == (f["n"], f["n_pad"], f["nnz"], f["nbands"])
            assert list(mi.band_offset[:mi.nbands]) == f["band_offset"]
            assert (mi.tail_rows, mi.tail_entries_padded) == (f["tail_rows"], f["tail_entries_padded"])
            assert (mi.dict_classes > 0) == (dictionary and intent["dict"])
            for label, x in vectors(f["n"], few_units=big):
                check_product(s, oracle, valA, irow, jcol, label, x, bound=not (big and label.startswith("unit")))


# -------------------------------------------------------------------------------------------- launch variants
@pytest.mark.parametrize("name", G.CASES)
def test_launch_variants_give_the_same_bits(E, oracle, monkeypatch, name):
    """Workgroup counts 1, 3, 8; with seven bands EC3D_ZMARCH 0 / 1; on the wrap matrices EC3D_PATCH 0 / 1 as well.
    s.geometry(1) says which form ran: the z-march exists where the outermost offset is a whole number of tiles and
    there are >= 8 planes -- the wrap matrices --, the 2-D patches where such a matrix is in the dictionary form and
    has no tail."""
    valA, irow, jcol, intent = G.case(name)
    n = intent["n"]
    x = vectors(n)[0][1]
    want = oracle.spmv_csr(valA, irow, jcol, x)
    planes = name in G.WRAP_OFFSETS
    variants = [dict(nblk=k) for k in (1, 3, 8)]
    if intent["nbands"] == 7:
        variants += [dict(zm=z) for z in ("0", "1")]
    if planes:
        variants += [dict(zm=z, patch=p) for z in ("0", "1") for p in ("0", "1")]
    seen = set()
    for dictionary in formats_of(intent):
        for v in variants:
            for key, env in (("zm", "EC3D_ZMARCH"), ("patch", "EC3D_PATCH")):
                if key in v:
                    monkeypatch.setenv(env, v[key])
                else:
                    monkeypatch.delenv(env, raising=False)
            with E.EC3DSolver(nblk=v.get("nblk")) as s:
                s.set_format(dictionary)
                s.set_matrix_csr(valA, irow, jcol)
                g = s.geometry(1)
                zm = planes and v.get("zm", "1") == "1"
                patch = zm and v.get("patch", "1") == "1" and dictionary and intent["dict"] and intent["tail_rows"] == 0
                assert g.zm_tpp == (G.WRAP_OFFSETS[name][6] // 512 if zm else 0), v
                assert (g.patch_x, g.patch_y) == ((128, 4) if patch else (0, 0)), v
                assert (g.patch_sdx == G.WRAP_OFFSETS[name][5]) if patch else (g.patch_sdx == 0), v
                seen.add((bool(s.info.dict_classes), zm, patch))
                assert np.array_equal(s.spmv(x), want), (v, describe(s))
    print(f"{name}: (dictionary, z-march, patches) that ran: {sorted(seen)}")
    if name in ("wrap128_dict", "wrap256_dict"):
        assert {(True, True, True), (True, True, False), (True, False, False), (False, True, False),
                (False, False, False)} <= seen


def test_an_extra_entry_only_changes_its_own_row(E):
    """wrap128_extra is a wrap matrix plus one tail entry: the z-march stays, the patches go, and y differs from the
    product of the matrix without that entry in that one row, by that one product added last."""
    valA, irow, jcol, intent = G.case("wrap128_extra")
    n = intent["n"]
    f = form_of("wrap128_extra")
    t = np.flatnonzero(f["band"] < 0)
    assert len(t) == 1
    keep = np.ones(len(valA), bool)
    keep[t] = False
    r = int(f["row"][t[0]])
    irow2 = irow.copy()
    irow2[r + 1:] -= 1
    x = vectors(n)[0][1]
    with E.EC3DSolver() as s:
        s.set_matrix_csr(valA, irow, jcol)
        assert s.geometry(1).zm_tpp == 4 and s.geometry(1).patch_x == 0 and s.info.tail_rows == 1
        y = s.spmv(x)
        s.set_matrix_csr(valA[keep], irow2, jcol[keep])
        assert s.geometry(1).patch_x == 128 and s.info.tail_rows == 0
        y0 = s.spmv(x)
    assert np.array_equal(np.delete(y, r), np.delete(y0, r))
    assert y[r] == y0[r] + valA[t[0]] * x[jcol[t[0]] - 1]


# ------------------------------------------------------------------------------------------------------ solve
def same_as_twin(O, s, valA, irow, jcol, b, x0, tol, itmax, cap):
    """x, iter and the residual history against the GPU-order twin, bit for bit.  The device records ||R|| of an
    iteration in the kernel that begins the next one, so the last iteration's is compared through x alone."""
    x, it, hist = s.solve(b, x0, tol, itmax, hist_cap=cap)
    xt, itt, hs, hr = O.twin_solve(s, valA, irow, jcol, b, x0, tol, itmax, hist_cap=cap)
    m = min(it, cap)
    assert it == itt, (it, itt)
    assert np.array_equal(x, xt)
    assert np.array_equal(hist[:m, 0], hs[:m]) and np.array_equal(hist[:m - 1, 1], hr[:m - 1])
    assert np.all(np.isnan(hist[m:])) and np.all(np.isnan(hs[m:]))
    return x, it


@pytest.mark.parametrize("name", G.SOLVE)
def test_solve_equals_the_twin_and_meets_the_references_x(E, oracle, monkeypatch, name):
    valA, irow, jcol, intent = G.case(name)
    n = intent["n"]
    b = rhs_of(name)
    xr, itr, _, _ = oracle.bicgstab_wr(valA, irow, jcol, b, np.zeros(n), TOL, ITMAX)
    assert 0 < itr < ITMAX
    runs = [(d, "0") for d in formats_of(intent)]
    if name in ("wrap128_dict", "wrap256_dict"):
        runs.append((True, "2"))                # K2 inside K3, K5 inside the next K1, on the 2-D patches
    for dictionary, fuse in runs:
        monkeypatch.setenv("EC3D_FUSE23", fuse)
        monkeypatch.setenv("EC3D_FUSE51", fuse)
        with E.EC3DSolver() as s:
            s.set_format(dictionary)
            s.set_matrix_csr(valA, irow, jcol)
            assert s.fusion() == ((1, 1) if fuse == "2" else (0, 0))
            x, it = same_as_twin(oracle, s, valA, irow, jcol, b, np.zeros(n), TOL, ITMAX, 64)
            err = np.linalg.norm(x - xr) / np.linalg.norm(xr)
            print(f"{name}: {describe(s)}, fusion {s.fusion()}: {it} iterations (reference order {itr}), "
                  f"x vs the reference's {err:.2e}")
            assert 0 < it < ITMAX and err <= 10 * TOL
            xw, itw = same_as_twin(oracle, s, valA, irow, jcol, b, 0.5 * x, TOL, ITMAX, 64)
            xwr, _, _, _ = oracle.bicgstab_wr(valA, irow, jcol, b, 0.5 * x, TOL, ITMAX)
            assert 0 < itw < ITMAX and np.linalg.norm(xw - xwr) <= 10 * TOL * np.linalg.norm(xwr)
            _, it3 = same_as_twin(oracle, s, valA, irow, jcol, b, np.zeros(n), TOL, 3, 8)       # the itmax exit
            assert it3 == 4


@pytest.mark.parametrize("name", G.DROPIN)
def test_dropin_symbol_gives_what_the_handle_gives(E, name):
    valA, irow, jcol, intent = G.case(name)
    n = intent["n"]
    b = rhs_of(name)
    with E.EC3DSolver() as s:
        s.set_matrix_csr(valA, irow, jcol)
        xh, ith, _ = s.solve(b, np.zeros(n), TOL, ITMAX)
    try:
        x = np.zeros(n)
        it = E.sprsBCGstabWR(valA, irow, jcol, n, b, x, TOL, ITMAX)
        assert it == ith and np.array_equal(x, xh)
    finally:
        E.load_library().ec3d_invalidate()


# ------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", [c for c in G.CASES if c != "sampling"] + ["sampling"])
def test_export_gives_the_matrix_back(E, oracle, name):
    """ec3d_export_csr: the exported triple multiplies out to the handle's own product bit for bit; without explicit
    zeros it IS the input with every row's band part in band order (zeros do not round-trip: include/ec3d_hip.h)."""
    valA, irow, jcol, intent = G.case(name)
    x = vectors(intent["n"])[0][1] if name != "sampling" else np.random.Generator(np.random.PCG64(3)).standard_normal(intent["n"])
    for dictionary in formats_of(intent):
        with E.EC3DSolver() as s:
            s.set_format(dictionary)
            s.set_matrix_csr(valA, irow, jcol)
            va, ir, jc = s.export_csr()
            assert np.array_equal(oracle.spmv_csr(va, ir, jc, x), s.spmv(x))
        if intent["zero"]:
            assert len(va) == np.count_nonzero(valA) and np.all(va != 0.0)
        else:
            vb, ib, jb = BT.band_order(valA, irow, jcol, form_of(name))
            assert np.array_equal(ir, ib) and np.array_equal(jc, jb) and np.array_equal(va, vb)


# ------------------------------------------------------------------------ several GPUs' code on one card
@pytest.mark.parametrize("name", G.CASES)
def test_slabs_on_one_card(E, oracle, name):
    """The wrap matrices are cut plane by plane (ec3d_probe_csr_multi says so on the host): the slabs' product is
    the oracle's bit for bit, the solve meets the undivided handle's x within 10 tol.  Everything else is refused
    with status 7, and the handle takes a Poisson matrix afterwards."""
    valA, irow, jcol, intent = G.case(name)
    n = intent["n"]
    x = np.random.Generator(np.random.PCG64(19)).standard_normal(n)
    for world in (2, 3):
        cut, _ = E.probe_csr_multi(valA, irow, jcol, world)
        assert cut == (name in G.WRAP)
        with E.EC3DMulti(world, devices=[0] * world) as m:
            if cut:
                m.set_matrix_csr(valA, irow, jcol)
                assert m.n == n
                assert np.array_equal(m.spmv(x), oracle.spmv_csr(valA, irow, jcol, x))
                if intent["solve"]:
                    b = rhs_of(name)
                    with E.EC3DSolver() as s:
                        s.set_matrix_csr(valA, irow, jcol)
                        xs, its, _ = s.solve(b, np.zeros(n), TOL, ITMAX)
                    xm, itm = m.solve(b, np.zeros(n), TOL, ITMAX)
                    print(f"{name} in {world} slabs: {itm} iterations, undivided {its}")
                    assert 0 < itm < ITMAX and np.linalg.norm(xm - xs) <= 10 * TOL * np.linalg.norm(xs)
            else:
                with pytest.raises(E.EC3DError) as err:
                    m.set_matrix_csr(valA, irow, jcol)
                assert err.value.status == 7
                m.assemble_poisson(8, 8, 8)
                xp = np.random.Generator(np.random.PCG64(23)).standard_normal(512)
                assert np.array_equal(m.spmv(xp), oracle.spmv_csr(*oracle.poisson_csr(8, 8, 8), xp))


# --------------------------------------------------------------------------------------------------- refusals
def test_bad_triples_are_refused_and_the_handle_lives_on(E, oracle):
    valA, irow, jcol, intent = G.case("n513")
    n = intent["n"]
    b = rhs_of("n513")
    mid = len(jcol) // 2
    bad_low, bad_high, bad_start = jcol.copy(), jcol.copy(), irow.copy()
    bad_low[mid] = 0
    bad_high[mid] = n + 1
    bad_start[0] = 0
    with E.EC3DSolver() as s:
        for v, i, j in ((np.zeros(0), np.ones(1, np.int32), np.zeros(0, np.int32)), (valA, bad_start, jcol),
                        (valA, irow, bad_low), (valA, irow, bad_high)):
            with pytest.raises(E.EC3DError) as err:
                s.set_matrix_csr(v, i, j)
            assert err.value.status == 2 and str(err.value).split("): ", 1)[1].startswith("ec3d_set_matrix_csr: ")
            s.set_matrix_csr(valA, irow, jcol)
            x, it, _ = s.solve(b, np.zeros(n), TOL, ITMAX)
            xt, itt, _, _ = oracle.twin_solve(s, valA, irow, jcol, b, np.zeros(n), TOL, ITMAX)
            assert it == itt and np.array_equal(x, xt)


@pytest.mark.parametrize("name", ["nb3", "wrap128_dict"])
def test_multigrid_is_refused_on_a_generic_matrix(E, oracle, name):
    valA, irow, jcol, intent = G.case(name)
    n = intent["n"]
    b = rhs_of(name)
    with E.EC3DSolver() as s:
        s.set_matrix_csr(valA, irow, jcol)
        x0, it0, _ = s.solve(b, np.zeros(n), TOL, ITMAX)
        for kind in ("mg", "block-mg"):
            with pytest.raises(E.EC3DError) as err:
                s.set_preconditioner(kind)
            assert err.value.status == PRECOND_E_MATRIX
            assert s.preconditioner()[0] == "none"
            x, it, _ = s.solve(b, np.zeros(n), TOL, ITMAX)
            assert it == it0 and np.array_equal(x, x0)
