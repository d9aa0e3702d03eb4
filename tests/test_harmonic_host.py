"""CPU-only: the time-harmonic operator and solve as tests/harmonic_numpy.py restates them.

* table pin: on five captured A-V systems, every stored entry of the reference's CSR is re + im r of the twin's two tables,
  r = 2 / (omega dt) in A rows and 1 / (omega dt) in U rows, to 4 ulp of the terms; no twin entry outside the captured
  pattern; im != 0 only on the diagonal of a conducting A row and in the A slots of a U row;
* the source phasor of host.run_harmonic: a for a cos(2 pi f t), -j a for a sin(2 pi f t); moving sources are refused;
* g1 (no conductor): m is all zero and the solve of (1 + 2j) b is (1 + 2j) times the real solve within 2 cond(A) tol."""
import numpy as np
import pytest

import harmonic_numpy as HN
from conftest import load_golden

PIN = ["g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14", "g3_moving_coil_18x16x12",
       "g8a_two_plates_18x16x16", "g9b_L_hole_near_faces_17x16x16"]
OMEGA = 2.0 * np.pi * 61.7          # arbitrary: nothing in the pin depends on it


@pytest.mark.parametrize("name", PIN)
def test_table_pin(name):
    g = load_golden(name)
    op = HN.Operator(g, OMEGA)
    n, nC, dt = op.n, op.nC, float(g["dt"])
    irow, jcol, valA = g["irow"].astype(np.int64), g["jcol"].astype(np.int64) - 1, g["valA"]
    assert n == len(irow) - 1
    crow = np.repeat(np.arange(n), np.diff(irow))
    ckey = crow * n + jcol
    tkey = op.row * n + op.col
    assert len(np.unique(tkey)) == len(tkey)
    o = np.argsort(tkey)
    pos = np.searchsorted(tkey[o], ckey)
    assert np.all(pos < len(tkey)) and np.array_equal(tkey[o][pos], ckey), "a captured entry has no table slot"
    re, im = op.re[o][pos], op.im[o][pos]
    r = np.where(crow < 3 * nC, 2.0 / (OMEGA * dt), 1.0 / (OMEGA * dt))
    err = np.abs(re + im * r - valA)
    bound = 4.0 * 2.0 ** -53 * (np.abs(re) + np.abs(im) * r)
    worst = int(np.argmax(err - bound))
    print(f"{name}: {len(valA)} entries, max |re + im r - valA| / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
    assert np.all(err <= bound), (crow[worst], jcol[worst], re[worst], im[worst], valA[worst])
    # the twin has no entry where the capture has none
    nz = (op.re != 0.0) | (op.im != 0.0)
    assert np.all(np.isin(tkey[nz], ckey))
    # im != 0 only in the slots the definition names
    cls = op.cls[op.row]
    a_diag = (cls >= op.ids["a0"]) & (cls < op.ids["u0"]) & (op.slot == 3)
    u_a = (cls >= op.ids["u0"]) & (op.slot >= 7)
    assert not np.any((op.im != 0.0) & ~(a_diag | u_a))
    assert np.all(op.im[a_diag] != 0.0)
    # conductor velocity terms stay in re (g2v moves its conductor)
    if "moving" in name and "g2v" in name:
        a_rows = (cls >= op.ids["a0"]) & (cls < op.ids["u0"])
        assert np.any(op.re[a_rows & (op.slot == 2)] != op.re[a_rows & (op.slot == 4)])


def test_tables_have_the_documented_shape():
    g = load_golden(PIN[0])
    op = HN.Operator(g, OMEGA)
    ids = op.ids
    assert ids["ncls"] == 64 and op.re_t.shape == (64, 16)
    assert not op.m_t[:ids["a0"]].any() and not op.m_t[ids["zero"]].any() and not op.re_t[ids["zero"]].any()
    C = float(g["valPHYS"][op.doms[0] - 1, 1])
    assert np.all(op.m_t[ids["a0"]:ids["u0"], 3] == C)
    d = np.asarray(g["delta"], np.float64)
    full = op.m_t[ids["u0"]]                       # nmiss == 0
    for k in range(3):
        assert full[7 + 3 * k] == 0.5 * (1.0 / d[k]) and full[7 + 3 * k + 1] == 0.0 and full[7 + 3 * k + 2] == 0.5 * (-1.0 / d[k])
    assert np.array_equal(op.im_t, OMEGA * op.m_t)


class _F:
    def __init__(self, fn):
        self.value = fn


def test_source_phasor():
    from eddy_currents_3d_amd import host
    f, a = 50.0, 3.25
    c = host.source_phasor(_F(lambda t: a * np.cos(2 * np.pi * f * t)), f)
    s = host.source_phasor(_F(lambda t: a * np.sin(2 * np.pi * f * t)), f)
    assert abs(c - a) <= 1e-12 * a and abs(s - (-1j * a)) <= 1e-12 * a
    assert abs(HN.source_phasor(lambda t: a * np.cos(2 * np.pi * f * t), f) - c) <= 1e-15 * a


def test_shipped_model_phasor_and_moving_sources_refused():
    import os
    from conftest import GOLDEN
    from eddy_currents_3d_amd import host, vxc
    model = vxc.read_vxc(os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc"))
    t = vxc.domain_tables(model)
    prog = host.SourceProgram(model, t)
    assert not prog.moving
    n = 3 * model.vox.size + t["ncells0"]
    b = host.harmonic_rhs(prog, 50.0, n)
    nzb = b[b != 0]
    assert len(nzb) == sum(len(f["nodes"]) for f in prog.funs) > 0
    for f in prog.funs:      # f1 = a cos(2 pi 50 t): a real phasor, the function's value at T = 0
        a = f["f"].value(0.0) * host.MU0
        got = b[f["nodes"][0] + f["axis"] * prog.ncells - 1]
        assert abs(got - a) <= 1e-12 * abs(a)
    moving = vxc.read_vxc(os.path.join(GOLDEN, "g4_ec_src_move_hole.vxc"))
    mp = host.SourceProgram(moving, vxc.domain_tables(moving))
    assert mp.moving
    with pytest.raises(ValueError, match="move"):
        host.harmonic_rhs(mp, 50.0, 3 * moving.vox.size + vxc.domain_tables(moving)["ncells0"])


def test_g1_without_conductor_is_the_real_solve_times_a_constant(oracle):
    g = load_golden("g1_nonconducting_8x7x6")
    op = HN.Operator(g, OMEGA)
    # no row has a conducting or a U class, so m of every stored entry is zero (the table's unused classes are not)
    assert op.cls.max() < op.ids["a0"] and not op.m_t[op.cls[op.row], op.slot].any() and not op.im.any()
    n, tol, itmax = op.n, float(g["tol"]), int(g["itmax"])
    assert n == 1008
    A = op.dense()
    assert np.array_equal(A.imag, np.zeros_like(A.imag))
    # the real part IS the captured matrix, entry for entry (no dt term anywhere without a conductor)
    irow, jcol = g["irow"].astype(np.int64), g["jcol"].astype(np.int64) - 1
    ref = np.zeros((n, n))
    ref[np.repeat(np.arange(n), np.diff(irow)), jcol] = g["valA"]
    assert np.array_equal(A.real, ref)
    cond = np.linalg.cond(ref)
    b = g["b0"]
    assert np.linalg.norm(b) > 0
    sums = HN.DeviceSums(np.arange(n), -(-n // 512) * 512)
    z = 1.0 + 2.0j
    xh, it_h, _, relres, _ = HN.bicgstab(op, sums, HN.split(z * b), HN.split(np.zeros(n)), tol, itmax)
    xre, it_re = oracle.bicgstab_wr(g["valA"], g["irow"], g["jcol"], b, np.zeros(n), tol, itmax)[:2]   # the real solve
    assert it_h <= itmax and it_re <= itmax and relres < tol
    xh = xh[0] + 1j * xh[1]
    want = z * xre
    err = np.linalg.norm(xh - want) / np.linalg.norm(want)
    print(f"g1: cond(A) = {cond:.3e}, iterations {it_h} / {it_re}, |x^ - (1 + 2j) x| / |x| = {err:.3e}, bar {2 * cond * tol:.3e}")
    assert err <= 2.0 * cond * tol
    # and both are solutions of the captured system
    assert np.linalg.norm(ref @ xre - b) / np.linalg.norm(b) <= 10 * tol
    assert np.linalg.norm(A @ xh - z * b) / np.linalg.norm(z * b) <= 10 * tol
