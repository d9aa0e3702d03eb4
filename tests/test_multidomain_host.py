"""Models with several conducting domains, on the host (no GPU): the reference's captures tests/golden/g8*_*.npz
(tools/make_multidomain_goldens.py) against vxc.domain_tables, the numpy restatement tests/multidomain_numpy.py of
the reference's U-row right-hand side rule, and the structured-form condition."""
import numpy as np
import pytest

import multidomain_numpy as MD
from conftest import load_golden

G8 = {"g8a": "g8a_two_plates_18x16x16", "g8b": "g8b_stacked_moving_20x16x14", "g8c": "g8c_side_by_side_20x18x14",
      "g8d": "g8d_g3_split_18x16x12"}


def _model(g):
    from eddy_currents_3d_amd import vxc
    return vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                        tuple(float(x) for x in g["adj"]))


@pytest.mark.parametrize("case", sorted(G8))
def test_domain_tables_number_u_as_the_captured_csr(case):
    """geoPHYS_C of vxc.domain_tables is the reference's U column numbering (domain-major), and U row 3N + n of
    the captured CSR is the equation of the n-th conducting cell in SCAN order: its U columns are that cell's own
    id and its conducting neighbours' ids."""
    from eddy_currents_3d_amd import vxc
    g = load_golden(G8[case])
    t = vxc.domain_tables(_model(g))
    gc = t["geoPHYS_C"].reshape(-1).astype(np.int64)
    assert np.array_equal(gc, g["geoPHYS_C"].reshape(-1))
    assert np.array_equal(t["geoPHYS"].reshape(-1), g["geoPHYS"].reshape(-1))
    assert np.array_equal(t["valPHYS"], g["valPHYS"])
    assert len(MD.conductors(t["geoPHYS"], t["geoPHYS_C"])) == 2
    sdz, sdy, sdx = g["vox"].shape
    N = gc.size
    irow, jcol = g["irow"], g["jcol"]
    assert len(irow) - 1 == 3 * N + np.count_nonzero(gc)
    g3 = gc.reshape(sdz, sdy, sdx)
    for n, q in enumerate(np.flatnonzero(gc)):
        k, j, i = np.unravel_index(q, g3.shape)
        nb = {int(g3[k, j, i])} | {int(g3[k + a, j + b, i + c]) for a, b, c in
                                   ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))}
        nb.discard(0)
        r = 3 * N + n
        cols = jcol[irow[r] - 1:irow[r + 1] - 1]
        assert set(int(c) for c in cols[cols > 3 * N]) == nb
    # rows and columns agree exactly when the U ids are in scan order
    scan = np.array_equal(gc[gc != 0], 3 * N + 1 + np.arange(np.count_nonzero(gc)))
    assert scan == (case != "g8c")


@pytest.mark.parametrize("case", sorted(G8))
def test_reference_rule_rebuilds_every_captured_rhs(case):
    """Starting from zeros, then from each captured x_out after the post-update, the restatement of
    src/EC3D.f90:277-404 with the project's source program gives every captured b bit for bit; the U rows past
    max siznod are 0 there, and rule "all" would have given some of them a nonzero value (not on g8d, whose rows
    past max siznod all lie on the plate's top face, which cel_bndUz zeroes anyway)."""
    from eddy_currents_3d_amd import host, vxc
    g = load_golden(G8[case])
    model = _model(g)
    prog = host.SourceProgram(model, vxc.domain_tables(model))
    shape, dt = g["vox"].shape, float(g["dt"])
    N = int(np.prod(shape))
    sizes = [len(c) for _, c in MD.conductors(g["geoPHYS"], g["geoPHYS_C"])]
    b = np.zeros(len(g["irow"]) - 1)
    x = np.zeros_like(b)
    T = 0.0
    differs = False
    for k in range(len(g["iters"])):
        idx, val, moving = prog.step(T)
        args = (g["irow"], g["jcol"], g["valA"], g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape, b, x, idx,
                val, moving)
        bk = MD.rhs_step(*args)
        assert np.array_equal(bk, g[f"b{k}"]), f"step {k}"
        assert not np.any(g[f"b{k}"][3 * N + max(sizes):])
        differs |= bool(np.any(MD.rhs_step(*args, rule="all")[3 * N + max(sizes):]))
        b, x = MD.post_update(g["geoPHYS"], g["geoPHYS_C"], g["valPHYS"], dt, shape, g[f"b{k}"], g[f"xout{k}"])
        T = T + dt
    assert differs == (case != "g8d")


def test_structured_condition_classifies_the_captures():
    """g8a/b/d keep the structured form (U ids in scan order), g8c (domain 2 on the -x side of domain 1) does not;
    22 conducting domains are the most the class byte holds."""
    got = {c: MD.structured_applies(load_golden(n)["geoPHYS"], load_golden(n)["geoPHYS_C"]) for c, n in G8.items()}
    assert got == {"g8a": True, "g8b": True, "g8c": False, "g8d": True}
    from eddy_currents_3d_amd import vxc
    for D, want in ((22, True), (23, False), (24, False)):
        vox, names = MD.blocks_model(D)
        t = vxc.domain_tables(vxc.VxcModel(vox, names, 0.004, (1, 1, 1)))
        assert len(MD.conductors(t["geoPHYS"], t["geoPHYS_C"])) == D
        assert MD.structured_applies(t["geoPHYS"], t["geoPHYS_C"]) == want
