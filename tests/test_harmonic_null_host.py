"""The twin of the harmonic operator's left null vectors (tests/harmonic_null_numpy.py) on the CPU:
what the GPU tests compare the device with is itself checked here against dense linear algebra and against the property
the feature exists for.

* OperatorH == op.dense().conj().T @ x within 4 * 2^-53 * sum |a| |x| per row on g2, g2v, g9b, and <y, A x> == <A^H y, x>
  to 1e-12 relative;
* left_null_vectors on g2, g3, g8a, g9b at 50 Hz: every adjoint solve reaches 1e-10 under its cap, two vectors kept on
  g8a, ||A^H q|| <= 1e-2, q is NOT real (max |Im q| > 0.1 max |q|: the real Q of section 16 cannot serve) and has more
  than a tenth of its U weight on the A rows;
* solves from x^ = 0 with b^ = the fixture's b0: bicgstab_projected takes an exit within itmax = 2000 at tol 1e-6 on g2,
  g2v, g3, g8a, g9b and at 1e-8 on g3, g8a, g9b, its projected residual, recomputed from x^, is <= 10 tol, and
  harmonic_numpy.bicgstab without Q takes no exit at 1e-6.

Left out: g2 and g2v at 1e-8.  There the projected solve stalls near 1.2e-8 (4.2e-8 in this twin's sums on g2), which is
the accuracy of w at null_tol 1e-10, not a defect of the projection."""
import numpy as np
import pytest

import harmonic_null_numpy as HH
import harmonic_numpy as HN
import null_projection_numpy as NP
from conftest import load_golden

OMEGA = 2.0 * np.pi * 50.0
G2, G2V, G3 = "g2_conducting_hole_16x15x14", "g2v_conducting_moving_16x15x14", "g3_moving_coil_18x16x12"
G8A, G9B = "g8a_two_plates_18x16x16", "g9b_L_hole_near_faces_17x16x16"
_SETUP = {}


def setup_of(name):
    if name not in _SETUP:
        g = load_golden(name)
        op = HN.Operator(g, OMEGA)
        opH = HH.OperatorH(op)
        n = op.n
        sums = HN.DeviceSums(np.arange(n), -(-n // 512) * 512)
        Q, info = HH.left_null_vectors(op, opH, sums, NP.seed_rows(g["geoPHYS_C"]))
        _SETUP[name] = dict(g=g, op=op, opH=opH, sums=sums, Q=Q, info=info)
    return _SETUP[name]


def _random_complex(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.mark.parametrize("name", [G2, G2V, G9B])
def test_the_ordered_product_is_the_conjugate_transpose(name):
    g = load_golden(name)
    op = HN.Operator(g, OMEGA)
    opH = HH.OperatorH(op)
    x, y = _random_complex(op.n, 1), _random_complex(op.n, 2)
    got = opH(HN.split(x))
    want = op.dense().conj().T @ x
    bound = 4.0 * 2.0 ** -53 * opH.abs_sum(HN.split(x))
    assert np.all(np.abs(got[0] - want.real) <= bound) and np.all(np.abs(got[1] - want.imag) <= bound)
    assert np.any(got[1] != 0.0)
    ax, ahy = op(HN.split(x)), opH(HN.split(y))
    lhs, rhs = np.vdot(y, ax[0] + 1j * ax[1]), np.vdot(ahy[0] + 1j * ahy[1], x)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize("name", [G2, G3, G8A, G9B])
def test_left_null_vectors(name):
    t = setup_of(name)
    op, opH, Q, info = t["op"], t["opH"], t["Q"], t["info"]
    cap = HH.adjoint_cap(op.n)
    assert Q is not None and all(c["reached"] and c["iterations"] <= cap and c["kept"] for c in info)
    assert len(Q) == (2 if name == G8A else 1)
    nA = 3 * op.nC
    for q, c in zip(Q, info):
        aq = opH(q)
        res = np.sqrt(np.sum(aq[0] ** 2 + aq[1] ** 2))
        mod = np.hypot(q[0], q[1])
        wa, wu = np.linalg.norm(mod[:nA]), np.linalg.norm(mod[nA:])
        print(f"{name}: seed {c['seed']}, {c['iterations']} iterations (cap {cap}), ||A^H q|| = {res:.3e}, max |Im q| / max |q| = "
              f"{np.abs(q[1]).max() / mod.max():.3f}, weight on A rows {wa:.3f}, on U rows {wu:.3f}")
        assert abs(np.linalg.norm(mod) - 1.0) <= 1e-12
        assert res <= 1e-2
        assert np.abs(q[1]).max() > 0.1 * mod.max()
        assert wa > 0.1 * wu
    if len(Q) == 2:
        assert abs(np.vdot(Q[0][0] + 1j * Q[0][1], Q[1][0] + 1j * Q[1][1])) <= 1e-12


SOLVES = [(G2, 1e-6), (G2V, 1e-6), (G3, 1e-6), (G8A, 1e-6), (G9B, 1e-6), (G3, 1e-8), (G8A, 1e-8), (G9B, 1e-8)]


@pytest.mark.parametrize("name,tol", SOLVES, ids=[f"{n.split('_')[0]}-{t:g}" for n, t in SOLVES])
def test_projected_solves_go_below_the_floor(name, tol):
    t = setup_of(name)
    op, sums, Q = t["op"], t["sums"], t["Q"]
    b = HN.split(t["g"]["b0"].astype(np.complex128))
    zero = (np.zeros(op.n), np.zeros(op.n))
    x, it, restarts, relres, kind, removed = HH.bicgstab_projected(op, sums, Q, b, zero, tol, 2000)
    pres, _ = HH.projected_residual(op, sums, Q, b, x)
    print(f"{name} tol {tol:g}: iter {it}, restarts {restarts}, exit {kind}, projected residual {pres:.3e}, removed {removed:.3e}")
    assert kind != 0 and it <= 2000 and relres < tol
    assert pres <= 10 * tol
    if tol == 1e-6:
        _, it0, _, rel0, kind0 = HN.bicgstab(op, sums, b, zero, tol, 2000)
        print(f"{name} without Q: iter {it0}, exit {kind0}, recurrence residual {rel0:.3e}")
        assert kind0 == 0 and it0 == 2001
