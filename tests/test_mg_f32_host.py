"""The fp32 V-cycle (EC3D_PRECOND_FP32), host side (no GPU): its numpy float32 restatement (tests/mg_numpy_f32.py)
against the fp64 one (tests/mg_numpy.py).

* one application: M32 r is M64 r up to float32 rounding, and is not M64 r (the float32 path ran);
* mg_numpy.pbicgstab_gpuorder, unchanged, with the fp32 M plugged in: it converges to tol 1e-8, and the TRUE residual
  ||b - A x|| / ||b|| from the fp64 CSR of oracle.poisson_csr is below tol (right preconditioning: v = A p^ and
  x += alpha p^ use the same p^, so R = b - A x holds in fp64 whatever M returns).

mg_numpy_f32.TWIN_ITERS records the outer iteration counts of the two twins, asserted here; tests/test_gpu_mg_f32.py
takes the cap of the device's fp32 count from them (fp64 count + the twins' difference + 2)."""
import numpy as np
import pytest

import mg_numpy as M
import mg_numpy_f32 as M32

TOL = 1e-8

TWIN_ITERS = M32.TWIN_ITERS


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ||z32 - z64|| / ||z64|| measured on the build host (numpy float32, seed 31): 4.62e-07 at 32^3, 4.18e-07 at 48x40x33.
# The bound is 4x the measured value: a sum of float32 rounding errors (eps = 6e-8, about 40 half-sweeps and transfers
# per cycle) that moves with the seed, not a property of the device code.
@pytest.mark.parametrize("dims, measured", [((32, 32, 32), 4.62e-07), ((48, 40, 33), 4.18e-07)])
def test_fp32_apply_agrees_with_fp64(oracle, dims, measured):
    r = _rng(31).standard_normal(int(np.prod(dims)))
    m32 = M32.MG32(*dims)
    z64 = M.MG(*dims).apply(r)
    z32 = m32.apply(r)
    dist = np.linalg.norm(z32 - z64) / np.linalg.norm(z64)
    print(f"{dims}: ||z32 - z64|| / ||z64|| = {dist:.3e} (recorded {measured:.2e})")
    assert z32.dtype == np.float64 and m32.apply32(r).dtype == np.float32
    assert np.array_equal(z32, m32.apply32(r).astype(np.float64))    # widening is exact
    assert not np.array_equal(z32, z64)                               # the float32 path really ran
    assert dist <= 4 * measured
    # the inputs keep the cycle's result in the float32 normal range
    assert np.abs(z32[z32 != 0]).min() > np.finfo(np.float32).tiny


def _solve_case(oracle, case):
    from bench import bar_rhs
    if case.startswith("bar"):
        N = int(case[3:])
        return (N, N, N), bar_rhs(N)
    dims = (48, 40, 33)
    return dims, _rng(11).standard_normal(int(np.prod(dims)))


@pytest.mark.parametrize("case", sorted(TWIN_ITERS))
def test_fp32_twin_converges_to_the_true_residual(oracle, case):
    dims, b = _solve_case(oracle, case)
    n = len(b)
    valA, irow, jcol = oracle.poisson_csr(*dims)
    res = {}
    for name, mg in (("fp32", M32.MG32(*dims)), ("fp64", M.MG(*dims))):
        x, it, _, _, restarts, kind = M.pbicgstab_gpuorder(mg, b, np.zeros(n), TOL, 200)
        true = np.linalg.norm(b - oracle.spmv_csr(valA, irow, jcol, x)) / np.linalg.norm(b)
        print(f"{case} {name}: {it} outer iterations, exit {kind}, restarts {restarts}, true residual {true:.3e}")
        assert kind in (M.EXIT_S, M.EXIT_R)
        assert true < TOL
        res[name] = it
    assert (res["fp32"], res["fp64"]) == TWIN_ITERS[case]
