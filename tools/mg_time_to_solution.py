"""Time-to-solution of the bar-RHS Poisson solve (BASELINE config 2) with and without the multigrid preconditioner.

    python tools/mg_time_to_solution.py [--sizes 256 512] [--tol 1e-8] [--fixed 200] [--precision fp64|fp32]
                                        [--coarsening rediscretize|aggregate] [--mg-only | --none-only] [--label TEXT]
                                        [--csr jump|convect]

One JSON line per size: wall time of ec3d_solve_resident to `tol` with MG (after one untimed solve) and its outer
iterations; the same without a preconditioner -- a full solve where --fixed is 0 or the size is <= 256, otherwise a
fixed `--fixed` iterations (tol 1e-300) scaled by the reference's iteration count (tests/golden/g5_cube*.npz `iter`,
or BASELINE.md section 2b's projection of 7 500 at 512^3), which the line says; and us per V-cycle, from
ec3d_precond_apply minus ec3d_spmv (both move the same two host vectors; the split by level comes from a
rocprofv3 --kernel-trace --stats run of this tool, profiles/mg_*.txt).  --precision fp32: the V-cycle in single
precision (ec3d_set_precond_precision); --coarsening aggregate: the hierarchy of ec3d_set_precond_coarsening, which every
size has (the line then names each level's kind); a size without a reference count is scaled by the nearest one's,
in proportion to N, which the line says.  --mg-only leaves the unpreconditioned solve out, --none-only the
preconditioned one (it then runs on a library without either setter); --label goes into the line as "build".
--csr jump|convect: instead of ec3d_assemble_poisson, the variable-coefficient operator of that name
(tests/csr_grid_generate.py: a diffusion coefficient with a jump of 10^3; diffusion + upwind convection) is built on
the host, uploaded with ec3d_set_matrix_csr and given its box with ec3d_set_precond_grid, so the hierarchy is made from
the matrix alone (--coarsening is then ignored).  There is no reference count for these: the unpreconditioned figure is
a full solve capped at --none-itmax iterations, and when the cap is hit the line says so and gives the rate
(none_ms_per_iteration) instead of a time to solution."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REF_ITERS = {64: 603, 128: 1439, 256: 4097, 512: 7500}


def ref_iters(N):
    """(the reference's iteration count at N^3, how it was got)"""
    if N in REF_ITERS:
        return REF_ITERS[N], f"the reference's {REF_ITERS[N]}"
    near = min(REF_ITERS, key=lambda m: abs(m - N))
    it = round(REF_ITERS[near] * N / near)
    return it, f"{it} = the reference's {REF_ITERS[near]} at {near}^3 times {N}/{near}"


def timed(fn, reps=1):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--fixed", type=int, default=200)
    ap.add_argument("--precision", choices=["fp64", "fp32"], default="fp64")
    ap.add_argument("--coarsening", choices=["rediscretize", "aggregate"], default="rediscretize")
    ap.add_argument("--mg-only", action="store_true")
    ap.add_argument("--none-only", action="store_true")
    ap.add_argument("--label")
    ap.add_argument("--csr", choices=["jump", "convect"])
    ap.add_argument("--none-itmax", type=int, default=20000)
    a = ap.parse_args()
    import eddy_currents_3d_amd as E
    from bench import bar_rhs
    for N in a.sizes:
        out = dict(N=N, tol=a.tol, precision=a.precision, coarsening=a.coarsening)
        if a.label:
            out = dict(build=a.label, **out)
        if a.none_only:
            del out["precision"], out["coarsening"]
        if a.csr:
            out["operator"] = a.csr
            out.pop("coarsening", None)
        b = bar_rhs(N)
        x0 = np.zeros(N ** 3)
        with E.EC3DSolver() as s:
            if a.csr:
                sys.path.insert(0, os.path.join(REPO, "tests"))
                import csr_grid_generate as G
                s.set_matrix_csr(*G.case(a.csr, (N, N, N))[:3])
                info = s.info
                out["dict_classes"] = int(info.dict_classes)
                G._cache.clear()
            else:
                s.assemble_poisson(N, N, N)

            def solve(tol=a.tol, itmax=100000):
                s.upload("B", b)
                s.upload("X", x0)
                s.synchronize()
                t = time.perf_counter()
                it, _ = s.solve_resident(tol, itmax)
                return time.perf_counter() - t, it

            if not a.none_only:
                if a.precision == "fp32":   # (the defaults set nothing: the tool then also runs on a library without the setters)
                    s.set_precond_precision("fp32")
                if a.csr:
                    s.set_preconditioner("mg", grid=(N, N, N))
                    out["level_kinds"] = s.precond_coarsening()[2]
                elif a.coarsening == "aggregate":
                    s.set_precond_coarsening("aggregate")
                    s.set_preconditioner("mg")
                    out["level_kinds"] = s.precond_coarsening()[2]
                else:
                    s.set_preconditioner("mg")
                out["levels"] = s.preconditioner()[1]
                solve()
                out["mg_s"], out["mg_iter"] = solve()
                out["mg_true_residual"] = s.true_residual()[0]
                r = np.random.Generator(np.random.PCG64(1)).standard_normal(N ** 3)
                t_apply, _ = timed(lambda: s.precond_apply(r), 3)
                t_spmv, _ = timed(lambda: s.spmv(r), 3)
                out["us_per_vcycle"] = round(1e6 * (t_apply - t_spmv), 1)
                out["mg_us_per_outer_iteration"] = round(1e6 * out["mg_s"] / max(out["mg_iter"], 1), 1)
                s.set_preconditioner("none")
            if not a.mg_only and a.csr:
                out["none_s"], out["none_iter"] = solve(itmax=a.none_itmax)
                out["none_true_residual"] = s.true_residual()[0]
                out["none_ms_per_iteration"] = round(1e3 * out["none_s"] / max(out["none_iter"], 1), 4)
                out["none_capped"] = out["none_iter"] > a.none_itmax
                if out["none_capped"]:
                    out["none_note"] = f"stopped at itmax = {a.none_itmax} without reaching tol: a rate, not a time to solution"
            elif not a.mg_only:
                if a.fixed and N > 256:
                    solve(1e-300, a.fixed - 1)
                    t, it = solve(1e-300, a.fixed - 1)
                    out["none_fixed_iters"], out["none_fixed_s"] = it, t
                    out["none_iter"], how = ref_iters(N)
                    out["none_s"] = t / it * out["none_iter"]
                    out["none_note"] = f"{it} fixed iterations scaled to {how}"
                else:
                    out["none_s"], out["none_iter"] = solve()
        if "none_s" in out and "mg_s" in out and not out.get("none_capped"):
            out["speedup"] = round(out["none_s"] / out["mg_s"], 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
