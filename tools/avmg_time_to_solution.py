"""Time to solution of the A-V time-step solve (BASELINE configs 3 and 5) with and without the block multigrid
preconditioner (EC3D_PRECOND_BLOCK_MG).

    python tools/avmg_time_to_solution.py [--cases av256 ec_src_move_hole LIM compare_to_Elmer]

Cases: av256 is ec_src_move_hole resampled to 256^3 (the set-up of tests/test_gpu_av256.py, config 3); the others are
the shipped .vxc inputs (tests/golden/g4_*.vxc).  For each, the first time step's right-hand side is built by host.run
on the device, then ec3d_solve_resident from x = 0 to the model's tol is timed (after one untimed solve) without a
preconditioner and with block-mg.  One JSON line per case: iterations, seconds, the true residual, and us per
application of M (ec3d_precond_apply minus ec3d_spmv: both move the same two host vectors)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def model_of(case):
    from eddy_currents_3d_amd import vxc
    if case == "av256":
        g = np.load(os.path.join(GOLDEN, "g4_ec_src_move_hole.npz"))
        small = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                             tuple(float(x) for x in g["adj"]))
        return vxc.resample(small, 256, 256, 256)
    return vxc.read_vxc(os.path.join(GOLDEN, f"g4_{case}.vxc"))


def timed(fn, reps=1):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["av256", "ec_src_move_hole", "LIM", "compare_to_Elmer"])
    a = ap.parse_args()
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    for case in a.cases:
        model = model_of(case)
        t = vxc.domain_tables(model)
        tol, itmax = float(t["tol"]), int(t["itmax"])
        sdz, sdy, sdx = model.vox.shape
        out = dict(case=case, grid=[sdx, sdy, sdz], tol=tol)
        kept = {}

        def on_rhs(k, s, info):
            kept["b"] = s.download("B")

        with E.EC3DSolver() as s:
            host.run(model, s, steps=1, on_rhs=on_rhs)
            out["n"] = s.n
            b, x0 = kept["b"], np.zeros(s.n)

            def solve():
                s.upload("B", b)
                s.upload("X", x0)
                s.synchronize()
                t0 = time.perf_counter()
                it, _ = s.solve_resident(tol, itmax)
                return time.perf_counter() - t0, it

            for kind in ("none", "block-mg"):
                s.set_preconditioner(kind)
                solve()
                sec, it = solve()
                out[f"{kind}_iter"], out[f"{kind}_s"] = it, round(sec, 5)
                out[f"{kind}_true_residual"] = s.true_residual()[0]
                if kind == "block-mg":
                    out["levels"] = s.preconditioner()[1]
                    r = np.random.Generator(np.random.PCG64(1)).standard_normal(s.n)
                    t_apply = timed(lambda: s.precond_apply(r), 3)
                    t_spmv = timed(lambda: s.spmv(r), 3)
                    out["us_per_M"] = round(1e6 * (t_apply - t_spmv), 1)
                    out["block-mg_us_per_iteration"] = round(1e6 * sec / max(it, 1), 1)
                else:
                    out["none_us_per_iteration"] = round(1e6 * sec / max(it, 1), 1)
        out["speedup"] = round(out["none_s"] / out["block-mg_s"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
