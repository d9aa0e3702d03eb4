"""The reference's time loop with and without a history of earlier solutions (ec3d_set_guess_history).

    python tools/guess_history_time_loop.py [--cases LIM ec_src_move_hole] [--depths 0 4 8] [--steps N] [--runs R]
                                            [--label TEXT] [--out profiles/guess_history.jsonl]

One JSON line per case, depth and run, appended to --out and printed: iterations of every step, the wall time of the
loop (host.run without output, the assembly included) and of the solves alone (EC3DSolver.solve_resident, which
returns when x is there: projection, iteration and update of the history), every step's true residual
(ec3d_true_residual, on the device, before the post-update) and -- with a history -- how often the new pair was kept
and the residual the projection left on average.  LIM: the shipped input (tests/golden/g4_LIM), 200 steps;
ec_src_move_hole: the shipped input resampled to 256 x 256 x 60 (vxc.resample, as tests/test_gpu_fullsize.py), 50 steps.
Depth 0 never calls ec3d_set_guess_history, so the tool also runs on a build that has no such call (--label names the
build in the line): that is how depth 0 is compared with the parent commit.  The device time of the projection's and
the update's kernels (k_guess_*) comes from a rocprofv3 --kernel-trace --stats run of this tool with one case and depth."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "eddy_currents_3d_amd")) for p in sys.path if p):
    sys.path.insert(0, REPO)      # (a PYTHONPATH that names another build of the package wins)

CASES = {"LIM": (None, 200), "ec_src_move_hole": ((256, 256, 60), 50)}


def model_of(case):
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(REPO, "tests", "golden", f"g4_{case}.npz"))
    m = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    dims = CASES[case][0]
    return (vxc.resample(m, *dims) if dims else m), float(g["tol"])


def one_run(E, host, model, depth, steps):
    res, kept, after, solve_s = [], [], [], [0.0]
    with E.EC3DSolver() as s:
        inner = s.solve_resident

        def timed_solve(*a, **k):
            t = time.perf_counter()
            out = inner(*a, **k)
            solve_s[0] += time.perf_counter() - t
            return out
        s.solve_resident = timed_solve

        def on_solved(k, s, info):
            res.append(float(s.true_residual()[0]))
            if "guess" in info:
                kept.append(info["guess"]["kept"])
                after.append(info["guess"]["res_after"])
        t0 = time.perf_counter()
        log = host.run(model, s, steps=steps, on_solved=on_solved, **({"guess_history": depth} if depth else {}))
        s.synchronize()
        wall = time.perf_counter() - t0
        n = int(s.n)
    out = dict(n=n, steps=len(log), iters=[int(i["iter"]) for i in log], wall_s=round(wall, 4), solve_s=round(solve_s[0], 4),
               true_residual_max=max(res), true_residual=[float(f"{r:.4e}") for r in res])
    out["iters_total"] = sum(out["iters"])
    if depth:
        out["pairs_kept"] = int(sum(1 for k in kept if k == 1))
        out["history_cleared"] = int(sum(1 for k in kept if k == -1))
        out["res_after_mean"] = float(np.mean(after))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--depths", type=int, nargs="+", default=[0, 4, 8])
    ap.add_argument("--steps", type=int, default=None, help="instead of the case's own count")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "guess_history.jsonl"))
    a = ap.parse_args()
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host
    for case in a.cases:
        model, tol = model_of(case)
        for depth in a.depths:
            for run in range(a.runs):
                line = dict(case=case, depth=depth, run=run, tol=tol)
                if a.label:
                    line = dict(build=a.label, **line)
                line.update(one_run(E, host, model, depth, a.steps or CASES[case][1]))
                text = json.dumps(line)
                print(text[:400] + (" ..." if len(text) > 400 else ""), flush=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
