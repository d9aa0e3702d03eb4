"""The reference's time loop at tolerances below the reference's, with and without the left-null-vector projection
(ec3d_set_null_projection).

    python tools/tight_tolerance_time_loop.py [--cases LIM ec_src_move_hole] [--tols model 1e-6 1e-8] [--modes off on]
                                              [--steps N] [--runs R] [--itmax M] [--null-tol Y] [--precond block-mg]
                                              [--null-precond none|block-mg|block-mg-a] [--label TEXT]
                                              [--out profiles/null_projection.jsonl]
    python tools/tight_tolerance_time_loop.py --config3 [--label TEXT]
    python tools/tight_tolerance_time_loop.py --setup-only [--cases ..] [--null-tol Y ..] [--null-precond KIND ..]

One JSON line per case, tolerance, mode and run, appended to --out and printed: iterations of every step, the wall time
of the loop (host.run without output, the assembly and -- with the projection -- its set-up included) and of the solves
alone, every step's true residual (ec3d_true_residual) and, with the projection, every step's PROJECTED true residual
||P (b - A x)|| / ||b|| -- b - A x through ec3d_spmv on the device, P = I - Q Q^T on the host with the handle's own
vectors (ec3d_left_null_vector) -- and the set-up: per component the adjoint solve's iterations and ||A^T w|| / ||w||,
and the milliseconds it took.  LIM: the shipped input (tests/golden/g4_LIM), 200 steps; ec_src_move_hole: the shipped
input resampled to 256 x 256 x 60 (vxc.resample, as tests/test_gpu_fullsize.py), 20 steps.  --itmax caps a solve's
iterations (default: the model's): without the projection a tolerance below the floor runs every step into it.
--precond block-mg: the preconditioned iteration around the same projection.
Mode off never calls ec3d_set_null_projection, so the tool also runs on a build that has no such call (EC3D_LIB names
its library, --label the build): that is how the default loop is compared with the parent commit.

--null-precond: the preconditioner of the adjoint solves (ec3d_set_null_precond); the set-up record then also holds its
kind, the hierarchy's levels and hierarchy_ms.  A set-up that misses null_tol (EC3D_NULL_E_SETUP) is recorded as
setup_failed with the library's text, not raised.
--setup-only: no time loop -- per case, null_tol and preconditioner one line with the assembly, the set-up (adjoint
iterations per component, whether null_tol was reached, ||A^T w|| / ||w||, setup_ms, hierarchy_ms) and nothing else.

--config3: one solve of BASELINE config 3 at 256^3 (tests/test_gpu_av256.py's model) at tol 5e-4, projection off and
on, each compared with the reference's converged step in tests/golden/g7x_*: the fixture holds a count-sketch and probes
of x, not x, so the distance reported is that of the sketches and of the probes on the A blocks."""
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

CASES = {"LIM": (None, 200), "ec_src_move_hole": ((256, 256, 60), 20)}


def model_of(case):
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(REPO, "tests", "golden", f"g4_{case}.npz"))
    m = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    dims = CASES[case][0]
    m = vxc.resample(m, *dims) if dims else m
    return m, float(g["tol"]), int(vxc.domain_tables(m)["itmax"])


def projected_residual(s, W):
    """||P (b - A x)|| / ||b|| of the resident vectors; W: the handle's orthonormal left null vectors."""
    b = s.download("B")
    r = b - s.spmv(s.download("X"))
    c = [w @ r for w in W]
    for ci, w in zip(c, W):
        r = r - ci * w
    return float(np.linalg.norm(r) / np.linalg.norm(b))


def setup_record(s, setup):
    kind, levels, hms = s.null_precond() if hasattr(s, "null_precond") else ("none", [], 0.0)
    return dict(found=setup["found"], kept=setup["kept"], dropped=setup["dropped"], ms=round(setup["setup_ms"], 3),
                null_tol=setup["null_tol"], components=setup["components"], null_precond=kind, levels=len(levels),
                hierarchy_ms=round(hms, 3))


def setup_only(E, model, null_tol, null_precond):
    """Assembly and the null set-up alone: what the adjoint solves cost and whether they reach null_tol."""
    from eddy_currents_3d_amd import vxc
    t = vxc.domain_tables(model)
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        s.set_null_projection(True, **({} if null_tol is None else {"null_tol": null_tol}),
                              **({} if null_precond is None else {"precond": null_precond}))
        t0 = time.perf_counter()
        try:
            s.left_null_vector(0)
        except E.EC3DError as e:
            if getattr(e, "status", None) != E.solver.NULL_E_SETUP:
                raise
            kind, levels, hms = s.null_precond()
            return dict(n=int(s.n), reached=False, setup_failed=str(e), wall_s=round(time.perf_counter() - t0, 4),
                        null_precond=kind)
        return dict(n=int(s.n), reached=True, wall_s=round(time.perf_counter() - t0, 4),
                    setup=setup_record(s, s.null_projection()))


def one_run(E, host, model, tol, itmax, on, steps, null_tol=None, precond=None, null_precond=None):
    res, pres, removed, solve_s, W = [], [], [], [0.0], []
    with E.EC3DSolver() as s:
        inner = s.solve_resident

        def timed_solve(t_, m_, *a, **k):
            t = time.perf_counter()
            out = inner(t_, itmax if itmax else m_, *a, **k)
            solve_s[0] += time.perf_counter() - t
            return out
        s.solve_resident = timed_solve

        def on_solved(k, s, info):
            res.append(float(s.true_residual()[0]))
            if on:
                if not W:
                    W.extend(s.left_null_vector(i) for i in range(s.null_projection()["kept"]))
                pres.append(projected_residual(s, W))
                removed.append(info["null"]["removed"])
        t0 = time.perf_counter()
        extra = dict(null_projection=True, tol=tol, null_tol=null_tol) if on else dict(tol=tol) if tol is not None else {}
        if precond:
            extra["precond"] = precond
        if on and null_precond:
            extra["null_precond"] = null_precond
        try:
            log = host.run(model, s, steps=steps, on_solved=on_solved, **extra)
        except E.EC3DError as e:
            if getattr(e, "status", None) != E.solver.NULL_E_SETUP:
                raise
            return dict(n=int(s.n), setup_failed=str(e), wall_s=round(time.perf_counter() - t0, 4))
        s.synchronize()
        wall = time.perf_counter() - t0
        n = int(s.n)
        setup_rec = setup_record(s, s.null_projection()) if on else None
    out = dict(n=n, steps=len(log), iters=[int(i["iter"]) for i in log], wall_s=round(wall, 4), solve_s=round(solve_s[0], 4),
               true_residual_max=max(res), true_residual=[float(f"{r:.4e}") for r in res])
    out["iters_total"] = sum(out["iters"])
    if on:
        out["projected_residual_max"] = max(pres)
        out["projected_residual"] = [float(f"{r:.4e}") for r in pres]
        out["removed"] = [float(f"{r:.4e}") for r in removed]
        out["setup"] = setup_rec
        out["wall_s_note"] = "includes the host-side projected residual of every step"
    return out


def config3(E, host, label, out_path, null_tol=None):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from oracle import oracle as O
    from test_gpu_av256 import _model
    model, gx = _model()
    nA = 3 * int(np.prod([int(v) for v in gx["dims"]]))
    a = gx["probes"] < nA
    for on in (False, True):
        got = {}

        def on_solved(k, s, info):
            x = s.download("X")
            got.update(iter=int(info["iter"]), res=float(s.true_residual()[0]), sketch=O.count_sketch(x), probe=x[gx["probes"]])
        with E.EC3DSolver() as s:
            t0 = time.perf_counter()
            host.run(model, s, steps=1, on_solved=on_solved, tol=5e-4,
                     **(dict(null_projection=True, null_tol=null_tol) if on else {}))
            wall = time.perf_counter() - t0
            setup = s.null_projection() if on else None
        line = dict(case="config3_256", tol=5e-4, mode="on" if on else "off", iter=got["iter"], true_residual=got["res"],
                    wall_s=round(wall, 3),
                    sketch_distance=float(np.linalg.norm(got["sketch"] - gx["xsketch_ref"]) / np.linalg.norm(gx["xsketch_ref"])),
                    a_probe_distance=float(np.abs(got["probe"][a] - gx["xprobe"][a]).max() / np.abs(gx["xprobe"][a]).max()),
                    reference_tol=float(gx["tol"]))
        if on:
            line["setup"] = dict(kept=setup["kept"], ms=round(setup["setup_ms"], 3), null_tol=setup["null_tol"],
                                 components=setup["components"])
        if label:
            line = dict(build=label, **line)
        emit(line, out_path)


def emit(line, out_path):
    text = json.dumps(line)
    print(text[:500] + (" ..." if len(text) > 500 else ""), flush=True)
    with open(out_path, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--tols", nargs="+", default=["model", "1e-6", "1e-8"])
    ap.add_argument("--modes", nargs="+", default=["off", "on"], choices=["off", "on"])
    ap.add_argument("--steps", type=int, default=None, help="instead of the case's own count")
    ap.add_argument("--itmax", type=int, default=None, help="cap of a solve's iterations instead of the model's")
    ap.add_argument("--null-tol", type=float, nargs="+", default=[None],
                    help="accuracy of the adjoint solves instead of 1e-10 (--setup-only: one line per value)")
    ap.add_argument("--null-precond", nargs="+", default=[None], choices=["none", "block-mg", "block-mg-a"],
                    help="preconditioner of the adjoint solves (--setup-only: one line per value)")
    ap.add_argument("--setup-only", action="store_true")
    ap.add_argument("--precond", default=None, choices=["block-mg"], help="host.run(..., precond=...) on top")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--label", default=None)
    ap.add_argument("--config3", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "null_projection.jsonl"))
    a = ap.parse_args()
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host
    if a.config3:
        return config3(E, host, a.label, a.out, a.null_tol[0])
    for case in a.cases:
        model, model_tol, model_itmax = model_of(case)
        if a.setup_only:
            for null_tol in a.null_tol:
                for kind in a.null_precond:
                    line = dict(case=case, setup_only=True, null_tol=null_tol or 1e-10, null_precond=kind or "none")
                    if a.label:
                        line = dict(build=a.label, **line)
                    line.update(setup_only(E, model, null_tol, kind))
                    emit(line, a.out)
            continue
        for tol_text in a.tols:
            tol = None if tol_text == "model" else float(tol_text)
            for mode in a.modes:
                for run in range(a.runs):
                    line = dict(case=case, tol=model_tol if tol is None else tol, mode=mode, run=run,
                                itmax=a.itmax or model_itmax, **({"precond": a.precond} if a.precond else {}),
                                **({"null_precond": a.null_precond[0]} if a.null_precond[0] else {}))
                    if a.label:
                        line = dict(build=a.label, **line)
                    line.update(one_run(E, host, model, tol, a.itmax, mode == "on", a.steps or CASES[case][1], a.null_tol[0], a.precond,
                                        a.null_precond[0]))
                    emit(line, a.out)


if __name__ == "__main__":
    main()
