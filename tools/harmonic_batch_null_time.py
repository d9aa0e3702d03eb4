"""A frequency sweep below the floor, on one MI355X: the left null vectors inside a batch against the same frequencies
one after another through select and the single projected solve.

    python tools/harmonic_batch_null_time.py --mode sweep [--null-tol 1e-10] [--tol 1e-6] [--itmax N] [--runs 1]
    python tools/harmonic_batch_null_time.py --mode unused [--iters 200]
    [--out profiles/harmonic_batch_null.jsonl]

One JSON line per measurement, appended to --out and printed.

sweep    compare_to_Elmer, 16 frequencies from 10 to 1000 Hz, logarithmically spaced (the sweep of
         tools/harmonic_batch_time.py), the model's own b^ (the phasors at 50 Hz), x^ = 0, tol 1e-6, the model's iteration
         limit.  First the frequencies one after another: harmonic_batch_select, harmonic_set_null_projection,
         harmonic_solve -- the set-up time (setup_ms of the report) and the solve time (ms) per frequency; a frequency
         whose adjoint solve misses null_tol (EC3D_NULL_E_SETUP) is recorded and left out of both sides.  Then the rest
         in ONE batch with harmonic_batch_set_null_projection: the set-up's time, the solve's time, the iterations per
         frequency, how many converge, device_bytes.  Assembly and uploads are outside both.
unused   the feature unused: the unprojected batch of 16 at 50 Hz (tol 0, --iters iterations; the right-hand side of
         tools/harmonic_time.py), three solves, the times in ms -- to be run once per library (EC3D_LIB) by the job that
         alternates the two builds."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "eddy_currents_3d_amd")) for p in sys.path if p):
    sys.path.insert(0, REPO)

TOOL = "tools/harmonic_batch_null_time.py"


def emit(out, line):
    text = json.dumps(dict(tool=TOOL, **line))
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text + "\n")


def sweep(a):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    from eddy_currents_3d_amd.solver import NULL_E_SETUP
    model = vxc.read_vxc(os.path.join(REPO, "tests", "golden", "g4_compare_to_Elmer.vxc"))
    t = vxc.domain_tables(model)
    n = 3 * model.vox.size + t["ncells0"]
    b = host.harmonic_rhs(host.SourceProgram(model, t), 50.0, n)
    freqs = [float(f) for f in np.logspace(1.0, 3.0, 16)]
    itmax = int(t["itmax"]) if a.itmax is None else a.itmax
    zero = np.zeros(n)
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        n_pad = int(s.vector_layout()["n_pad"])

        def upload(fs):
            s.harmonic_batch_setup([2.0 * np.pi * f for f in fs])
            for q in range(len(fs)):
                s.harmonic_batch_upload(q, "B", b)
                s.harmonic_batch_upload(q, "X", zero)

        def successive(fs):
            """per frequency dict(freq, missed | setup_ms, solve_ms, iter, relres, adjoint) and the wall time"""
            upload(fs)
            recs = []
            t0 = time.perf_counter()
            for q, f in enumerate(fs):
                s.harmonic_batch_select(q)
                s.harmonic_set_null_projection(True, a.null_tol)
                try:
                    it, relres = s.harmonic_solve(a.tol, itmax)
                except E.EC3DError as e:
                    if e.status != NULL_E_SETUP:
                        raise
                    recs.append(dict(freq=f, missed=str(e)))
                    continue
                finally:
                    info = s.harmonic_null_projection()
                    s.harmonic_set_null_projection(False)
                recs.append(dict(freq=f, setup_ms=info["setup_ms"], solve_ms=s.harmonic_info()["ms"], iter=it, relres=relres,
                                 adjoint=[(c["iterations"], c["restarts"]) for c in info["components"]]))
            return recs, time.perf_counter() - t0

        def batch(fs):
            upload(fs)
            s.harmonic_batch_set_null_projection(True, a.null_tol)
            base = s.harmonic_batch_info(0)["device_bytes"]
            t0 = time.perf_counter()
            try:
                solved = s.harmonic_batch_solve(a.tol, itmax)
            finally:
                s.harmonic_batch_set_null_projection(False)
            wall = time.perf_counter() - t0
            infos = [s.harmonic_batch_null_projection(q) for q in range(len(fs))]
            return dict(wall_s=wall, setup_ms=infos[0]["setup_ms"], solve_ms=s.harmonic_batch_info(0)["ms"],
                        iterations=[it for it, _ in solved], relres=[r for _, r in solved],
                        adjoint=[[(c["iterations"], c["restarts"]) for c in q["components"]] for q in infos],
                        device_bytes=s.harmonic_batch_info(0)["device_bytes"], null_device_bytes=s.harmonic_batch_info(0)["device_bytes"] - base)

        first, _ = successive(freqs)
        missed = [r for r in first if "missed" in r]
        rest = [r["freq"] for r in first if "missed" not in r]
        for r in missed:
            emit(a.out, dict(mode="sweep", what="adjoint solve missed null_tol", case="compare_to_Elmer", null_tol=a.null_tol,
                             freq=r["freq"], text=r["missed"]))
        if not rest:
            return
        for run in range(a.runs):
            one = batch(rest)
            recs, wall = successive(rest)
            conv_b = sum(1 for it in one["iterations"] if it <= itmax)
            conv_s = sum(1 for r in recs if r["iter"] <= itmax)
            emit(a.out, dict(mode="sweep", case="compare_to_Elmer", n_pad=n_pad, run=run, tol=a.tol, null_tol=a.null_tol, itmax=itmax,
                             freqs=rest, left_out=[r["freq"] for r in missed],
                             batch=dict(one, converged=conv_b, setup_plus_solve_ms=one["setup_ms"] + one["solve_ms"]),
                             successive=dict(wall_s=wall, setup_ms=sum(r["setup_ms"] for r in recs),
                                             solve_ms=sum(r["solve_ms"] for r in recs), iterations=[r["iter"] for r in recs],
                                             relres=[r["relres"] for r in recs], adjoint=[r["adjoint"] for r in recs],
                                             converged=conv_s,
                                             setup_plus_solve_ms=sum(r["setup_ms"] + r["solve_ms"] for r in recs)),
                             same_iterations=one["iterations"] == [r["iter"] for r in recs]))


def unused(a):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(REPO, "tests", "golden", "g4_compare_to_Elmer.npz"))
    m = vxc.VxcModel(g["vox"], [str(q) for q in g["names"]], float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    t = vxc.domain_tables(m)
    omega = 2.0 * np.pi * 50.0
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        n, nC = s.n, int(np.asarray(t["geoPHYS"]).size)
        b = np.zeros(n)
        b[:2 * nC] = np.tile((np.asarray(t["geoPHYS_C"]).reshape(-1) == 0).astype(np.float64), 2)
        zero = np.zeros(n)
        s.harmonic_batch_setup([omega] * 16)
        for q in range(16):
            s.harmonic_batch_upload(q, "B", b)
        ms = []
        for run in range(4):                                                    # (the first one warms)
            for q in range(16):
                s.harmonic_batch_upload(q, "X", zero)
            solved = s.harmonic_batch_solve(0.0, a.iters - 1)
            assert [it for it, _ in solved] == [a.iters] * 16
            ms.append(s.harmonic_batch_info(0)["ms"])
        emit(a.out, dict(mode="unused", what="unprojected batch of 16, 50 Hz", case="compare_to_Elmer", iters=a.iters,
                         library=os.environ.get("EC3D_LIB") or "this tree", ms_runs=ms[1:],
                         ms_per_iter=[v / a.iters for v in ms[1:]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="sweep", choices=("sweep", "unused"))
    ap.add_argument("--null-tol", type=float, default=1e-10)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--itmax", type=int, default=None)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harmonic_batch_null.jsonl"))
    a = ap.parse_args()
    sweep(a) if a.mode == "sweep" else unused(a)


if __name__ == "__main__":
    main()
