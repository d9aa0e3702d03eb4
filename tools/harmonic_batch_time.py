"""What a batch of harmonic systems in lock step costs beside the single solve, on one MI355X.

    python tools/harmonic_batch_time.py --mode iteration --case compare_to_Elmer|ec_src_move_hole [--iters 200]
    python tools/harmonic_batch_time.py --mode sweep
    [--out profiles/harmonic_batch.jsonl]

One JSON line per measurement, appended to --out and printed.

iteration   tol = 0, every system at --freq, the right-hand side of tools/harmonic_time.py (ones on the A rows of the
            non-conducting cells) in every system, x^ = 0.  The time of one lock-step iteration is
            (t(N) - t(N / 4)) / (N - N / 4), t the medians of three solves: the set-up and the polls drop out of the
            difference.  First the single solve and the batch of ONE system alternating, three runs a side (the rule of
            docs/rounds/r11.md: unchanged when the difference of the medians is within twice the larger min-max
            spread); then S = 1, 2, 4, 8, 16:
                ratio            t_batch(S) / (S t_single): below 1 is what lock step saves
                fraction_of_8tbs 306 B x n_pad x S / t_batch against 8 TB/s
            and device_bytes of the batch of 16.
sweep       compare_to_Elmer, 16 frequencies from 10 to 1000 Hz, logarithmically spaced, the model's own b^ (the phasors at
            50 Hz), tolerance and iteration limit, x^ = 0: one batch of 16 against 16 successive harmonic_setup +
            harmonic_solve on the same handle, the assembly excluded, the uploads included on both sides; three runs a
            side, alternating; the iteration counts per frequency."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "eddy_currents_3d_amd")) for p in sys.path if p):
    sys.path.insert(0, REPO)

CASES = {"compare_to_Elmer": None, "ec_src_move_hole": (256, 256, 60)}
BYTES_PER_ROW = 306   # per device row, iteration and RUNNING system: DESIGN.md section 18
SIZES = (1, 2, 4, 8, 16)


def model_of(case):
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(REPO, "tests", "golden", f"g4_{case}.npz"))
    m = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    return vxc.resample(m, *CASES[case]) if CASES[case] else m


def emit(out, line):
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text + "\n")


def spread(v):
    return max(v) - min(v)


def single_ms(s, zero, k):
    s.harmonic_upload("X", zero)
    it, _ = s.harmonic_solve(0.0, k - 1)
    assert it == k
    return s.harmonic_info()["ms"]


def batch_ms(s, S, zero, k):
    for q in range(S):
        s.harmonic_batch_upload(q, "X", zero)
    solved = s.harmonic_batch_solve(0.0, k - 1)
    assert [it for it, _ in solved] == [k] * S
    return s.harmonic_batch_info(0)["ms"]


def per_iteration(ms, lo, hi):
    return (statistics.median(ms[hi]) - statistics.median(ms[lo])) / (hi - lo)


def iteration(a):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import vxc
    t = vxc.domain_tables(model_of(a.case))
    omega = 2.0 * np.pi * a.freq
    hi, lo = a.iters, max(a.iters // 4, 1)
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        n, nC = s.n, int(np.asarray(t["geoPHYS"]).size)
        n_pad = int(s.vector_layout()["n_pad"])
        b = np.zeros(n)
        b[:2 * nC] = np.tile((np.asarray(t["geoPHYS_C"]).reshape(-1) == 0).astype(np.float64), 2)
        zero = np.zeros(n)
        s.harmonic_setup(omega)
        s.harmonic_upload("B", b)
        s.harmonic_batch_setup([omega])
        s.harmonic_batch_upload(0, "B", b)
        single_ms(s, zero, lo), batch_ms(s, 1, zero, lo)                       # (both sides warm)
        one = {lo: [], hi: []}
        bat = {lo: [], hi: []}
        for _ in range(3):                                                      # alternating, in one process
            for k in (lo, hi):
                one[k].append(single_ms(s, zero, k))
                bat[k].append(batch_ms(s, 1, zero, k))
        t_single, t_b1 = per_iteration(one, lo, hi), per_iteration(bat, lo, hi)
        # r11's rule on the solves of `hi` iterations, per iteration
        d = (statistics.median(bat[hi]) - statistics.median(one[hi])) / hi
        bar = 2.0 * max(spread(bat[hi]), spread(one[hi])) / hi
        emit(a.out, dict(tool="tools/harmonic_batch_time.py", mode="iteration", what="batch of 1 against the single solve",
                         case=a.case, n_pad=n_pad, iters=hi, single_ms_per_iter=t_single, batch1_ms_per_iter=t_b1,
                         single_ms_runs={str(k): v for k, v in one.items()}, batch1_ms_runs={str(k): v for k, v in bat.items()},
                         delta_median_ms_per_iter=d, twice_spread_ms_per_iter=bar, unchanged=bool(d <= bar)))
        for S in SIZES:
            s.harmonic_batch_setup([omega] * S)
            for q in range(S):
                s.harmonic_batch_upload(q, "B", b)
            ms = {lo: [], hi: []}
            for _ in range(3):
                for k in (lo, hi):
                    ms[k].append(batch_ms(s, S, zero, k))
            tb = per_iteration(ms, lo, hi)
            emit(a.out, dict(tool="tools/harmonic_batch_time.py", mode="iteration", case=a.case, n_pad=n_pad, systems=S, iters=hi,
                             batch_ms_per_iter=tb, batch_ms_runs={str(k): v for k, v in ms.items()},
                             single_ms_per_iter=t_single, ratio=tb / (S * t_single), bytes_per_row=BYTES_PER_ROW,
                             fraction_of_8tbs=BYTES_PER_ROW * n_pad * S / (tb * 1e-3) / 8e12,
                             device_bytes=s.harmonic_batch_info(0)["device_bytes"],
                             device_bytes_per_row_and_system=s.harmonic_batch_info(0)["device_bytes"] / (n_pad * S)))


def sweep(a):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    model = vxc.read_vxc(os.path.join(REPO, "tests", "golden", "g4_compare_to_Elmer.vxc"))
    t = vxc.domain_tables(model)
    n = 3 * model.vox.size + t["ncells0"]
    b = host.harmonic_rhs(host.SourceProgram(model, t), 50.0, n)
    freqs = [float(f) for f in np.logspace(1.0, 3.0, 16)]
    omegas = [2.0 * np.pi * f for f in freqs]
    tol, itmax = float(t["tol"]), int(t["itmax"])
    zero = np.zeros(n)
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        n_pad = int(s.vector_layout()["n_pad"])

        def batch():
            t0 = time.perf_counter()
            s.harmonic_batch_setup(omegas)
            for q in range(16):
                s.harmonic_batch_upload(q, "B", b)
                s.harmonic_batch_upload(q, "X", zero)
            solved = s.harmonic_batch_solve(tol, itmax)
            return time.perf_counter() - t0, [it for it, _ in solved], s.harmonic_batch_info(0)["ms"]

        def successive():
            t0 = time.perf_counter()
            its, ms = [], 0.0
            for w in omegas:
                s.harmonic_setup(w)
                s.harmonic_upload("B", b)
                s.harmonic_upload("X", zero)
                its.append(s.harmonic_solve(tol, itmax)[0])
                ms += s.harmonic_info()["ms"]
            return time.perf_counter() - t0, its, ms

        batch(), successive()                                                   # (both sides warm)
        runs = dict(batch=[], successive=[])
        for _ in range(3):
            runs["batch"].append(batch())
            runs["successive"].append(successive())
        assert runs["batch"][0][1] == runs["successive"][0][1], "the batch and the single solves disagree on the iterations"
        med = {k: statistics.median(r[0] for r in v) for k, v in runs.items()}
        solve = {k: statistics.median(r[2] for r in v) for k, v in runs.items()}
        emit(a.out, dict(tool="tools/harmonic_batch_time.py", mode="sweep", case="compare_to_Elmer", n_pad=n_pad, freqs=freqs, tol=tol,
                         itmax=itmax, iterations=runs["batch"][0][1], batch_s=med["batch"], successive_s=med["successive"],
                         batch_s_runs=[r[0] for r in runs["batch"]], successive_s_runs=[r[0] for r in runs["successive"]],
                         batch_solve_ms=solve["batch"], successive_solve_ms=solve["successive"],
                         speedup_wall=med["successive"] / med["batch"], speedup_solve=solve["successive"] / solve["batch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="iteration", choices=("iteration", "sweep"))
    ap.add_argument("--case", default="compare_to_Elmer", choices=list(CASES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--freq", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harmonic_batch.jsonl"))
    a = ap.parse_args()
    iteration(a) if a.mode == "iteration" else sweep(a)


if __name__ == "__main__":
    main()
