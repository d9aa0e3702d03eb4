"""Time per iteration of the complex (time-harmonic) solve beside the real iteration of the same handle, on one MI355X.

    python tools/harmonic_time.py --case compare_to_Elmer|ec_src_move_hole [--iters N] [--out profiles/harmonic.jsonl]

compare_to_Elmer: the shipped input (tests/golden/g4_compare_to_Elmer); ec_src_move_hole: the shipped input resampled to
256 x 256 x 60 (only its matrix is used: its sources move, which the harmonic solve refuses).  One JSON line appended to
--out and printed:
    harmonic_ms_per_iter   (t(N) - t(N / 4)) / (N - N / 4) of ec3d_harmonic_solve(tol = 0, itmax = k - 1), three runs each, the
                           medians: the set-up (residual launch) and the polls drop out of the difference
    real_ms_per_iter       ec3d_time_iterations of the same handle (the real five- or three-launch iteration), median of three
    bytes_per_row          the byte model of DESIGN.md section 18 (306 B per device row and iteration)
    fraction_of_8tbs       bytes_per_row * n_pad / harmonic time / 8e12
The right-hand side is the same in both: ones on the A rows of the non-conducting cells."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "eddy_currents_3d_amd")) for p in sys.path if p):
    sys.path.insert(0, REPO)

CASES = {"compare_to_Elmer": None, "ec_src_move_hole": (256, 256, 60)}
BYTES_PER_ROW = 306   # 49 (AP = A P) + 48 (S) + 33 (AS = A S) + 112 (X, R) + 64 (P): DESIGN.md section 18


def model_of(case):
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(REPO, "tests", "golden", f"g4_{case}.npz"))
    m = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    return vxc.resample(m, *CASES[case]) if CASES[case] else m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="compare_to_Elmer", choices=list(CASES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--freq", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harmonic.jsonl"))
    a = ap.parse_args()
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import vxc
    t = vxc.domain_tables(model_of(a.case))
    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        n, nC = s.n, int(np.asarray(t["geoPHYS"]).size)
        b = np.zeros(n)
        b[:2 * nC] = np.tile((np.asarray(t["geoPHYS_C"]).reshape(-1) == 0).astype(np.float64), 2)
        s.upload("B", b)
        s.upload("X", np.zeros(n))
        real = [s.time_iterations(a.iters) / a.iters for _ in range(3)]
        s.harmonic_setup(2.0 * np.pi * a.freq)
        s.harmonic_upload("B", b)
        lo = max(a.iters // 4, 1)
        ms = {lo: [], a.iters: []}
        for _ in range(3):
            for k in (lo, a.iters):
                s.harmonic_upload("X", np.zeros(n))
                it, _ = s.harmonic_solve(0.0, k - 1)
                assert it == k
                ms[k].append(s.harmonic_info()["ms"])
        h = (statistics.median(ms[a.iters]) - statistics.median(ms[lo])) / (a.iters - lo)
        n_pad = s.vector_layout()["n_pad"]
        line = dict(tool="tools/harmonic_time.py", case=a.case, n=int(n), n_pad=int(n_pad), classes=int(s.info.dict_classes),
                    iters=a.iters, harmonic_ms_per_iter=h, harmonic_ms_runs={str(k): v for k, v in ms.items()},
                    real_ms_per_iter=statistics.median(real), real_ms_runs=real, ratio=h / statistics.median(real),
                    bytes_per_row=BYTES_PER_ROW, fraction_of_8tbs=BYTES_PER_ROW * n_pad / (h * 1e-3) / 8e12,
                    device_bytes=s.harmonic_info()["device_bytes"])
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
