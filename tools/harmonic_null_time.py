"""The harmonic solve below its floor on compare_to_Elmer at 50 Hz, on one MI355X: the set-up of the complex left null
vectors and projected solves beside plain ones.

    python tools/harmonic_null_time.py [--freq 50] [--itmax 20000] [--out profiles/harmonic_null.jsonl]

One JSON line per measurement, appended to --out and printed:
    kind = "setup"   per null_tol (1e-8, 1e-10): the adjoint solve's iterations and restarts, ||A^H w|| / ||w||, the
                     set-up's wall time and the device bytes it added (ec3d_get_harmonic before and after)
    kind = "solve"   per tol (5e-3, 1e-4, 1e-6, 1e-8), projection off and on (null_tol 1e-10; 1e-6 also with 1e-8): iter,
                     restarts, the solve's wall time, the true and -- with the handle's Q -- the projected residual of
                     x^, and removed
b^ comes from the model's sources (host.harmonic_rhs), every solve starts from x^ = 0."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "eddy_currents_3d_amd")) for p in sys.path if p):
    sys.path.insert(0, REPO)

TOLS = (5e-3, 1e-4, 1e-6, 1e-8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--freq", type=float, default=50.0)
    ap.add_argument("--itmax", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harmonic_null.jsonl"))
    a = ap.parse_args()
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    model = vxc.read_vxc(os.path.join(REPO, "tests", "golden", "g4_compare_to_Elmer.vxc"))
    t = vxc.domain_tables(model)
    n = 3 * model.vox.size + t["ncells0"]
    b = host.harmonic_rhs(host.SourceProgram(model, t), a.freq, n)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(**rec):
        text = json.dumps(dict(tool="tools/harmonic_null_time.py", case="compare_to_Elmer", freq=a.freq, n=int(n), **rec))
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    with E.EC3DSolver() as s:
        s.assemble(t["geoPHYS"], t["geoPHYS_C"], t["valPHYS"], t["BND"], t["delta"], t["dt"])
        s.harmonic_setup(2.0 * np.pi * a.freq)
        s.harmonic_upload("B", b)
        base = s.harmonic_info()["device_bytes"]

        def solve(tol, **rec):
            s.harmonic_upload("X", np.zeros(n))
            it, relres = s.harmonic_solve(tol, a.itmax)
            info = s.harmonic_info()
            true, _ = s.harmonic_true_residual()
            q = s.harmonic_null_projection()
            if q["on"]:
                rec["projected_residual"], rec["removed"] = s.harmonic_projected_residual()
            emit(kind="solve", tol=tol, itmax=a.itmax, iter=it, restarts=info["restarts"], stop_kind=info["stop_kind"],
                 relres=relres, ms=info["ms"], true_residual=true, projection=q["on"], **rec)

        for tol in TOLS:
            solve(tol)
        for null_tol in (1e-8, 1e-10):
            s.harmonic_set_null_projection(True, null_tol)
            try:
                s.harmonic_left_null_vector(0)
            except E.EC3DError as e:
                emit(kind="setup", null_tol=null_tol, error=str(e))
                continue
            q = s.harmonic_null_projection()
            emit(kind="setup", null_tol=null_tol, found=q["found"], kept=q["kept"], setup_ms=q["setup_ms"],
                 components=q["components"], cap=int(20.0 * np.cbrt(float(n))) + 2000,
                 device_bytes=s.harmonic_info()["device_bytes"] - base)
            for tol in (TOLS if null_tol == 1e-10 else (1e-6,)):
                solve(tol, null_tol=null_tol)


if __name__ == "__main__":
    main()
