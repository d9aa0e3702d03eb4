"""One harmonic solve against the time loop's periodic steady state on compare_to_Elmer (TEAM 7, 50 Hz), one MI355X.

    python tools/harmonic_vs_transient.py [--periods 5] [--harmonic-tol X [--null-projection]] [--out profiles/harmonic.jsonl]

* the harmonic solve at 50 Hz at the model's tolerance: iterations, seconds (assembly excluded and included), the true
  residual; and the true residual reached at tol = 1e-6 and 1e-8 (itmax 20000);
* the time loop over --periods periods at the model's dt and at dt / 2, A recorded at the probes of "Line X" -- the line
  along x through the plate's centre in the plate's top plane -- after every step; the 50 Hz Fourier fit of the last period,
  a^ = (2 / N) sum A(T_n) exp(-j omega T_n), against the harmonic A^ there: |fit - A^| / |A^| over the line's three
  components; beside it the loop's own period-to-period change |fit(last) - fit(last - 1)| / |fit(last)|.
--harmonic-tol X: the harmonic side at tolerance X (itmax 20000) instead of the model's, with --null-projection below
the floor; the time loop keeps the model's tolerance.
Exact agreement is not expected: the U rows are backward-differenced, the A rows trapezoidal, and the reference zeroes Uaf
on cel_bnd* after every step.  One JSON line appended to --out and printed."""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "eddy_currents_3d_amd")) for p in sys.path if p):
    sys.path.insert(0, REPO)

FREQ = 50.0


def model_with(names_edit=None):
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(REPO, "tests", "golden", "g4_compare_to_Elmer.npz"))
    names = [str(s) for s in g["names"]]
    if names_edit:
        names = [names_edit(s) for s in names]
    return vxc.VxcModel(g["vox"], names, float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))


def line_x(geoC):
    from eddy_currents_3d_amd.probes import probe_line
    sdz, sdy, sdx = geoC.shape
    k = int(np.flatnonzero((geoC != 0).any(axis=(1, 2))).max())
    jj = np.flatnonzero((geoC[k] != 0).any(axis=1))
    jc = int(jj.min() + jj.max()) // 2
    return probe_line((2, jc, k), (sdx - 3, jc, k), (sdx, sdy, sdz))


def fit(T, A, omega):
    """the 50 Hz Fourier coefficient of the samples A[n] at times T[n] (one period, equally spaced)"""
    return (2.0 / len(T)) * np.tensordot(np.exp(-1j * omega * np.asarray(T)), A, axes=(0, 0))


def transient(model, cells, periods):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    t = vxc.domain_tables(model)
    dt = float(t["dt"])
    per = int(round(1.0 / (FREQ * dt)))
    steps = periods * per
    with E.EC3DSolver() as s:
        t0 = time.perf_counter()
        log = host.run(model, s, steps=steps, probes=cells)
        s.synchronize()
        wall = time.perf_counter() - t0
    T = np.array([i["T"] for i in log])
    A = np.stack([i["probes"][:, 0:3] for i in log])               # (steps, nprobes, 3)
    omega = 2.0 * np.pi * FREQ
    last, prev = fit(T[-per:], A[-per:], omega), fit(T[-2 * per:-per], A[-2 * per:-per], omega)
    return dict(dt=dt, steps=steps, seconds=wall, iters_total=int(sum(i["iter"] for i in log)), fit=last,
                fit_shifted=fit(T[-per:] + dt, A[-per:], omega),     # had step k's fields belonged to T_k + dt
                period_change=float(np.linalg.norm(last - prev) / np.linalg.norm(last)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=5)
    ap.add_argument("--harmonic-tol", type=float, default=None)
    ap.add_argument("--null-projection", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harmonic.jsonl"))
    a = ap.parse_args()
    assert a.periods >= 3
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    model = model_with()
    t = vxc.domain_tables(model)
    cells = line_x(np.asarray(t["geoPHYS_C"]))
    line = dict(tool="tools/harmonic_vs_transient.py", case="compare_to_Elmer", freq=FREQ, nprobes=int(len(cells)),
                tol=float(t["tol"]))
    with E.EC3DSolver() as s:
        t0 = time.perf_counter()
        r = host.run_harmonic(model, s, FREQ, probes=cells, tol=a.harmonic_tol, itmax=20000 if a.harmonic_tol else None,
                              null_projection=a.null_projection)
        if a.harmonic_tol:
            line.update(harmonic_tol=a.harmonic_tol, null_projection=a.null_projection)
        if a.null_projection:
            line.update(harmonic_projected_residual=r["projected_residual"], removed=r["removed"],
                        adjoint_iterations=[c["iterations"] for c in r["null"]["components"]])
        line.update(harmonic_iter=r["iter"], harmonic_restarts=r["info"]["restarts"], harmonic_solve_s=r["info"]["ms"] * 1e-3,
                    harmonic_wall_s=time.perf_counter() - t0, harmonic_relres=r["relres"], harmonic_true_residual=r["true_residual"])
        ah = r["probes"][:, 0:3]
        tight = {}
        for tol in (1e-6, 1e-8):
            s.harmonic_upload("X", np.zeros(s.n))
            it, rel = s.harmonic_solve(tol, 20000)
            tight[repr(tol)] = dict(iter=it, relres=rel, true_residual=s.harmonic_true_residual()[0], ms=s.harmonic_info()["ms"])
        line["tight"] = tight
    for label, edit in (("dt", None), ("dt_half", lambda s: re.sub(r"(?i)step=1m", "step=0.5m", s))):
        q = transient(model_with(edit), cells, a.periods)
        f = q.pop("fit")
        q["difference_to_harmonic"] = float(np.linalg.norm(f - ah) / np.linalg.norm(ah))
        g = q.pop("fit_shifted")
        q["difference_if_fields_belong_to_T_plus_dt"] = float(np.linalg.norm(g - ah) / np.linalg.norm(ah))
        q["amplitude_ratio"] = float(np.linalg.norm(f) / np.linalg.norm(ah))
        line[label] = q
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
