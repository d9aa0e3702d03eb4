"""An energy balance over a shipped model's time loop, from the device's own integrals, on one MI355X.

    python tools/energy_balance.py [--model tests/golden/g4_LIM.vxc] [--steps 200] [--out profiles/energy_balance.jsonl]

host.run(..., integrals=True, energy=True); per step k >= 1, with Lambda = aj_source (the sum of the listed domains'
linkages), W = energy_b and P = the sum of joule_w:

    source   -(Lambda_k - Lambda_{k-1}) / dt         (s * Jaf is MINUS the source current density)
    stored   (W_k - W_{k-1}) / dt
    balance  stored + P_k

and the static identity of a linear medium, W = 1/2 * integral(A.J), as the ratio W_k / (0.5 * (aj_eddy_k - aj_source_k)).
An observation, not a test: the curl is clamped at the faces and the time derivative is first order.  One JSON line:
the largest relative mismatches (relative to the largest |balance| of the run) of `source` and of `source / 2` against
`balance`, and the range of the static ratio."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=os.path.join(REPO, "tests", "golden", "g4_LIM.vxc"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "energy_balance.jsonl"))
    a = ap.parse_args(argv)
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    model = vxc.read_vxc(a.model)
    dt = float(vxc.domain_tables(model)["dt"])
    with E.EC3DSolver() as s:
        log = host.run(model, s, steps=a.steps, integrals=True, energy=True)
    W = np.array([i["energy"]["energy_b"] for i in log])
    src = np.array([i["energy"]["aj_source"] for i in log])
    eddy = np.array([i["energy"]["aj_eddy"] for i in log])
    P = np.array([sum(r["joule_w"] for r in i["integrals"]) for i in log])
    source = -(src[1:] - src[:-1]) / dt
    stored = (W[1:] - W[:-1]) / dt
    balance = stored + P[1:]
    scale = float(np.abs(balance).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        static = W / (0.5 * (eddy - src))
    static = static[np.isfinite(static)]
    row = dict(tool="tools/energy_balance.py", model=os.path.basename(a.model), steps=len(log), dt=dt,
               max_abs_balance_w=scale, max_joule_w=float(P.max()), max_energy_b=float(W.max()),
               mismatch_source=float(np.abs(source - balance).max() / scale),
               mismatch_half_source=float(np.abs(0.5 * source - balance).max() / scale),
               static_ratio_min=float(static.min()), static_ratio_max=float(static.max()),
               static_ratio_median=float(np.median(static)),
               first_steps=[dict(step=k + 1, source=float(source[k]), stored=float(stored[k]), joule=float(P[k + 1]))
                            for k in range(min(5, len(source)))])
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
