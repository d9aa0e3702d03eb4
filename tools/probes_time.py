"""What probes cost in the reference's time loop, on one MI355X.

    python tools/probes_time.py --case LIM|ec_src_move_hole --variant none|lines|plane|vtk [--steps N] [--label TEXT]
                                [--out profiles/probes.jsonl]

One run per process: host.run without output files, one JSON line appended to --out and printed.  LIM: the shipped
input (tests/golden/g4_LIM), 200 steps; ec_src_move_hole: the shipped input resampled to 256 x 256 x 60, 20 steps.
    none    no probes (never touches a probe call, so it also runs on a build that has none: --label names the build,
            a PYTHONPATH that names another build of the package wins -- that is how the parent commit is compared)
    lines   two lines across the plate's top surface through its centre, along x and along y, plus the centre cell,
            recorded every step (host.run(..., probes=...)), the record read once at the end
    plane   every cell of the plate's top surface plane, likewise
    vtk     the old way to the same numbers: EC3DSolver.vtk_fields of the whole box after every step (no file written)
The line holds the wall time of the loop (from the first right-hand side, the device drained, to the drained device after
the last step and the reading of the record), the iterations of every step, the probe count, and -- with probes -- the
host time inside EC3DSolver.probe_record per call and inside the reads; `vtk`: inside vtk_fields per call."""
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
    return vxc.resample(m, *dims) if dims else m


def plate_probes(geoC, variant):
    """The probe cells of a variant from the conductor mask [k, j, i]: the plate's top plane, its extent there."""
    from eddy_currents_3d_amd.probes import probe_box, probe_line
    sdz, sdy, sdx = geoC.shape
    dims = (sdx, sdy, sdz)
    k = int(np.flatnonzero((geoC != 0).any(axis=(1, 2))).max())
    jj = np.flatnonzero((geoC[k] != 0).any(axis=1))
    ii = np.flatnonzero((geoC[k] != 0).any(axis=0))
    i0, i1, j0, j1 = int(ii.min()), int(ii.max()), int(jj.min()), int(jj.max())
    ic, jc = (i0 + i1) // 2, (j0 + j1) // 2
    if variant == "plane":
        return probe_box((i0, j0, k), (i1, j1, k), dims)
    return np.concatenate([probe_line((i0, jc, k), (i1, jc, k), dims), probe_line((ic, j0, k), (ic, j1, k), dims),
                           probe_box((ic, jc, k), (ic, jc, k), dims)])


def one_run(case, variant, steps):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    model = model_of(case)
    tab = vxc.domain_tables(model)
    spent = dict(record=0.0, read=0.0, vtk=0.0)
    t = {}
    kw = {}
    cells = None
    if variant in ("lines", "plane"):
        cells = plate_probes(np.asarray(tab["geoPHYS_C"]), variant)
        kw = dict(probes=cells)

    def timed(name, inner):
        def f(*a, **k):
            t0 = time.perf_counter()
            out = inner(*a, **k)
            spent[name] += time.perf_counter() - t0
            return out
        return f

    def on_rhs(k, s, info):
        if k == 0:
            s.synchronize()
            t["loop0"] = time.perf_counter()

    def on_step(k, s, info):
        if variant == "vtk":
            s.vtk_fields(tab["delta"], int(model.vox.size), tab["ncells0"] > 0)

    with E.EC3DSolver() as s:
        if cells is not None:
            s.probe_record = timed("record", s.probe_record)
            s.probe_read = timed("read", s.probe_read)
        if variant == "vtk":
            s.vtk_fields = timed("vtk", s.vtk_fields)
        t0 = time.perf_counter()
        log = host.run(model, s, steps=steps, on_rhs=on_rhs, on_step=on_step, **kw)
        s.synchronize()
        t1 = time.perf_counter()
        n = int(s.n)
        info = s.probes() if cells is not None else None
    out = dict(n=n, steps=len(log), iters=[int(i["iter"]) for i in log], iters_total=int(sum(i["iter"] for i in log)),
               wall_s=round(t1 - t0, 5), loop_s=round(t1 - t["loop0"], 5), loop_ms_per_step=1e3 * (t1 - t["loop0"]) / len(log))
    if cells is not None:
        out.update(nprobes=int(len(cells)), capacity=info["capacity"], device_bytes=info["device_bytes"],
                   record_us_per_call=1e6 * spent["record"] / len(log), read_ms_total=1e3 * spent["read"],
                   checksum=float(np.sum([np.nansum(i["probes"]) for i in log])))
    if variant == "vtk":
        out.update(vtk_fields_ms_per_call=1e3 * spent["vtk"] / len(log))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="LIM", choices=list(CASES))
    ap.add_argument("--variant", default="none", choices=("none", "lines", "plane", "vtk"))
    ap.add_argument("--steps", type=int, default=None, help="instead of the case's own count")
    ap.add_argument("--label", default=None)
    ap.add_argument("--run", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "probes.jsonl"))
    a = ap.parse_args()
    line = dict(tool="tools/probes_time.py", case=a.case, variant=a.variant, run=a.run)
    if a.label:
        line = dict(build=a.label, **line)
    line.update(one_run(a.case, a.variant, a.steps or CASES[a.case][1]))
    text = json.dumps(line)
    print(text[:600] + (" ..." if len(text) > 600 else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
