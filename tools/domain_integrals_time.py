"""Cost of ec3d_domain_integrals beside the time step it follows, on one MI355X.

    python tools/domain_integrals_time.py [--out profiles/domain_integrals.jsonl] [--grids 256x256x60 256x256x256]

ec_src_move_hole (tests/golden/g4_ec_src_move_hole) resampled to config 3's grids, as tests/test_gpu_fullsize.py and
tests/test_gpu_av256.py build them.  One time step of host.run; the step's solve_resident is timed on the host (the
device drained in front of it); after the post-update, 3 warm-up calls of EC3DSolver.domain_integrals' entry point
and 20 timed ones, host wall-clock around the synchronous call.  One JSON line per grid: the median call, the solve,
their ratio, and the bytes per second the call reaches under its byte model (15 gathered doubles + the 4-byte list
entry per conductor cell = 124 B)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
BYTES_PER_CELL = 15 * 8 + 4


def model_of(dims):
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(GOLDEN, "g4_ec_src_move_hole.npz"))
    small = vxc.VxcModel(g["vox"], [str(s) for s in g["names"]], float(str(g["lattice_dim"])),
                         tuple(float(x) for x in g["adj"]))
    return vxc.resample(small, *dims)


def measure(dims, calls=20, warmup=3):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    from eddy_currents_3d_amd.solver import DomainIntegral
    model = model_of(dims)
    delta = np.ascontiguousarray(vxc.domain_tables(model)["delta"], np.float64)
    row = dict(grid="ec_src_move_hole %dx%dx%d" % tuple(dims))
    t = {}

    def on_rhs(k, s, info):
        s.L.ec3d_device_synchronize(s.h)
        t["solve0"] = time.perf_counter()

    def on_solved(k, s, info):
        t["solve1"] = time.perf_counter()

    def on_step(k, s, info):
        n = C.c_int32(0)
        assert s.L.ec3d_domain_integrals(s.h, delta, 0, C.byref(n), None) == 0
        out = (DomainIntegral * max(n.value, 1))()
        times = []
        for i in range(warmup + calls):
            t0 = time.perf_counter()
            rc = s.L.ec3d_domain_integrals(s.h, delta, n.value, C.byref(n), out)
            times.append(time.perf_counter() - t0)
            assert rc == 0
        recs = s.domain_integrals(delta)
        cells = sum(r["cells"] for r in recs)
        med = statistics.median(times[warmup:])
        row.update(n=int(s.n), conductor_cells=int(cells), domains=len(recs), iter=int(info["iter"]),
                   call_ms_median=1e3 * med, call_ms_min=1e3 * min(times[warmup:]), call_ms_max=1e3 * max(times[warmup:]),
                   model_bytes=cells * BYTES_PER_CELL, model_GB_per_s=cells * BYTES_PER_CELL / med / 1e9,
                   integrals=[dict(domain=r["domain"], cells=r["cells"], sigma=r["sigma"], joule_w=r["joule_w"],
                                   force_n=r["force_n"].tolist()) for r in recs])

    with E.EC3DSolver() as s:
        host.run(model, s, steps=1, on_rhs=on_rhs, on_solved=on_solved, on_step=on_step)
    row["solve_resident_ms"] = 1e3 * (t["solve1"] - t["solve0"])
    row["call_over_solve"] = row["call_ms_median"] / row["solve_resident_ms"]
    row.update(tool="tools/domain_integrals_time.py", calls=calls, warmup=warmup)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "domain_integrals.jsonl"))
    ap.add_argument("--grids", nargs="+", default=["256x256x60", "256x256x256"])
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for grid in a.grids:
        row = measure([int(v) for v in grid.split("x")])
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
