"""Cost of ec3d_field_energy and ec3d_domain_linkage beside the time step they follow and the field output they replace,
on one MI355X.

    python tools/field_energy_time.py [--out profiles/field_energy.jsonl] [--grids 256x256x60 256x256x256]

ec_src_move_hole (tests/golden/g4_ec_src_move_hole) resampled to config 3's grids, as tools/domain_integrals_time.py builds
them.  One time step of host.run; the step's solve_resident is timed on the host (the device drained in front of it); after
the post-update, for each of ec3d_field_energy, ec3d_domain_linkage and ec3d_vtk_fields 3 warm-up calls and 20 timed ones,
host wall-clock around the synchronous call (the first warm-up call of the two new ones allocates and uploads).  One JSON
line per grid: the median calls, the solve, their ratios, and the bytes per second the streaming pass reaches under its
byte model (six doubles and the conductor byte per cell = 49 B) as a fraction of 8 TB/s."""
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
from tools.domain_integrals_time import model_of  # noqa: E402

BYTES_PER_CELL = 6 * 8 + 1
LINK_BYTES_PER_CELL = 6 * 8 + 4
HBM_BYTES_PER_S = 8e12


def timed(f, calls, warmup):
    times = []
    for _ in range(warmup + calls):
        t0 = time.perf_counter()
        f()
        times.append(time.perf_counter() - t0)
    t = times[warmup:]
    return dict(median=1e3 * statistics.median(t), min=1e3 * min(t), max=1e3 * max(t))


def measure(dims, calls=20, warmup=3):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host, vxc
    from eddy_currents_3d_amd.solver import DomainLink, FieldEnergy
    model = model_of(dims)
    tab = vxc.domain_tables(model)
    delta = np.ascontiguousarray(tab["delta"], np.float64)
    cells = int(model.vox.size)
    row = dict(grid="ec_src_move_hole %dx%dx%d" % tuple(dims), cells=cells)
    t = {}

    def on_rhs(k, s, info):
        s.L.ec3d_device_synchronize(s.h)
        t["solve0"] = time.perf_counter()

    def on_solved(k, s, info):
        t["solve1"] = time.perf_counter()

    def on_step(k, s, info):
        e = FieldEnergy()
        n = C.c_int32(0)
        assert s.L.ec3d_domain_linkage(s.h, delta, 0, C.byref(n), None) == 0
        out = (DomainLink * max(n.value, 1))()

        def energy():
            assert s.L.ec3d_field_energy(s.h, delta, C.byref(e)) == 0

        def linkage():
            assert s.L.ec3d_domain_linkage(s.h, delta, n.value, C.byref(n), out) == 0
        te, tl = timed(energy, calls, warmup), timed(linkage, calls, warmup)
        tv = timed(lambda: s.vtk_fields(delta, cells, tab["ncells0"] > 0), calls, warmup)
        link = s.domain_linkage(delta)
        listed = sum(r["cells"] for r in link)
        bps = cells * BYTES_PER_CELL / (te["median"] * 1e-3)
        row.update(n=int(s.n), iter=int(info["iter"]), domains=len(link), listed_cells=int(listed),
                   energy_ms_median=te["median"], energy_ms_min=te["min"], energy_ms_max=te["max"],
                   linkage_ms_median=tl["median"], linkage_ms_min=tl["min"], linkage_ms_max=tl["max"],
                   vtk_fields_ms_median=tv["median"], vtk_fields_ms_min=tv["min"], vtk_fields_ms_max=tv["max"],
                   energy_model_bytes=cells * BYTES_PER_CELL, energy_model_TB_per_s=bps / 1e12,
                   energy_fraction_of_8TBps=bps / HBM_BYTES_PER_S,
                   linkage_model_TB_per_s=listed * LINK_BYTES_PER_CELL / (tl["median"] * 1e-3) / 1e12,
                   energy=dict(energy_b=e.energy_b, energy_axis=list(e.energy_axis), aj_source=e.aj_source, aj_eddy=e.aj_eddy),
                   linkage=[dict(domain=r["domain"], cells=r["cells"], linkage=r["linkage"], jsum=r["jsum"].tolist())
                            for r in link])

    with E.EC3DSolver() as s:
        host.run(model, s, steps=1, on_rhs=on_rhs, on_solved=on_solved, on_step=on_step)
    row["solve_resident_ms"] = 1e3 * (t["solve1"] - t["solve0"])
    row["energy_over_solve"] = row["energy_ms_median"] / row["solve_resident_ms"]
    row["linkage_over_solve"] = row["linkage_ms_median"] / row["solve_resident_ms"]
    row["both_over_vtk_fields"] = (row["energy_ms_median"] + row["linkage_ms_median"]) / row["vtk_fields_ms_median"]
    row.update(tool="tools/field_energy_time.py", calls=calls, warmup=warmup)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "field_energy.jsonl"))
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
