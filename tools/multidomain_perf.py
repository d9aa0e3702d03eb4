"""Cost of several conducting domains: ec_src_move_hole resampled to 256x256x60 (tests/test_gpu_fullsize.py's config 3
grid) with its conducting plate split by a z-plane into two domains of the same material.

    python tools/multidomain_perf.py [--out profiles/multidomain_iteration.jsonl] [--iters 300] [--steps 3]

A z-plane split keeps the U ids in scan order (the lower part is domain 1), so ec3d_assemble keeps the structured form;
an x- or y-plane split would not.  For one domain (as shipped), two domains structured and two
domains on bands + tail (ec3d_set_structured(h, 0)) it records ms per iteration (ec3d_time_iterations, after a
host.run of --steps steps) and seconds per host.run step, and checks that the two-domain run under u_rhs="all" leaves
X bit-identical to the one-domain run after every step.  One JSON line per variant."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def models():
    from eddy_currents_3d_amd import vxc
    g = np.load(os.path.join(GOLDEN, "g4_ec_src_move_hole.npz"))
    names = [str(s) for s in g["names"]]
    small = vxc.VxcModel(g["vox"], names, float(str(g["lattice_dim"])), tuple(float(x) for x in g["adj"]))
    one = vxc.resample(small, 256, 256, 60)
    t = vxc.domain_tables(one)
    cond = [d for d in range(1, len(names) + 1) if t["valPHYS"][d - 1, 1] != 0.0 and np.any(one.vox == d)]
    assert len(cond) == 1, cond
    m = cond[0]
    ks = np.flatnonzero((one.vox == m).any(axis=(1, 2)))
    assert len(ks) >= 2, "the plate is one plane thick"
    split = ks[0] + len(ks) // 2
    vox = one.vox.copy()
    nsub = int(vox.max())
    upper = vox[split:]
    upper[upper == m] = nsub + 1                       # planes split.. of the plate: a new, later palette entry
    two = vxc.VxcModel(vox, names[:nsub] + [names[m - 1].replace(names[m - 1].split()[0], "plate_upper", 1)]
                       + names[nsub:], one.lattice_dim, one.adj)
    assert np.array_equal(two.delta, one.delta)
    return one, two, dict(plate_planes=[int(ks[0]), int(ks[-1])], split_plane=int(split))


def run(model, structured, u_rhs, steps, iters):
    import eddy_currents_3d_amd as E
    from eddy_currents_3d_amd import host
    xs, t_step = [], []
    t0 = [time.perf_counter()]

    def on_step(k, s, info):
        t_step.append(time.perf_counter() - t0[0])
        xs.append(s.download("X"))
        t0[0] = time.perf_counter()
    with E.EC3DSolver(structured=structured) as s:
        log = host.run(model, s, steps=steps, u_rhs=u_rhs, on_step=on_step)
        mi = s.info
        s.time_iterations(20)
        ms = min(s.time_iterations(iters), s.time_iterations(iters)) / iters   # ec3d_time_iterations: ms in total
        out = dict(n=int(mi.n), tail_rows=int(mi.tail_rows), dict_classes=int(mi.dict_classes),
                   iters_per_step=[int(i["iter"]) for i in log], ms_per_iteration=ms,
                   s_per_step=[round(v, 4) for v in t_step])
    return out, xs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multidomain_iteration.jsonl"))
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args(argv)
    one, two, where = models()
    rows = []
    base, x1 = run(one, None, None, a.steps, a.iters)
    rows.append(dict(variant="one domain", **where, **base))
    r, x2 = run(two, None, "all", a.steps, a.iters)
    same = len(x1) == len(x2) and all(np.array_equal(p, q) for p, q in zip(x1, x2))
    rows.append(dict(variant="two domains, structured, u_rhs=all", x_bitwise_equal_one_domain=same, **r))
    r, _ = run(two, None, "reference", a.steps, a.iters)
    rows.append(dict(variant="two domains, structured, u_rhs=reference", **r))
    r, _ = run(two, False, "reference", a.steps, a.iters)
    rows.append(dict(variant="two domains, bands + tail (ec3d_set_structured(h, 0))", **r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for row in rows:
            row.update(tool="tools/multidomain_perf.py", grid="ec_src_move_hole 256x256x60", iters_timed=a.iters)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
