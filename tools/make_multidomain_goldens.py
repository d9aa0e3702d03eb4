#!/usr/bin/env python3
"""Write tests/golden/g8*_*.npz and g9*_*.npz: models with SEVERAL conducting domains, and models with six distinct
boundary values, captured from the unmodified reference.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py, whose helpers it uses: needs the reference sources and
oracle/_ref/EC3D_capture (``make -C oracle ref``).  Each fixture holds the inputs (vox, palette names, lattice,
the reference's geoPHYS / geoPHYS_C / valPHYS rebuilt by oracle.make_goldens.geometry_tables), every solver call's
b, x_in, x_out and iteration count, the CSR (checked equal across the calls), and the reference's field_N.vtk of
the last step.

  g8a  two separated plates stacked along z, the upper one larger (siznod(2) > siznod(1)): the U rows past
       max siznod keep a zero right-hand side, interior cells among them.  Static coil, 3 steps.
  g8b  two blocks touching along z, domain 1 below (U ids in scan order), domain 2 moving (Vex).  3 steps.
  g8c  two blocks touching along x, domain 2 on the -x side: the U ids are not in scan order, so the reference's
       U rows (scan order) and U columns (domain-major) disagree and it stalls.  itmax = 40, 3 steps.
  g8ck g8c's first solve cut after 5 iterations: the reference's early iterate, before the stall.
  g8d  g3's geometry with its plate split by a z-plane into two domains of the same material.  4 steps.  Its U
       rows past max siznod are the top plane's, which cel_bndUz zeroes anyway: both rules give the same b.

The g9 pair leaves the ground every earlier fixture stands on (BND = -0.95 on all six faces, box-shaped conductors):
a ``boundary`` record with six distinct values, one of them 0 (the reference then stores explicit zeros) and two
positive, on the anisotropic lattice (1, 1.25, 0.75).

  g9a  two blocks touching along z, domain 1 below (U ids in scan order: the structured form applies), different
       conductivities, each with its own Vex / Vey / Vez of mixed sign.  Static coil, 3 steps.
  g9b  one conducting domain, L-shaped in the x-y plane (a concave step) with a 1 x 1 through hole along z, one cell
       from the box on the low-x and on the high-y side, z planes [5, 11) of 16.  dist.slab_bounds cuts 16 planes at 8
       for two slabs and at 6 and 11 for three: the cut at 11 coincides with the conductor's top face (the one-sided z
       stencil of the plane below reads the second halo plane), the cut at 6 lies one plane above its bottom face, and
       8 cuts it in the middle.  Moving coil (Vsx, and Vsy a FUNC), 3 steps, tol = 5m.  The reference stalls easily on
       this shape (at tol = 1m, with the coil one plane lower, or with the conductor one plane thicker it takes the
       itmax exit on the second or third step); this placement converges in 24, 14 and 13 iterations.

    python tools/make_multidomain_goldens.py [g8a g8b g8c g8d g8ck g9a g9b]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import make_goldens as G  # noqa: E402

ALU, CU = "mu0*35.26e6", "mu0*58e6"
SIGMA = {ALU: 35.26e6, CU: 58e6}
SRC = ["f1 func Fp=a*cos(p2*f*t) a='183/(dx*2*dz)' p2='2*pi' f=50 t=t",
       "f2 func Fm=a*cos(p2*f*t) a='-183/(dx*2*dz)' p2='2*pi' f=50 t=t"]


def _case(stem, vox, conductors, coil_extra, steps, tol, itmax, lattice="0.004", extra=(), adj=("1", "1", "1"),
          bnd=None):
    """conductors: [(palette name, C expression, (vex, vey, vez))], palette ids 1..D; coil ids D+1..D+4.
    bnd: ((BXM, BXP), (BYM, BYP), (BZM, BZP)) of a ``boundary`` record; None: the reference's default, -0.95."""
    D = len(conductors)
    names = [f"{nm} D=1 C='{c}'" + ("" if not any(v) else " Vex={} Vey={} Vez={}".format(*v))
             for nm, c, v in conductors]
    names += G.coil_names(coil_extra) + [f"param tran stop={steps}m step=1m",
                                         f"p2 solver tol={tol} itmax={itmax} dir={stem[:3]}"] + SRC + list(extra)
    BND = np.full((3, 2), -0.95)
    if bnd is not None:
        BND = np.array(bnd, np.float64)
        names.append("bnd boundary " + " ".join(f"B{ax}{side}={BND[d, s]:g}" for d, ax in enumerate("XYZ")
                                                for s, side in enumerate("MP")))
    calls, log = G.run_reference(vox=vox, names=names, lattice_dim=lattice, adj=adj, max_calls=steps,
                                 all_matrices=True)
    assert len(calls) == steps, (stem, len(calls))
    for c in calls[1:]:   # one assembly for the whole run: every call's CSR is the first one's
        assert np.array_equal(c["irow"], calls[0]["irow"]) and np.array_equal(c["jcol"], calls[0]["jcol"])
        assert np.array_equal(c["valA"], calls[0]["valA"])
    geo, geoC, _ = G.geometry_tables(vox, list(range(1, D + 1)), D + 4)
    valPHYS = np.zeros((int(geo.max()), 5))
    valPHYS[:, 0] = 1.0
    for m, (_, c, v) in enumerate(conductors):
        valPHYS[m, 1] = G.MU0 * SIGMA[c]
        valPHYS[m, 2:5] = v
    last = max((k for k in calls[0]["vtk"] if k.startswith("field_")), key=lambda k: int(k[6:-4]))
    calls[0]["vtk"] = {last: calls[0]["vtk"][last]}
    d = G.pack_calls(calls)
    d["vtk_last"] = np.array(last)
    fadj = np.array([float(a) for a in adj])
    G.save(stem, vox=vox, names=np.array(names), lattice_dim=np.array(lattice), adj=fadj,
           geoPHYS=geo, geoPHYS_C=geoC, delta=float(lattice) * fadj, dt=np.float64(1e-3),
           BND=BND, valPHYS=valPHYS, **d)
    print(stem, "iterations", [c["iter"] for c in calls])


def g8a():
    vox = np.zeros((16, 16, 18), np.uint8)
    vox[2:7, 5:11, 6:12] = 1            # 5 x 6 x 6 = 180 cells
    vox[9:13, 3:13, 3:15] = 2           # 4 x 10 x 12 = 480 cells, above with a 2-plane gap; the U rows past 480
    G.put_coil(vox, (3, 4, 5, 6), 14, 15, 4, 12, 4, 14)  # reach below its top plane, to interior cells
    _case("g8a_two_plates_18x16x16", vox, [("alu", ALU, (0, 0, 0)), ("cu", CU, (0, 0, 0))], "", 3, "5m", 10000)


def g8b():
    vox = np.zeros((14, 16, 20), np.uint8)
    vox[3:6, 4:12, 4:16] = 1            # domain 1 below
    vox[6:9, 4:12, 4:16] = 2            # domain 2 on top of it, moving along x
    G.put_coil(vox, (3, 4, 5, 6), 10, 12, 3, 13, 3, 17)
    _case("g8b_stacked_moving_20x16x14", vox, [("alu", ALU, (0, 0, 0)), ("cu", CU, (1.5, 0, 0))], "", 3, "5m",
          10000)


def g8c():
    vox = np.zeros((14, 18, 20), np.uint8)
    vox[3:7, 4:13, 10:16] = 1           # domain 1 on the +x side
    vox[3:7, 4:13, 4:10] = 2            # domain 2 on the -x side, touching
    G.put_coil(vox, (3, 4, 5, 6), 9, 11, 3, 14, 3, 17)
    _case("g8c_side_by_side_20x18x14", vox, [("alu", ALU, (0, 0, 0)), ("cu", CU, (0, 0, 0))], "", 3, "5m", 40)


def g8d():
    inp = G.inputs_g3()
    vox = inp["vox"].copy()
    plate = vox == 1
    vox[vox > 1] += 1                   # coil ids 2..5 -> 3..6
    vox[plate] = 2
    ks = np.flatnonzero(plate.any(axis=(1, 2)))
    vox[ks[0]][plate[ks[0]]] = 1        # the plate's lowest plane is domain 1, the rest domain 2
    _case("g8d_g3_split_18x16x12", vox, [("plast", ALU, (0, 0, 0)), ("plast2", ALU, (0, 0, 0))],
          " Vsx=2.0 Vsy=Vmy", 4, "1m", 10000,
          extra=["m2 func Vmy=a*p2*f*cos(p2*f*t) a='-dY*3' p2='2*pi' f=100 t=t"])


def g8ck():
    """g8c's first solve cut after K = 5 iterations (itmax = 4): the reference's early iterate of the stalling
    case, b and x only (the CSR is g8c's)."""
    vox = np.zeros((14, 18, 20), np.uint8)
    vox[3:7, 4:13, 10:16] = 1
    vox[3:7, 4:13, 4:10] = 2
    G.put_coil(vox, (3, 4, 5, 6), 9, 11, 3, 14, 3, 17)
    names = [f"alu D=1 C='{ALU}'", f"cu D=1 C='{CU}'"] + G.coil_names() + [
        "param tran stop=1m step=1m", "p2 solver tol=5m itmax=4 dir=g8c"] + SRC
    calls, _ = G.run_reference(vox=vox, names=names, lattice_dim="0.004", max_calls=1)
    c = calls[0]
    G.save("g8ck_side_by_side_first_iterates", b0=c["b"], xin0=c["x_in"], xout0=c["x_out"],
           iters=np.array([c["iter"]], np.int32), itmax=np.int32(c["itmax"]), tol=np.float64(c["tol"]))
    print("g8ck iterations", c["iter"])


BND9 = ((-0.95, 0.5), (-1.0, 1.5), (0.0, -0.25))   # six distinct values: one 0, two positive
ADJ9 = ("1", "1.25", "0.75")


def g9a():
    vox = np.zeros((14, 16, 20), np.uint8)
    vox[3:6, 4:12, 4:16] = 1            # domain 1 below
    vox[6:9, 4:12, 4:16] = 2            # domain 2 on top of it: U ids in scan order
    G.put_coil(vox, (3, 4, 5, 6), 10, 12, 3, 13, 3, 17)
    _case("g9a_two_moving_mixed_bnd_20x16x14", vox, [("alu", ALU, (1.5, -0.7, 0.3)), ("cu", CU, (-0.9, 0.4, -1.1))],
          "", 3, "5m", 10000, adj=ADJ9, bnd=BND9)


def g9b():
    vox = np.zeros((16, 16, 17), np.uint8)
    vox[5:11, 2:15, 1:14] = 1           # 13 x 13 x 6, one cell from the low-x and from the high-y face
    vox[5:11, 2:8, 8:14] = 0            # the quadrant high-x / low-y cut away: an L with a concave step
    vox[5:11, 11, 4] = 0                # through hole along z in the corner of the L, 1 x 1, walls 3 cells
    G.put_coil(vox, (2, 3, 4, 5), 13, 15, 4, 12, 3, 11)
    _case("g9b_L_hole_near_faces_17x16x16", vox, [("plast", ALU, (0, 0, 0))], " Vsx=2.0 Vsy=Vmy", 3, "5m", 10000,
          extra=["m2 func Vmy=a*p2*f*cos(p2*f*t) a='-dY*3' p2='2*pi' f=100 t=t"], adj=ADJ9, bnd=BND9)


CASES = dict(g8a=g8a, g8b=g8b, g8c=g8c, g8d=g8d, g8ck=g8ck, g9a=g9a, g9b=g9b)

if __name__ == "__main__":
    for name in sys.argv[1:] or CASES:
        CASES[name]()
