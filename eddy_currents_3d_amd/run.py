"""Run a VoxCad ``.vxc`` model the way the reference program does, on one MI355X.

    python -m eddy_currents_3d_amd.run model.vxc [--steps N] [--out DIR] [--device D] [--integrals FILE] [--guess-history N]
                                                 [--energy FILE] [--null-projection [--null-tol Y]] [--tol X]
                                                 [--probes FILE [--probe I,J,K]... [--probe-line I0,J0,K0:I1,J1,K1]...
                                                  [--probe-box I0,J0,K0:I1,J1,K1]...]
    python -m eddy_currents_3d_amd.run model.vxc --harmonic FREQ [--out DIR] [--integrals FILE] [--tol X]
                                                 [--null-projection [--null-tol Y]]
    python -m eddy_currents_3d_amd.run model.vxc --harmonic F0 --sweep F1,F2,... [--sweep-batch N] [--out DIR]
                                                 [--integrals FILE] [--tol X]
                                                 [--sweep-null-projection [--sweep-null-tol Y]]
    python -m torch.distributed.run --nproc-per-node G -m eddy_currents_3d_amd.run model.vxc ...   (G GPUs)

Reads the file (eddy_currents_3d_amd/vxc.py), assembles the A-V system on the device, and runs the
reference's time loop (eddy_currents_3d_amd/host.py) with the fields resident in HBM; ``field_N.vtk`` files
and ``src_N.vtk`` files go to ``--out`` (default: the ``dir=`` name of the model's solver line, as the
reference does).  ``--integrals FILE``: Joule loss [W] and Lorentz force [N] of every conducting domain after every
step, as CSV (one GPU only).  ``--guess-history N``: start every step's solve from the projection onto up to N earlier
steps' solutions (EC3DSolver.set_guess_history; default 0 = off, one GPU only).  ``--energy FILE``: magnetic energy of
the box [J], the integral of A.J outside and inside the conductors [J] and the flux linkage psi*I [J] of every
non-conducting domain after every step, as CSV, one line per step (one GPU only).  ``--null-projection``: take the left
null vectors of the A-V system out of every solve's initial residual (EC3DSolver.set_null_projection; one GPU only), which
lets ``--tol X`` -- the solves' tolerance instead of the model's -- go below the reference's.  ``--probes FILE``: A, the
eddy and source current densities, B and U at chosen cells (0-based I,J,K: points, lines, boxes; a plane is a box one cell
thick) after every step, in float64, as CSV, one line per step and probe; they are recorded on the device and written
after the run (one GPU only).  ``--harmonic FREQ``: no time loop -- the periodic steady state at FREQ [Hz] by one complex
solve (host.run_harmonic): ``harmonic_re.vtk`` and ``harmonic_im.vtk`` go to ``--out``, ``--integrals FILE`` gets the Joule
loss and force of every conducting domain averaged over a period (one GPU only; moving sources are refused); with
``--null-projection`` the complex operator's left null vectors leave the initial residual, the
report line gains the projected residual and the adjoint solves' iterations, and ``--null-precond`` is refused.
``--harmonic F0 --sweep F1,F2,...``: a constant-current frequency sweep (host.run_harmonic_sweep) --
the source phasors are read at F0 and the same b^ is solved at every frequency of the list, up to ``--sweep-batch N``
(default and most: 16) of them in lock step in the launches of one iteration; ``harmonic_<k>_re.vtk`` and
``harmonic_<k>_im.vtk``, k the position in the list, go to ``--out``, ``--integrals FILE`` gets one line per frequency and
domain, and there is one report line per frequency; ``--null-projection`` is refused.  ``--sweep-null-projection``: every
frequency of a batch projects with the left null vectors of its own operator, found by adjoint
solves in lock step to ``--sweep-null-tol Y`` (default 1e-10), so that ``--tol X`` can go below the floor over the whole
sweep; the report lines gain the projected residual and the adjoint solves' iterations.
"""
from __future__ import annotations

import argparse
import os
import sys
import time


INTEGRALS_HEADER = "step,T,domain,cells,joule_w,force_x,force_y,force_z"


def integrals_rows(step, T, records):
    """CSV lines of one step's EC3DSolver.domain_integrals() records, floats at repr() precision."""
    return [",".join([str(int(step)), repr(float(T)), str(r["domain"]), str(r["cells"]), repr(float(r["joule_w"]))]
                     + [repr(float(f)) for f in r["force_n"]]) for r in records]


ENERGY_HEADER = "step,T,energy_b,aj_source,aj_eddy"   # then linkage_<id> per domain of EC3DSolver.domain_linkage()


def energy_header(linkage):
    return ",".join([ENERGY_HEADER] + [f"linkage_{r['domain']}" for r in linkage])


def energy_row(step, T, energy, linkage):
    """The CSV line of one step's EC3DSolver.field_energy() and domain_linkage(), floats at repr() precision."""
    return ",".join([str(int(step)), repr(float(T))] + [repr(float(energy[k])) for k in ("energy_b", "aj_source", "aj_eddy")]
                    + [repr(float(r["linkage"])) for r in linkage])


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m eddy_currents_3d_amd.run", description=__doc__.split("\n\n")[0])
    ap.add_argument("model", help="path of the .vxc file")
    ap.add_argument("--steps", type=int, default=None, help="stop after this many time steps (default: the model's stop time)")
    ap.add_argument("--out", default=None, help="directory for field_N.vtk (default: the model's dir= name)")
    ap.add_argument("--no-output", action="store_true", help="do not write VTK files")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--refine", type=int, nargs=3, metavar=("FX", "FY", "FZ"), default=None,
                    help="split every cell FX x FY x FZ times first (same physical size, finer grid)")
    ap.add_argument("--precond", choices=("none", "block-mg"), default="none",
                    help="preconditioner of the time step's solve: none (the reference's BiCGSTAB, default) or block-mg "
                         "(right-preconditioned BiCGSTAB, block multigrid M; one GPU only)")
    ap.add_argument("--u-rhs", choices=("reference", "all"), default="reference",
                    help="U rows that get their right-hand side when the model has several conducting domains: "
                         "reference (rows up to the largest domain's cell count, as the reference does; default) or "
                         "all (every U row: the consistent form, a departure from the reference; one GPU only)")
    ap.add_argument("--integrals", metavar="FILE", default=None,
                    help="write Joule loss and Lorentz force per conducting domain and time step to this CSV file "
                         "(" + INTEGRALS_HEADER + "; one GPU only)")
    ap.add_argument("--energy", metavar="FILE", default=None,
                    help="write the magnetic energy, the integral of A.J and the flux linkage of every non-conducting "
                         "domain per time step to this CSV file (" + ENERGY_HEADER + ",linkage_<id>...; one GPU only)")
    ap.add_argument("--guess-history", type=int, default=0, metavar="N", choices=range(0, 9),
                    help="start every step's solve from the projection onto up to N (0 .. 8) earlier steps' solutions; "
                         "0 (default): off, the reference's warm start from the previous step alone (one GPU only)")
    ap.add_argument("--null-projection", action="store_true",
                    help="take the left null vectors of the A-V system (one per connected conductor, found by an adjoint "
                         "solve after the assembly) out of every solve's initial residual, so that tolerances below the "
                         "reference's can be reached (one GPU only)")
    ap.add_argument("--null-tol", type=float, default=None, metavar="Y",
                    help="accuracy the adjoint solves of --null-projection are run to (default 1e-10); a solve fails when "
                         "one of them does not get there within its cap")
    ap.add_argument("--null-precond", choices=("none", "block-mg", "block-mg-a"), default=None,
                    help="preconditioner of the adjoint solves of --null-projection: the transposed block multigrid "
                         "(block-mg), the same with the A blocks' hierarchy of A as it stands (block-mg-a), or none "
                         "(default: the handle's setting, which starts as none)")
    ap.add_argument("--probes", metavar="FILE", default=None,
                    help="write the fields at the cells of --probe, --probe-line and --probe-box per time step to this "
                         "CSV file, from the record kept on the device (step,T,probe,i,j,k,ax,...,bz,u; one GPU only)")
    ap.add_argument("--probe", action="append", default=[], metavar="I,J,K", help="a probe at this cell (0-based; repeatable)")
    ap.add_argument("--probe-line", action="append", default=[], metavar="I0,J0,K0:I1,J1,K1",
                    help="probes along the line between the two cells, both included (repeatable)")
    ap.add_argument("--probe-box", action="append", default=[], metavar="I0,J0,K0:I1,J1,K1",
                    help="probes at every cell of the box with these inclusive corners, in scan order (repeatable)")
    ap.add_argument("--tol", type=float, default=None, metavar="X",
                    help="tolerance of the time step's solve instead of the model's (one GPU only)")
    ap.add_argument("--harmonic", type=float, default=None, metavar="FREQ",
                    help="instead of the time loop: one complex solve for the periodic steady state at FREQ Hz; writes "
                         "harmonic_re.vtk / harmonic_im.vtk to --out and the period averages to --integrals (one GPU only)")
    ap.add_argument("--sweep", default=None, metavar="F1,F2,...",
                    help="with --harmonic F0: solve the right-hand side of F0's source phasors at each of these "
                         "frequencies [Hz], batches of them in lock step; harmonic_<k>_re.vtk / harmonic_<k>_im.vtk per "
                         "frequency to --out, one line per frequency and domain to --integrals")
    ap.add_argument("--sweep-batch", type=int, default=16, metavar="N", choices=range(1, 17),
                    help="systems of --sweep solved in one batch (1 .. 16, default 16)")
    ap.add_argument("--sweep-null-projection", action="store_true",
                    help="with --sweep: take the left null vectors of every frequency's own operator out of its initial "
                         "residual, so that --tol can go below the floor at every frequency")
    ap.add_argument("--sweep-null-tol", type=float, default=None, metavar="Y",
                    help="accuracy the adjoint solves of --sweep-null-projection are run to (default 1e-10)")
    return ap


def check_sweep_options(ap, a):
    """The refusals of --sweep that need no model; returns the frequencies (None without --sweep)."""
    if a.sweep_null_tol is not None and not a.sweep_null_projection:
        ap.error("--sweep-null-tol needs --sweep-null-projection")
    if a.sweep is None:
        if a.sweep_null_projection:
            ap.error("--sweep-null-projection needs --sweep F1,F2,...")
        return None
    if a.harmonic is None:
        ap.error("--sweep needs --harmonic F0, the frequency at which the sources' phasors are read")
    if a.null_projection:
        ap.error("--sweep does not go with --null-projection: the left null vectors belong to one frequency "
                 "(--sweep-null-projection gives every frequency of the sweep its own)")
    try:
        freqs = [float(w) for w in a.sweep.split(",") if w.strip()]
    except ValueError:
        ap.error(f"--sweep needs a list of frequencies F1,F2,..., not {a.sweep!r}")
    if not freqs:
        ap.error("--sweep needs at least one frequency")
    if not all(f > 0.0 and f < float("inf") for f in freqs):
        ap.error("--sweep needs frequencies above 0")
    return freqs


def _write_harmonic_integrals(f, freq, records):
    for q in records:
        f.write(",".join([repr(float(freq)), str(q["domain"]), str(q["cells"]), repr(float(q["joule_w"]))]
                         + [repr(float(v)) for v in q["force_n"]]) + "\n")


def run_sweep_cli(ap, a, model, t, out_dir, freqs):
    """--harmonic F0 --sweep F1,F2,...: host.run_harmonic_sweep and one report line per frequency."""
    from . import EC3DSolver, host
    if not a.harmonic > 0.0:
        ap.error("--harmonic needs a frequency above 0")
    t0 = time.perf_counter()
    with EC3DSolver(device=a.device) as s:
        try:
            rs = host.run_harmonic_sweep(model, s, a.harmonic, freqs, tol=a.tol, out_dir=out_dir,
                                         integrals=bool(a.integrals), batch=a.sweep_batch,
                                         **(dict(null_projection=True, null_tol=a.sweep_null_tol)
                                            if a.sweep_null_projection else {}))
        except ValueError as e:
            ap.error(str(e))
    if a.integrals:
        with open(a.integrals, "w") as f:
            f.write(HARMONIC_INTEGRALS_HEADER + "\n")
            for r in rs:
                _write_harmonic_integrals(f, r["freq"], r["integrals"])
    for k, r in enumerate(rs):
        null = (f"projected residual={r['projected_residual']:.3e} adjoint iterations="
                f"{'+'.join(str(q['iterations']) for q in r['null']['components'])} " if a.sweep_null_projection else "")
        print(f"harmonic sweep {k} at {r['freq']:g} Hz (phasors of {a.harmonic:g} Hz): iter={r['iter']} "
              f"relres={r['relres']:.3e} true residual={r['true_residual']:.3e} restarts={r['info']['restarts']} {null}"
              f"({r['info']['ms']:.1f} ms in its batch's solve)"
              + (f"  -> {out_dir}/harmonic_{k}_re.vtk, harmonic_{k}_im.vtk" if out_dir else ""), flush=True)
    print(f"{len(rs)} frequencies in {time.perf_counter() - t0:.2f} s wall", flush=True)
    return 0


HARMONIC_INTEGRALS_HEADER = "freq,domain,cells,joule_w_avg,force_x_avg,force_y_avg,force_z_avg"


def run_harmonic_cli(ap, a, model, t, out_dir):
    """--harmonic FREQ: host.run_harmonic and its report."""
    from . import EC3DSolver, host
    if not a.harmonic > 0.0:
        ap.error("--harmonic needs a frequency above 0")
    if a.null_precond is not None:
        ap.error("--null-precond does not go with --harmonic: there is no preconditioner for the complex adjoint solves")
    if a.null_tol is not None and not a.null_projection:
        ap.error("--null-tol needs --null-projection")
    t0 = time.perf_counter()
    with EC3DSolver(device=a.device) as s:
        try:
            r = host.run_harmonic(model, s, a.harmonic, tol=a.tol, out_dir=out_dir, integrals=bool(a.integrals),
                                  null_projection=a.null_projection, null_tol=a.null_tol)
        except ValueError as e:
            ap.error(str(e))
    if a.integrals:
        with open(a.integrals, "w") as f:
            f.write(HARMONIC_INTEGRALS_HEADER + "\n")
            _write_harmonic_integrals(f, a.harmonic, r["integrals"])
    null = (f"projected residual={r['projected_residual']:.3e} adjoint iterations="
            f"{'+'.join(str(q['iterations']) for q in r['null']['components'])} " if a.null_projection else "")
    print(f"harmonic solve at {a.harmonic:g} Hz: iter={r['iter']} relres={r['relres']:.3e} "
          f"true residual={r['true_residual']:.3e} restarts={r['info']['restarts']} {null}"
          f"({r['info']['ms']:.1f} ms in the solve, {time.perf_counter() - t0:.2f} s wall)"
          + (f"  -> {out_dir}/harmonic_re.vtk, harmonic_im.vtk" if out_dir else ""), flush=True)
    return 0


def check_probe_options(ap, a, world):
    """The refusals of --probes that need no model: several ranks, no probe option, a probe option without --probes."""
    given = bool(a.probe or a.probe_line or a.probe_box)
    if a.probes and world > 1:
        ap.error("--probes runs on one GPU only; a z-slab holds only part of the box")
    if a.probes and not given:
        ap.error("--probes needs at least one of --probe, --probe-line, --probe-box")
    if given and not a.probes:
        ap.error("--probe, --probe-line and --probe-box need --probes FILE")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    check_probe_options(ap, a, world)
    sweep = check_sweep_options(ap, a)
    if world > 1 and a.integrals:
        ap.error("--integrals runs on one GPU only; a z-slab holds only part of a conducting domain")
    if world > 1 and a.energy:
        ap.error("--energy runs on one GPU only; a z-slab holds only part of the box and of every domain")

    from . import EC3DSolver, host, vxc
    model = vxc.read_vxc(a.model)
    if a.refine:
        model = vxc.refine(model, *a.refine)
    t = vxc.domain_tables(model)
    sdz, sdy, sdx = model.vox.shape
    out_dir = None if a.no_output else (a.out or str(t["directory"]).upper())
    print(f"{a.model}: grid {sdx}x{sdy}x{sdz}, {t['ncells0']} conducting cells, dt={t['dt']:g} stop={t['time']:g} "
          f"tol={t['tol']:g} itmax={t['itmax']}", flush=True)
    if a.harmonic is not None:
        if world > 1:
            ap.error("--harmonic runs on one GPU only; the complex solve has no z-slab form")
        if sweep is not None:
            return run_sweep_cli(ap, a, model, t, out_dir, sweep)
        return run_harmonic_cli(ap, a, model, t, out_dir)
    pcells = None
    if a.probes:
        from . import probes as P
        try:
            pcells = P.cells_from_options(a.probe, a.probe_line, a.probe_box, (sdx, sdy, sdz))
        except ValueError as e:
            ap.error(str(e))
    t0 = time.perf_counter()

    csv = None
    if a.integrals:   # one line per step and domain, written as the run goes
        csv = open(a.integrals, "w")
        csv.write(INTEGRALS_HEADER + "\n")

    ecsv = open(a.energy, "w") if a.energy else None   # one line per step; the header goes out with the first

    def on_step(k, s, info):
        if csv is not None:
            csv.writelines(line + "\n" for line in integrals_rows(k, info["T"], info["integrals"]))
            csv.flush()
        if ecsv is not None:
            if k == 0:
                ecsv.write(energy_header(info["linkage"]) + "\n")
            ecsv.write(energy_row(k, info["T"], info["energy"], info["linkage"]) + "\n")
            ecsv.flush()
        print(f"step {k:4d}  T={info['T']:.6g}  iter={info['iter']}"
              + (f"  -> field_{info['output']}.vtk" if "output" in info and out_dir else ""), flush=True)

    if world > 1 and a.precond != "none":
        ap.error(f"--precond {a.precond} runs on one GPU only; the multi-rank z-slab path has no preconditioner")
    if world > 1 and a.guess_history:
        ap.error("--guess-history runs on one GPU only; the history's sums would need every rank's")
    if world > 1 and (a.null_projection or a.tol is not None):
        ap.error("--null-projection and --tol run on one GPU only; the left null vectors' sums would need every rank's")
    if world > 1 and a.u_rhs != "reference":
        ap.error(f"--u-rhs {a.u_rhs} runs on one GPU only; z-slabs take one conducting domain")
    if world > 1:   # one process per GPU: z-slabs, halo exchange and reductions over RCCL
        import torch
        import torch.distributed as dist
        rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        try:
            log = host.run_slabs(model, rank, world, device=local, steps=a.steps, out_dir=out_dir,
                                 on_step=on_step if rank == 0 else None)
        finally:
            dist.destroy_process_group()
        if rank != 0:
            return 0
        n = 3 * model.vox.size + t["ncells0"]
    else:
        try:
            with EC3DSolver(device=a.device) as s:
                log = host.run(model, s, steps=a.steps, out_dir=out_dir, on_step=on_step,
                               precond=None if a.precond == "none" else a.precond, u_rhs=a.u_rhs,
                               integrals=csv is not None, guess_history=a.guess_history or None,
                               energy=ecsv is not None, null_projection=True if a.null_projection else None,
                               tol=a.tol, null_tol=a.null_tol,
                               null_precond=a.null_precond if a.null_projection else None, probes=pcells)
                if pcells is not None:   # the record has been read: one line per step and probe
                    with open(a.probes, "w") as f:
                        f.write(P.CSV_HEADER + "\n")
                        for k, info in enumerate(log):
                            f.writelines(line + "\n" for line in P.csv_rows(k, info["T"], pcells, (sdx, sdy, sdz), info["probes"]))
                if a.null_projection:
                    q = s.null_projection()
                    kind, levels, hms = s.null_precond()
                    print(f"null projection: {q['kept']} of {q['found']} components kept, set-up {q['setup_ms']:.1f} ms "
                          f"(preconditioner {kind}, {len(levels)} levels, {hms:.1f} ms), "
                          + ", ".join(f"{c['iterations']} it / {c['residual']:.2e}" for c in q["components"]), flush=True)
                n = s.n
        finally:
            if csv is not None:
                csv.close()
            if ecsv is not None:
                ecsv.close()
    wall = time.perf_counter() - t0
    its = sum(i["iter"] for i in log)
    print(f"{len(log)} steps, {its} solver iterations, n={n}, {wall:.2f} s wall "
          f"({n * its / wall:.3e} DOF*iters/s including assembly, source update and output)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
