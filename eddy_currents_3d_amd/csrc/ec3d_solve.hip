// ec3d_solve.hip — the solve loop, host side of src/solvers.f90:3-50.
//
// The loop body is five asynchronous launches per iteration (ec3d_kernels.hip); all scalars and the
// convergence decision stay on the device.  The host runs ahead by up to two chunks of iterations and
// learns about an exit from an asynchronous copy of the SolverState; launches issued past the exit are
// no-ops, so the result is exactly the reference's.
#include "../../include/ec3d_hip.h"
#include "ec3d_internal.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

// ---------------------------------------------------------------------------------------------
// Where a consumer finds the sums it needs.  Single GPU: the producer's per-workgroup partials; the
// producers of slots BB, RR_INIT, D1, D2, D3 are SpMV-type kernels (sweep_s), those of SS, RR, RR0N
// vector kernels (sweep) -- every consumer reads slots of one producer class only.
static int parts_of(const ec3d_ctx *c, int producer, bool split)
{
    if (producer == EC3D_BY_K2) return ec3d_fused23(c) ? c->sweep_s.nblk : c->sweep_k2.nblk; // fused: S.S comes from K23
    if (producer == EC3D_BY_K4 && !ec3d_k4s(c)) return c->sweep.nblk; // (K4 in SpMV form sums on that grid)
    if (!split) return c->sweep_s.nblk;
    // a split producer leaves both launches' partials (SplitSweep::parts): K4 in SpMV form and K5-in-K1 of the three-launch
    // iteration on the 2-D tiles, K1 and K3 otherwise
    const bool f = producer == EC3D_BY_K4 || (ec3d_fused51(c) && c->slab_fused);
    return (f ? c->split_f : c->split_s).parts();
}
RedSrc ec3d_src_of(const ec3d_ctx *c, int producer)
{
    if (c->dist && c->lsum_ptrs) return RedSrc{nullptr, c->nranks, 0, 0, c->lsum_ptrs};
    if (c->dist) return RedSrc{c->gsum, c->nranks, P_NSLOT, 1, nullptr};
    return RedSrc{c->partials, parts_of(c, producer, false), 1, c->sweep.pstride, nullptr};
}
RedSrc ec3d_part_of(const ec3d_ctx *c, int producer, bool split)
{
    return RedSrc{c->partials, parts_of(c, producer, split), 1, c->sweep.pstride, nullptr};
}

// Where vector `vec` of iteration `it` lives: P in the ring pbuf (K5-in-K1 alternates two buffers, the deferred X update
// keeps D), AP in apbuf (K5-in-K1), S in sbuf (deferred X update); otherwise the plain work vector.  The multi-rank
// drivers address the halo exchange of an iteration's vector through the same function (ec3d_multi.hip): the ring
// position is worked out from MY handle's state (every rank of a job runs the same plan with the same depths, and my
// state is current when I get here), the pointer taken from the owner's tables, which do not change while a job runs:
// another rank's thread may be iterations ahead or behind with its own host-side bookkeeping.
double *ec3d_vec_at(const ec3d_ctx *me, const ec3d_ctx *owner, int vec, int it)
{
    const bool f51 = ec3d_fused51(me);
    const int D = ec3d_xdefer(me);
    switch (vec) {
    case EC3D_VEC_P: return (f51 || D > 1) ? owner->pbuf[ec3d_p_slot(me, it)] : owner->vec[EC3D_VEC_P];
    case EC3D_VEC_AP: return f51 ? owner->apbuf[ec3d_ap_slot(it)] : owner->vec[EC3D_VEC_AP];
    case EC3D_VEC_S: return D > 1 ? owner->sbuf[ec3d_s_slot(me, it)] : owner->vec[EC3D_VEC_S];
    default: return owner->vec[vec];
    }
}

// P and S of the `count` iterations that end with `last`, oldest first: what a launch that applies pending X updates is
// handed.  Entries at or past the count repeat the newest one (count = 0: iteration `last`'s own, whose S a K4 that
// leaves X alone still reads as entry 0): no kernel dereferences them, any valid pointer will do.
static void pending_bufs(const ec3d_ctx *c, int last, int count, const double **pp, const double **sp)
{
    const int n = std::max(count, 1);
    for (int j = 0; j < EC3D_XD_MAX; ++j) {
        const int itj = last - (n - 1) + std::min(j, n - 1);
        pp[j] = ec3d_vec_at(c, EC3D_VEC_P, itj);
        sp[j] = ec3d_vec_at(c, EC3D_VEC_S, itj);
    }
}

// the cursor behind K2 / K2-in-K3 and behind K5 / K5-in-K1 of iteration it (ec3d_dist_step's split K2 / K5 launches too)
void ec3d_after_s(ec3d_ctx *c, int it) { c->run.scur = ec3d_xdefer(c) > 1 ? ec3d_s_slot(c, it) : 1; }
void ec3d_after_p(ec3d_ctx *c, int it)
{
    const bool f51 = ec3d_fused51(c);
    if (f51 || ec3d_xdefer(c) > 1) c->run.pcur = ec3d_p_slot(c, it + 1); // (else K5 updates P in place)
    if (f51) c->run.apcur = ec3d_ap_slot(it + 1);
    if (f51) c->run.ap_valid_for = it + 1;
    c->run.it_next = it + 1;
}

// the five launches of one iteration; `k` selects one of them (1..5) or all (0).
// With the fusions of the 2-D-tile kernels (single rank, vectors beyond the caches) an iteration is THREE launches:
//   stage 1: K1 -- only in iteration 1 (afterwards AP = A P was produced by the previous iteration's stage 5)
//   stage 2: empty, stage 3: K23 (S = R - alpha*AP inside AS = A S)
//   stage 4: K4 -- as an SpMV kernel that computes A S again (ec3d_k4s: K23 then does not store AS), or the vector kernel
//   stage 5: K51 (the exits and the P update of K5, then the NEXT iteration's K1 on the new P)
// P(it) and AP(it) then live in pbuf[ec3d_p_slot(it)] / apbuf[ec3d_ap_slot(it)] (ec3d_ctx).
// With the X update deferred (ec3d_xdefer = D > 1; three launches or five) P(it) and S(it) live in rings of D buffers, K4
// leaves X alone except in the last iteration of a group of D (counted from xd_base) or of the call (xd_last), where it
// applies what is pending; an exit in between is completed by ec3d_flush_x.
void ec3d_launch_stage(ec3d_ctx *c, const MatView &A, int it, int k, int part)
{
    double **v = c->vec;
    const Sweep &sw = c->sweep, &ss = part == 1 ? c->split_f.bnd : part == 2 ? c->split_f.inte : c->sweep_s;
    hipStream_t s = c->stream;
    const bool fused = ec3d_fused23(c); // K2 inside K3 (2-D tiles, single rank): stage 2 is empty, stage 3 is K23
    const bool f51 = ec3d_fused51(c);
    const int D = ec3d_xdefer(c);
    double *P = ec3d_vec_at(c, EC3D_VEC_P, it), *AP = ec3d_vec_at(c, EC3D_VEC_AP, it);
    double *S = ec3d_vec_at(c, EC3D_VEC_S, it);
    // fused: AP(it) was produced by the previous iteration's K51 -- unless this call does not continue that
    // iteration (iteration 1, ec3d_iterate from another first_iter, ec3d_time_kernel): then K1 runs on its own
    if ((k == 0 || k == 1) && (!f51 || it == 1 || c->run.ap_valid_for != it))
        ec3d_launch_k1(A, ss, c->state, it, P, v[EC3D_VEC_R0], AP, c->partials, s);
    if ((k == 0 || k == 2) && !fused) {
        ec3d_launch_k2(c->sweep_k2, ec3d_src_of(c, EC3D_BY_SPMV), c->state, it, v[EC3D_VEC_R], AP, S, c->partials, s);
        ec3d_after_s(c, it);
    }
    if ((k == 0 || k == 3) && fused) {
        ec3d_launch_k23(A, ss, ec3d_src_of(c, EC3D_BY_SPMV), c->state, it, v[EC3D_VEC_R], AP, S,
                        ec3d_k4s(c) ? nullptr : v[EC3D_VEC_AS], c->partials, s); // (K4 in SpMV form computes A S again)
        ec3d_after_s(c, it);
    }
    if ((k == 0 || k == 3) && !fused)
        ec3d_launch_k3(A, ss, c->state, it, S, v[EC3D_VEC_AS], c->partials, s);
    if (k == 0 || k == 4) {
        // position of this iteration in its group of D, and how many updates an applying launch finds pending
        const int xm = D > 1 ? (it - c->run.xd_base) % D : 0;
        // (ec3d_xasync: no K4 touches X; alpha / omega of iteration it wait in entry it % 2D, and the group's own launch --
        // below, behind the K4 of its last iteration -- applies them)
        const bool xa = ec3d_xasync(c);
        const bool group_end = D > 1 && (xm == D - 1 || it >= c->run.xd_last);
        const bool apply = !xa && (D <= 1 || group_end);
        const int xe = xa ? it % (2 * D) : xm; // the entry this K4 leaves its alpha / omega in
        if (!ec3d_k4s(c) && (D <= 1 || (apply && xm == 0))) {
            ec3d_launch_k4(sw, ec3d_src_of(c, EC3D_BY_K2), ec3d_src_of(c, EC3D_BY_SPMV), c->state, it, P, S, v[EC3D_VEC_AS],
                           v[EC3D_VEC_R0], v[EC3D_VEC_X], v[EC3D_VEC_R], c->partials, c->hist, c->hist_cap, s);
        } else {
            const double *pp[EC3D_XD_MAX], *sp[EC3D_XD_MAX];
            const int ne = apply ? xm + 1 : 0; // iterations it - xm .. it
            pending_bufs(c, it, ne, pp, sp);
            if (ec3d_k4s(c))
                ec3d_launch_k4s(A, ss, ec3d_src_of(c, EC3D_BY_K2), ec3d_src_of(c, EC3D_BY_SPMV), c->state, it, ne, xe, pp, sp,
                                v[EC3D_VEC_R0], v[EC3D_VEC_X], v[EC3D_VEC_R], c->partials, c->hist, c->hist_cap, s);
            else
                ec3d_launch_k4d(sw, ec3d_src_of(c, EC3D_BY_K2), ec3d_src_of(c, EC3D_BY_SPMV), c->state, it, ne, xe, pp, sp,
                                v[EC3D_VEC_AS], v[EC3D_VEC_R0], v[EC3D_VEC_X], v[EC3D_VEC_R], c->partials, c->hist,
                                c->hist_cap, s);
        }
        if (xa && group_end && part != 1) ec3d_launch_x_group_of(c, it - xm, xm + 1, it >= c->run.xd_last);
    }
    if ((k == 0 || k == 5) && !f51)
        ec3d_launch_k5(c->sweep_k5, ec3d_src_of(c, EC3D_BY_K4), c->state, it, v[EC3D_VEC_R], AP, P,
                       ec3d_vec_at(c, EC3D_VEC_P, it + 1), v[EC3D_VEC_R0], c->hist, c->hist_cap, s);
    if ((k == 0 || k == 5) && f51)
        ec3d_launch_k51(A, ss, ec3d_src_of(c, EC3D_BY_K4), c->state, it, v[EC3D_VEC_R], P, AP, ec3d_vec_at(c, EC3D_VEC_P, it + 1),
                        ec3d_vec_at(c, EC3D_VEC_AP, it + 1), v[EC3D_VEC_R0], c->partials, c->hist, c->hist_cap, s);
    // (a slab's boundary launch, part 1, is followed by the interior launch of the same stage: that one advances)
    if ((k == 0 || k == 5) && part != 1) ec3d_after_p(c, it);
}

// A new run of iterations on this handle.  Whatever the second stream still holds belongs to the last run and is waited
// for; then every field of the cursor is what a fresh handle has.
void ec3d_run_reset(ec3d_ctx *c)
{
    if (c->xstream && c->run.xg_n > 0) (void)hipStreamWaitEvent(c->stream, c->ev_xdone[(c->run.xg_n - 1) & 1], 0);
    c->run = IterCursor{};
}

int ec3d_run_open(ec3d_ctx *c, int first, int64_t last, const char *who)
{
    // The device state is addressed by the iteration number -- rr0[it & 1], AP in apbuf[it & 1], P and S in their rings --
    // so an iterate call has to continue where the last one ended (its _begin starts again from 1): iterate(1, n) twice
    // would read an older P and the other rr0.
    if (who && first != c->run.it_next) {
        ec3d_set_error(std::string(who) + ": first_iter = " + std::to_string(first) + " does not continue the iterations of "
                       "this handle (next: " + std::to_string(c->run.it_next) + "; " + who + "_begin starts again from 1)");
        return 6;
    }
    // deferred X update: the groups of D are counted from the call's first iteration, its last one applies what is pending
    c->run.xd_base = first;
    c->run.xd_last = (int)std::min<int64_t>(last, INT_MAX);
    return 0;
}

// ec3d_xasync: the X updates of iterations first .. first + count - 1 as a launch of their own on the second stream,
// ordered behind what the main stream holds now (the K4 of the group's last iteration).  Before that, the main stream
// is made to wait for the PREVIOUS group's launch: the kernels that follow write the ring buffers and SolverState
// entries two groups back, i.e. that group's.  join: the main stream also waits for this launch (the last group of a
// call: whoever synchronises the main stream then has X).
void ec3d_launch_x_group_of(ec3d_ctx *c, int first, int count, bool join)
{
    const int d2 = 2 * ec3d_xdefer(c), n = c->run.xg_n;
    const double *pp[EC3D_XD_MAX], *sp[EC3D_XD_MAX];
    pending_bufs(c, first + count - 1, count, pp, sp);
    c->run.xg_n = n + 1;
    c->run.xg_done_upto = first + count - 1;
    if (c->xinline) { // on the iteration's own stream, the vector kernels' grid: ordered by the stream itself
        // (256 ... 768 workgroups instead: the iteration within 0.3 % of the full grid's, profiles/r06_x_groups_own_launch.log)
        ec3d_launch_x_group(c->sweep, c->state, pp, sp, first, count, d2, c->vec[EC3D_VEC_X], 0, c->stream);
        return;
    }
    // 128 workgroups (half a workgroup per CU): beside the iteration's kernels the launch takes a small share of the
    // bandwidth, in the gaps between them -- halo planes under way, sums being gathered -- it has the card to itself.
    // 64 ... 256 measured within 2 % of each other on 7 - 16 Mi-row slabs, the vector kernels' own grid (512 and more) 3 % worse
    // (profiles/r05_x_groups_on_a_second_stream.log).  EC3D_XASYNC_WGS overrides (0: the vector kernels' grid).
    const int wgs = getenv("EC3D_XASYNC_WGS") ? atoi(getenv("EC3D_XASYNC_WGS")) : 128;
    EC3D_NOTE(c, hipEventRecord(c->ev_xready, c->stream));
    if (n > 0) EC3D_NOTE(c, hipStreamWaitEvent(c->stream, c->ev_xdone[(n - 1) & 1], 0));
    EC3D_NOTE(c, hipStreamWaitEvent(c->xstream, c->ev_xready, 0));
    ec3d_launch_x_group(c->sweep, c->state, pp, sp, first, count, d2, c->vec[EC3D_VEC_X], wgs, c->xstream);
    EC3D_NOTE(c, hipEventRecord(c->ev_xdone[n & 1], c->xstream));
    if (join) EC3D_NOTE(c, hipStreamWaitEvent(c->stream, c->ev_xdone[n & 1], 0));
}

// The X updates an exit at iteration stop_iter left pending (deferred X update): enqueued behind everything else.
int ec3d_flush_x(ec3d_ctx *c, int stop_iter)
{
    const int D = ec3d_xdefer(c);
    if (ec3d_xasync(c)) {
        // the groups already enqueued end themselves at the exit (k_x_group); the group the exit lies in may not have
        // been enqueued yet (the host stopped before its last iteration): now, cut at the exit by the kernel itself
        if (stop_iter > c->run.xg_done_upto) ec3d_launch_x_group_of(c, c->run.xg_done_upto + 1, D, true);
        else if (c->run.xg_n > 0 && !c->xinline) EC3D_HIP(hipStreamWaitEvent(c->stream, c->ev_xdone[(c->run.xg_n - 1) & 1], 0));
        EC3D_HIP(hipGetLastError());
        EC3D_ASYNC_CHECK(c);
        return 0;
    }
    if ((D <= 1 && !ec3d_k4s(c)) || stop_iter < c->run.xd_base) return 0;
    const double *pp[EC3D_XD_MAX], *sp[EC3D_XD_MAX];
    pending_bufs(c, stop_iter, (stop_iter - c->run.xd_base) % D + 1, pp, sp);
    ec3d_launch_x_flush(c->sweep, c->state, pp, sp, c->vec[EC3D_VEC_X], c->stream);
    EC3D_HIP(hipGetLastError());
    return 0;
}

void ec3d_launch_iteration(ec3d_ctx *c, const MatView &A, int it) { ec3d_launch_stage(c, A, it, 0); }

int ec3d_launch_begin(ec3d_ctx *c, const MatView &A, double tol, bool null_project)
{
    double **v = c->vec;
    ec3d_launch_residual(A, c->sweep_s, v[EC3D_VEC_X], v[EC3D_VEC_B], v[EC3D_VEC_R], v[EC3D_VEC_R0], v[EC3D_VEC_P],
                         c->partials, c->stream);
    // ec3d_set_null_projection: R = R - Q (Q^T R) before R0, P and R.R are what the iteration starts from (ec3d_null.hip)
    if (null_project) {
        const int rc = ec3d_null_project(c);
        if (rc) return rc;
    }
    ec3d_launch_setup(c->state, ec3d_src_of(c, EC3D_BY_SPMV), tol, c->stream);
    ec3d_run_reset(c);
    EC3D_HIP(hipGetLastError());
    return 0;
}

int ec3d_single_rank_only(ec3d_ctx *c, const char *who)
{
    // c->dist alone (a full-grid handle configured with nranks = 1, the 1-rank rehearsal layout) must be
    // refused as well: its kernels take their sums from gsum, which only the staged driver fills
    if (c->halo > 0 || c->nranks > 1 || c->dist) {
        ec3d_set_error(std::string(who) + ": this handle holds one z-slab of a multi-rank problem; drive it "
                                          "with ec3d_dist_step (eddy_currents_3d_amd/dist.py)");
        return 4;
    }
    return 0;
}

static int ensure_hist(ec3d_ctx *c, int64_t cap)
{
    if (cap <= 0) {
        c->hist_cap = 0;
        return 0;
    }
    EC3D_HIP(c->hist.alloc((size_t)cap * 2));
    EC3D_HIP(hipMemsetAsync(c->hist, 0xFF, (size_t)cap * 2 * sizeof(double), c->stream)); // NaN = "not reached"
    c->hist_cap = cap;
    return 0;
}

static int solve_core(ec3d_ctx *c, double tol, int32_t itmax, int32_t *iter, double *hist_host, int32_t hist_cap,
                      bool print_on_itmax)
{
    const MatView A = c->A.view();
    const int64_t total = std::max<int64_t>(0, (int64_t)itmax + 1); // src/solvers.f90:25-29
    int rc = ensure_hist(c, hist_host ? std::min<int64_t>(hist_cap, total) : 0);
    if (rc) return rc;
    const bool guess = c->guess.depth > 0; // ec3d_set_guess_history: X moved along earlier solutions first (ec3d_guess.hip)
    const bool nullp = c->nullp.on != 0;   // ec3d_set_null_projection: the left null vectors leave the initial residual
    if (nullp && (rc = ec3d_null_prepare(c))) return rc; // (the first solve on a matrix builds them, in the work vectors)
    if (guess && (rc = ec3d_guess_project(c, A))) return rc;
    if ((rc = ec3d_launch_begin(c, A, tol, nullp))) return rc;
    if (guess && (rc = ec3d_guess_note_setup(c))) return rc;
    (void)ec3d_run_open(c, 1, total); // the itmax exit: the last iteration applies what is pending

    // iterations per poll: about 0.4 ms of device work, so an exit is noticed within ~1 ms
    const double est_us = (double)c->A.n_pad * 264.0 / 4.0e6 + 12.0;
    const int chunk = c->mg ? ec3d_mg_chunk(c) : (int)std::min<double>(32.0, std::max<double>(1.0, 400.0 / est_us));
    int64_t launched = 0;
    int ci = 0;
    bool stopped = false;
    while (launched < total && !stopped) {
        const int64_t m = std::min<int64_t>(chunk, total - launched);
        for (int64_t i = 0; i < m; ++i) {
            if (c->mg) ec3d_mg_launch_iteration(c, (int)(++launched)); // ec3d_set_preconditioner (ec3d_mg.hip)
            else ec3d_launch_iteration(c, A, (int)(++launched));
        }
        EC3D_HIP(hipGetLastError());
        EC3D_ASYNC_CHECK(c);
        EC3D_HIP(hipMemcpyAsync(&c->state_pinned[ci & 1], c->state, sizeof(SolverState), hipMemcpyDeviceToHost,
                                c->stream));
        EC3D_HIP(hipEventRecord(c->ev[ci & 1], c->stream));
        if (ci > 0) {
            EC3D_HIP(hipEventSynchronize(c->ev[(ci - 1) & 1]));
            if (c->state_pinned[(ci - 1) & 1].stop_iter != INT_MAX) stopped = true;
        }
        ++ci;
    }
    EC3D_HIP(hipStreamSynchronize(c->stream));
    SolverState fin;
    EC3D_HIP(hipMemcpy(&fin, c->state, sizeof fin, hipMemcpyDeviceToHost));
    if (fin.stop_iter != INT_MAX && fin.npend > 0) { // an exit with X updates pending (deferred X update): apply them
        if ((rc = ec3d_flush_x(c, fin.stop_iter))) return rc;
        EC3D_HIP(hipStreamSynchronize(c->stream));
    }
    if (fin.stop_iter != INT_MAX) {
        *iter = fin.stop_iter;
    } else {
        *iter = (int32_t)total; // itmax exit: the reference prints norm2(R) and returns (:25-28)
        if (print_on_itmax) {
            // ||R|| as the device summed it: the last K5's value (K5 of iteration itmax + 1 ran without an exit), or the
            // setup's when no iteration ran at all (itmax < 0) -- the same number the residual history holds
            if (ec3d_itmax_print_hold) *ec3d_itmax_print_hold = fin.rnorm;
            else ec3d_print_rnorm(fin.rnorm);
        }
    }
    // whichever exit it took: the step this solve made joins the history (not after ||b|| = 0, which moved nothing)
    if (guess && (rc = ec3d_guess_update(c, A, fin.stop_iter != 0))) return rc;
    if (nullp && (rc = ec3d_null_note(c, fin.bnorm))) return rc;
    if (hist_host && c->hist_cap > 0)
        EC3D_HIP(hipMemcpy(hist_host, c->hist, (size_t)c->hist_cap * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ec3d_solve_resident(ec3d_handle c, double tolerance, int32_t itmax, int32_t *iter,
                                   double *resid_hist, int32_t hist_cap)
{
    int rc = ec3d_need_matrix(c, "ec3d_solve_resident");
    if (rc) return rc;
    if ((rc = ec3d_single_rank_only(c, "ec3d_solve_resident"))) return rc;
    return solve_core(c, tolerance, itmax, iter, resid_hist, hist_cap, true);
}

extern "C" int ec3d_solve(ec3d_handle c, const double *b, double *x, double tolerance, int32_t itmax,
                          int32_t *iter, double *resid_hist, int32_t hist_cap)
{
    int rc = ec3d_need_matrix(c, "ec3d_solve");
    if (rc) return rc;
    if ((rc = ec3d_single_rank_only(c, "ec3d_solve"))) return rc;
    if ((rc = ec3d_vec_h2d(c, c->vec[EC3D_VEC_B], b))) return rc;
    if ((rc = ec3d_vec_h2d(c, c->vec[EC3D_VEC_X], x))) return rc;
    if ((rc = solve_core(c, tolerance, itmax, iter, resid_hist, hist_cap, true))) return rc;
    if ((rc = ec3d_vec_d2h(c, x, c->vec[EC3D_VEC_X]))) return rc;
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

