// ec3d_multi.hip — z-slab multi-GPU INSIDE the library: one process, N devices, one host thread per slab.
//
// The reference is serial; its caller (src/EC3D.f90:408) must not have to know that the solve
// runs on several GPUs (SURVEY §8b "Threading").  So the decomposition of eddy_currents_3d_amd/dist.py --
// rank g owns the z-planes [k0, k1), halo planes of P and S once per SpMV, three reduction points per
// iteration, rank-ordered sums -- is driven here from C++, behind one handle:
//
//   * every slab is an ordinary ec3d_ctx on its own device (ec3d_assemble_poisson_slab / ec3d_assemble_slab)
//     and runs the stages of ec3d_dist_step; one host thread per slab enqueues them, so the enqueue cost
//     per iteration does not grow with the number of GPUs;
//   * halo planes are PULLED: the consumer's side stream waits for the neighbour's "boundary rows are final"
//     event and copies the planes out of the neighbour's vector (peer access over xGMI) straight into its own
//     ghost rows -- contiguous, in place, no packing -- while the interior launch runs on the compute stream;
//   * dot products are not gathered at all: every rank collapses its partials into its own lsum[8]
//     (k_finalize), records an event, and the consumer kernels of ALL ranks read the N lsum arrays in place
//     through a pointer table (RedSrc::ptrs) and add them in rank order -- identical decisions everywhere,
//     bit-identical to the staged drivers in dist.py; lsum lives in fine-grained memory;
//   * cross-device ordering is hipStreamWaitEvent on events recorded by the other slabs' threads; a thread
//     announces "recorded" through a per-slab sequence counter the others spin on (every thread runs the
//     same plan, and always posts before it waits, so there is no cycle).
// Several slabs may share one device (tests and rehearsals on a one-GPU box): same code, the peer copies
// become local ones.
//
// ONE PROCESS PER GPU (ec3d_multi_create_rank; what torch.distributed.run launches): the same handle, plans and stages with
// ONE local slab -- this process's rank of `world` -- and RCCL as the transport: the halo planes travel as ncclSend /
// ncclRecv pairs in one group on the side stream (communicator of its own, so the transfer runs beside the interior
// launch), the eight sums of every rank are all-gathered (64 B per rank) on the compute stream and added in rank order by
// the consumer kernels, exactly like the gathered copy of eddy_currents_3d_amd/dist.py.  The whole iteration loop is
// enqueued from C++: no Python between two launches.
//
// What needs no device is NOT here but in ec3d_slab_plan.hpp, where tests/test_slab_plan_host.py reaches it on the CPU: the
// op tables of the plans and the stage launched for each entry, the slabs' bounds, the halo runs and how neighbours' runs
// pair up, the refusals of a job whose ranks disagree, the environment knobs, and the job's decision (decide_job,
// decide_slab).  This file keeps the threads, streams, events, RCCL calls, the watchdog, uploads and downloads, the solve
// loop and the C entry points; finish_setup applies the decision to the handles.
#include "../../include/ec3d_hip.h"
#include "ec3d_internal.hpp"
#include "ec3d_rccl.hpp"
#include "ec3d_slab_plan.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

using namespace ec3d_slab;
static_assert(kXdMax == EC3D_XD_MAX, "decide_job starts from the deepest deferral a handle can allocate rings for");

namespace {
constexpr int RING = 4;

// what a slab holds of its device besides its handle; release() lets go of all of it in the order of declaration, on the
// slab's thread with that device set (ec3d_multi_destroy)
struct SlabDevice {
    Stream side;
    Event ev_ready[NHALO][RING], ev_halo[NHALO][RING], ev_sum[RING], ev_hub[RING];
    Event ev_stop[2];
    PinnedBuf<int32_t> stop_pinned;
    DevBuf<double> lsum;
    DevBuf<const double *> ptr_table; // device: every rank's lsum
    void release() { *this = SlabDevice(); }
};

struct Slab : SlabDevice {
    ec3d_ctx *c = nullptr;
    int rank = 0, device = 0;
    int32_t k0 = 0, k1 = 0, e0 = 0, e1 = 0; // owned planes [k0,k1), held planes [e0,e1)
    bool lsum_fine = false;
    uint64_t api_calls = 0, api_iters = 0; // runtime calls / iterations of the last ec3d_multi_iterate (this rank)
    uint64_t seq[NCH] = {0, 0, 0, 0, 0, 0, 0};
    std::atomic<uint64_t> posted[NCH];
    HaloRuns halo;                                       // the rows I send / receive, DEVICE rows
    std::vector<Copy> pull_lo, pull_hi;                  // my ghost rows <- neighbour's rows
    std::vector<Piece> snd_lo, rcv_lo, snd_hi, rcv_hi;   // RCCL: contiguous pieces of my rows to send / my ghost rows to fill
    bool split_ok = false;   // K2 / K5 can run as boundary + interior launch on this slab
    bool overlap_ok = false; // K1 / K3 can run as interior + boundary launch on this slab
    int plan = 0;            // begin_plan / iter_plan (ec3d_slab_plan.hpp)
    // A-V slab: local reference order [Ax_ext | Ay_ext | Az_ext | U_ext] <-> the global vector
    int64_t nC_ext = 0, nU_ext = 0, n_local = 0;
    std::vector<int32_t> u_glob;        // global U index of every held U unknown
    int64_t own_lo[4] = {0}, own_hi[4] = {0}; // owned rows, local reference numbering
    std::vector<double> io;             // staging for host <-> device copies of an A-V slab
    std::string err;
    // where this slab's thread is (watchdog report): operation, stage / channel, iteration, sequence number
    std::atomic<const char *> at{"idle"};
    std::atomic<int> at_arg{0}, at_it{0};
    std::atomic<uint64_t> at_seq{0};
    Slab() { for (auto &p : posted) p.store(0); }
};

struct Pool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, done_cv;
    std::function<int(int)> job;
    uint64_t gen = 0;
    int pending = 0;
    std::vector<int> rc;
    bool quit = false;
};
} // namespace

struct ec3d_multi {
    int n = 0;     // LOCAL slabs = host threads of this process (all of them, or one: this process's rank)
    int world = 0; // ranks of the job (== n unless one process per GPU)
    // one process per GPU: RCCL transport (ec3d_multi_create_rank)
    const ec3d_rccl_api *nccl = nullptr;
    ncclComm_t comm_halo = nullptr, comm_sum = nullptr;
    int comm_rank = 0, comm_world = 1; // this process in the communicators
    // Rehearsal of ONE rank of a larger job on one GPU (ec3d_multi_create_rank with as_world > nranks = 1): the slab, plan,
    // launches and RCCL calls of rank `as_rank` of `as_world` -- world and Slab::rank then describe THAT geometry -- with
    // every neighbour mapped to this process itself (send / recv to self) and the sums gathered over the one real rank.
    // Timing and call counts are those of the real rank; the numbers computed are not a solution of anything.
    bool rehearse = false;
    DevBuf<double> gsum;       // [world * P_NSLOT] the all-gathered sums
    DevBuf<double> agbuf;      // [(world + 1) * kFacts] set-up exchanges between the ranks
    std::vector<std::unique_ptr<Slab>> slab;
    Pool pool;
    std::atomic<bool> abort{false};
    int kind = 0; // 0: no matrix, 1: single component (ec3d_assemble_poisson), 2: A-V system
    int32_t sdx = 0, sdy = 0, sdz = 0;
    int64_t kdz = 0, nC_glob = 0, nU_glob = 0, n_glob = 0;
    int64_t nnz = 0;
    int chunk = 1; // iterations between two looks at the stop flag: ONE value for the job (ranks leave together)
};

namespace {
// only taken under EC3D_MULTI_SERIALIZE_WAITS=1 (see cross_wait)
std::mutex g_cross_wait;
// HIP runtime calls issued by the slab threads (launches are counted in run_plan): what the host pays per iteration
thread_local uint64_t t_api_calls = 0;
#define MHIP(call)                                                                             \
    do {                                                                                       \
        ++t_api_calls;                                                                         \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            ec3d_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                 \
            return 100;                                                                        \
        }                                                                                      \
    } while (0)

#define MNCCL(m_, call)                                                                        \
    do {                                                                                       \
        ++t_api_calls;                                                                         \
        ncclResult_t e_ = (call);                                                              \
        if (e_ != ncclSuccess) {                                                               \
            ec3d_set_error(std::string(#call) + ": " + (m_)->nccl->GetErrorString(e_));        \
            return 108;                                                                        \
        }                                                                                      \
    } while (0)

void worker(ec3d_multi *m, int r)
{
    Pool &p = m->pool;
    (void)hipSetDevice(m->slab[(size_t)r]->device);
    uint64_t seen = 0;
    for (;;) {
        std::function<int(int)> job;
        {
            std::unique_lock<std::mutex> lk(p.m);
            p.cv.wait(lk, [&] { return p.quit || p.gen != seen; });
            if (p.quit) return;
            seen = p.gen;
            job = p.job;
        }
        int rc = job(r);
        if (rc) {
            m->slab[(size_t)r]->err = ec3d_last_error();
            m->abort.store(true);
        }
        {
            std::lock_guard<std::mutex> lk(p.m);
            p.rc[(size_t)r] = rc;
            if (--p.pending == 0) p.done_cv.notify_all();
        }
    }
}

// run fn(rank) on every slab's thread; first failure wins (its message becomes ec3d_last_error())
// `watch`: the job makes the slabs wait for each other (halo pulls, reduction points), so a stall is possible and the
// watchdog is armed; jobs that only work on their own slab (assembly, uploads, creation) may take as long as they need.
int run_all(ec3d_multi *m, const std::function<int(int)> &fn, bool watch = false)
{
    Pool &p = m->pool;
    {
        std::unique_lock<std::mutex> lk(p.m);
        p.job = fn;
        p.pending = m->n;
        std::fill(p.rc.begin(), p.rc.end(), 0);
        ++p.gen;
        p.cv.notify_all();
        // watchdog: a job that makes no progress for EC3D_MULTI_WATCHDOG seconds (default 120; 0 = off) is a
        // deadlock between the slabs' streams or threads.  Say where every rank stands, let the ranks that
        // still can give up, and end the process if a thread stays stuck inside the runtime: there is no way
        // to cancel it, and the interfaces this library stands behind have no channel for "hung".
        static const int limit_env = getenv("EC3D_MULTI_WATCHDOG") ? atoi(getenv("EC3D_MULTI_WATCHDOG")) : 120;
        const int limit = watch ? limit_env : 0;
        auto report = [&]() {
            std::string r;
            for (auto &s : m->slab)
                r += "  rank " + std::to_string(s->rank) + ": " + s->at.load() + " arg " + std::to_string(s->at_arg.load()) +
                     " it " + std::to_string(s->at_it.load()) + " seq " + std::to_string(s->at_seq.load()) + " posted [" +
                     std::to_string(s->posted[0].load()) + " " + std::to_string(s->posted[1].load()) + " " +
                     std::to_string(s->posted[2].load()) + " " + std::to_string(s->posted[3].load()) + " " +
                     std::to_string(s->posted[4].load()) + " " + std::to_string(s->posted[5].load()) + " " +
                     std::to_string(s->posted[6].load()) + "]\n";
            return r;
        };
        if (limit <= 0) {
            p.done_cv.wait(lk, [&] { return p.pending == 0; });
        } else {
            std::string last;
            for (;;) {
                if (p.done_cv.wait_for(lk, std::chrono::seconds(limit), [&] { return p.pending == 0; })) break;
                const std::string now = report();
                if (now != last) { // still moving (a long solve): keep waiting
                    last = now;
                    continue;
                }
                fprintf(stderr, "libec3d_hip: multi-GPU job stalled for %d s:\n%s", limit, now.c_str());
                fflush(stderr);
                m->abort.store(true);
                if (p.done_cv.wait_for(lk, std::chrono::seconds(10), [&] { return p.pending == 0; })) break;
                // no signal, no core dump of a 100 GB process, an exit status the caller's shell can read; never a
                // re-exec (the process has touched the GPU)
                fprintf(stderr, "libec3d_hip: a rank is stuck inside the HIP runtime; ending the process (exit status 86)\n");
                fflush(stderr);
                fflush(stdout);
                _Exit(86);
            }
        }
    }
    int rc = 0;
    for (int r = 0; r < m->n; ++r)
        if (p.rc[(size_t)r]) {
            // a rank that only gave up because another one failed reports 90
            if (!rc || rc == 90) {
                rc = p.rc[(size_t)r];
                ec3d_set_error("rank " + std::to_string(r) + ": " + m->slab[(size_t)r]->err);
            }
        }
    if (m->abort.load()) { // leave every stream idle and the channels aligned for the next call
        for (auto &s : m->slab) {
            (void)hipSetDevice(s->device);
            (void)hipDeviceSynchronize();
            for (int ch = 0; ch < NCH; ++ch) {
                s->seq[ch] = 0;
                s->posted[ch].store(0);
            }
        }
        m->abort.store(false);
    }
    return rc;
}

int wait_posted(ec3d_multi *m, Slab &me, Slab &peer, int ch, uint64_t q)
{
    int spins = 0;
    me.at.store("wait_posted");
    me.at_arg.store(ch * 100 + peer.rank);
    me.at_seq.store(q);
    while (peer.posted[ch].load(std::memory_order_acquire) < q) {
        if (m->abort.load(std::memory_order_relaxed)) {
            ec3d_set_error("gave up: another rank failed");
            return 90;
        }
        if (++spins > 256) std::this_thread::yield();
    }
    return 0;
}

int cross_wait(hipStream_t stream, hipEvent_t ev)
{
    // hipStreamWaitEvent is thread safe like every HIP entry point and the threads issue these waits concurrently.
    // Rounds 2 and 3 took a process-wide mutex around every one of them by default -- "a precaution, not a measured
    // need": eight rank threads then queued up behind it at every reduction point and exchange.  It protected against
    // nothing that was ever observed (the suite's 2-8 slab cases and tools/multi_stress.py -- 3, 4 and 8 slabs on one card,
    // 20 x 7 repeated solves each, bit-identical every time: profiles/r04_multi_stress.log -- run with it off), so it is now
    // off; EC3D_MULTI_SERIALIZE_WAITS=1 brings it back for a run that wants to rule the runtime out.
    static const bool serialize = getenv("EC3D_MULTI_SERIALIZE_WAITS") && atoi(getenv("EC3D_MULTI_SERIALIZE_WAITS")) != 0;
    if (serialize) {
        std::lock_guard<std::mutex> lk(g_cross_wait);
        MHIP(hipStreamWaitEvent(stream, ev, 0));
    } else {
        MHIP(hipStreamWaitEvent(stream, ev, 0));
    }
    return 0;
}

constexpr int kPlainVec = INT_MIN; // `it` of a caller that means the plain work vector (uploads, probes, the time loop's X)
// Vector `vec` of iteration `it` in slab `owner`'s memory: the ring position from MY handle's cursor, the pointer from
// the owner's tables, which do not change while a job runs -- another rank's thread may be iterations ahead or behind
// with its own host-side bookkeeping (ec3d_vec_at)
double *vec_of(const ec3d_ctx *me, const ec3d_ctx *owner, int vec, int it)
{
    return it == kPlainVec ? owner->vec[vec] : ec3d_vec_at(me, owner, vec, it);
}

int halo_start(ec3d_multi *m, Slab &s, int v, int it = kPlainVec)
{
    const uint64_t q = ++s.seq[v];
    const int i = (int)(q % RING), vi = kVecOf[v];
    s.at.store("halo_start:record");
    s.at_arg.store(v);
    s.at_seq.store(q);
    MHIP(hipEventRecord(s.ev_ready[v][i], s.c->stream));
    s.posted[v].store(q, std::memory_order_release);
    // my own earlier readers of the ghost rows are behind this point of my compute stream
    MHIP(hipStreamWaitEvent(s.side, s.ev_ready[v][i], 0));
    if (m->nccl) {
        // one process per GPU: my boundary rows go out and my ghost rows come in as send / recv pairs of ONE group on the
        // side stream (the neighbour's matching pair is in its group; lower neighbour first on every rank)
        // (the k-th send to a neighbour meets its k-th receive from me: both sides list the blocks in the same order)
        double *mine = vec_of(s.c, s.c, vi, it);
        const bool lo = s.rank > 0 && !(s.snd_lo.empty() && s.rcv_lo.empty());
        const bool hi = s.rank + 1 < m->world && !(s.snd_hi.empty() && s.rcv_hi.empty());
        if (lo || hi) {
            s.at.store("halo_start:rccl group");
            MNCCL(m, m->nccl->GroupStart());
            if (lo) {
                const int pr = m->rehearse ? m->comm_rank : s.rank - 1;
                for (const Piece &c : s.snd_lo) MNCCL(m, m->nccl->Send(mine + c.off, (size_t)c.cnt, ncclDouble, pr, m->comm_halo, s.side));
                for (const Piece &c : s.rcv_lo) MNCCL(m, m->nccl->Recv(mine + c.off, (size_t)c.cnt, ncclDouble, pr, m->comm_halo, s.side));
            }
            if (hi) {
                const int pr = m->rehearse ? m->comm_rank : s.rank + 1;
                for (const Piece &c : s.snd_hi) MNCCL(m, m->nccl->Send(mine + c.off, (size_t)c.cnt, ncclDouble, pr, m->comm_halo, s.side));
                for (const Piece &c : s.rcv_hi) MNCCL(m, m->nccl->Recv(mine + c.off, (size_t)c.cnt, ncclDouble, pr, m->comm_halo, s.side));
            }
            MNCCL(m, m->nccl->GroupEnd());
        }
        MHIP(hipEventRecord(s.ev_halo[v][i], s.side));
        return 0;
    }
    for (int dir = -1; dir <= 1; dir += 2) {
        const std::vector<Copy> &cp = dir < 0 ? s.pull_lo : s.pull_hi;
        const int pr = s.rank + dir;
        if (pr < 0 || pr >= m->n || cp.empty()) continue;
        Slab &peer = *m->slab[(size_t)pr];
        int rc = wait_posted(m, s, peer, v, q);
        if (rc) return rc;
        s.at.store("halo_start:cross_wait");
        if ((rc = cross_wait(s.side, peer.ev_ready[v][i]))) return rc;
        s.at.store("halo_start:copy");
        double *mine = vec_of(s.c, s.c, vi, it);
        const double *theirs = vec_of(s.c, peer.c, vi, it);
        // EC3D_MULTI_FORCE_PEER_API=1: the peer-copy call also between slabs of ONE device (tests on a one-GPU box)
        static const bool force_peer = getenv("EC3D_MULTI_FORCE_PEER_API") && atoi(getenv("EC3D_MULTI_FORCE_PEER_API")) != 0;
        for (const Copy &c : cp) {
            if (peer.device == s.device && !force_peer)
                MHIP(hipMemcpyAsync(mine + c.dst, theirs + c.src, (size_t)c.cnt * 8, hipMemcpyDeviceToDevice, s.side));
            else
                MHIP(hipMemcpyPeerAsync(mine + c.dst, s.device, theirs + c.src, peer.device, (size_t)c.cnt * 8, s.side));
        }
    }
    MHIP(hipEventRecord(s.ev_halo[v][i], s.side));
    return 0;
}

int halo_wait(Slab &s, int v)
{
    if (s.seq[v] == 0) return 0;
    MHIP(hipStreamWaitEvent(s.c->stream, s.ev_halo[v][(int)(s.seq[v] % RING)], 0));
    return 0;
}

// "gather": nothing moves -- my lsum is final behind my event; my next kernel may read everybody's once all
// events are behind it.  All-to-all waits would cost N-1 cross-stream waits per rank and point (measured on
// one card: 74 / 157 / 373 / 1022 us of enqueue time per iteration at 1 / 2 / 4 / 8 slabs).  Instead the "final"
// events are folded up a binomial tree: rank r waits for its children r + 2^j (every j with r % 2^(j+1) == 0 and
// r + 2^j < N; a child's event is recorded behind the child's own waits, so it covers the child's whole subtree),
// records its own event, and rank 0 -- behind its log2(N) children -- records ONE event every other rank waits
// for.  Waits per reduction point: N - 1 going up (at most ceil(log2 N) on any one rank: 3 on rank 0 at N = 8, where
// a flat hub issued 7) plus N - 1 going down.  EC3D_MULTI_FLAT_HUB=1 restores the flat hub.
int gather(ec3d_multi *m, Slab &s)
{
    const uint64_t q = ++s.seq[CH_SUM];
    const int i = (int)(q % RING);
    s.at.store("gather:record");
    s.at_seq.store(q);
    if (m->nccl) {
        // one process per GPU: every rank's eight sums to every rank (64 B each), on the compute stream, where the
        // producer's collapse launch wrote them and the consumer kernel reads the gathered copy
        s.at.store("gather:rccl all_gather");
        MNCCL(m, m->nccl->AllGather(s.lsum, m->gsum, P_NSLOT, ncclDouble, m->comm_sum, s.c->stream));
        return 0;
    }
    if (m->n == 1) return 0;
    static const bool flat = getenv("EC3D_MULTI_FLAT_HUB") && atoi(getenv("EC3D_MULTI_FLAT_HUB")) != 0;
    Slab &hub = *m->slab[0];
    int rc = 0;
    // children of this rank in the tree (flat hub: every other rank is a child of rank 0)
    for (int step = 1; step < m->n; step <<= 1) {
        if (flat ? s.rank != 0 : (s.rank & (2 * step - 1)) != 0) break;
        const int lo = flat ? 1 : s.rank + step, hi = flat ? m->n : std::min(m->n, lo + 1);
        for (int h = lo; h < hi; ++h) {
            Slab &peer = *m->slab[(size_t)h];
            if ((rc = wait_posted(m, s, peer, CH_SUM, q))) return rc;
            s.at.store("gather:cross_wait");
            if ((rc = cross_wait(s.c->stream, peer.ev_sum[i]))) return rc;
        }
        if (flat) break;
    }
    if (s.rank != 0) {
        MHIP(hipEventRecord(s.ev_sum[i], s.c->stream)); // behind my sums and my subtree's
        s.posted[CH_SUM].store(q, std::memory_order_release);
        if ((rc = wait_posted(m, s, hub, CH_HUB, q))) return rc;
        s.at.store("gather:cross_wait hub");
        return cross_wait(s.c->stream, hub.ev_hub[i]);
    }
    MHIP(hipEventRecord(s.ev_hub[i], s.c->stream)); // behind rank 0's own sums and everybody else's
    s.posted[CH_HUB].store(q, std::memory_order_release);
    return 0;
}


struct StageTimer {
    std::vector<Event> ev;      // pairs
    std::vector<int> kern;      // 0 .. 4: the stage's kernel; T_GATHER / T_HALO_WAIT: a reduction point / a wait for halo planes
    bool sync_points = false;   // bracket the reduction points and the halo waits on the compute stream as well
};
enum { T_GATHER = 5, T_HALO_WAIT = 6 };
// instrumented pass: how long the compute stream stands at a reduction point / a wait for halo planes (an event in front, one
// behind: with nothing to wait for, the pair measures what two events cost)
template <class F> int timed_sync(StageTimer *tm, Slab &s, int kind, F &&f)
{
    if (!tm || !tm->sync_points) return f();
    Event a, b;
    MHIP(a.create());
    MHIP(b.create());
    MHIP(hipEventRecord(a, s.c->stream));
    int rc = f();
    if (rc) return rc;
    MHIP(hipEventRecord(b, s.c->stream));
    tm->ev.push_back(std::move(a));
    tm->ev.push_back(std::move(b));
    tm->kern.push_back(kind);
    return 0;
}

int run_plan(ec3d_multi *m, Slab &s, const std::vector<Op> &plan, int it, double tol, StageTimer *tm)
{
    int rc = 0;
    s.at_it.store(it);
    for (size_t oi = 0; oi < plan.size(); ++oi) {
        const Op &op = plan[oi];
        switch (op.kind) {
        case OP_HALO:
            if ((rc = halo_start(m, s, op.arg, it + op.dit))) return rc;
            if ((rc = timed_sync(tm, s, T_HALO_WAIT, [&] { return halo_wait(s, op.arg); }))) return rc;
            break;
        case OP_HALO_START: if ((rc = halo_start(m, s, op.arg, it + op.dit))) return rc; break;
        case OP_HALO_WAIT: if ((rc = timed_sync(tm, s, T_HALO_WAIT, [&] { return halo_wait(s, op.arg); }))) return rc; break;
        case OP_GATHER: if ((rc = timed_sync(tm, s, T_GATHER, [&] { return gather(m, s); }))) return rc; break;
        case OP_SKIP_IF_AP: // AP = A P of this iteration came out of the last K5-in-K1: no lone K1, no sum, no exchange
            if (it != 1 && s.c->run.ap_valid_for == it) oi += (size_t)op.arg;
            break;
        default: {
            const int st = launched_stage(s.plan, s.split_ok, s.overlap_ok, op.arg);
            if (st < 0) break;
            s.at.store("stage");
            s.at_arg.store(st);
            const int k = tm ? kernel_of_stage(st) : -1;
            t_api_calls += (uint64_t)ec3d_dist_launches(s.c, st, it); // the kernel launches of the stage
            if (k >= 0) {
                Event a, b;
                MHIP(a.create());
                MHIP(b.create());
                MHIP(hipEventRecord(a, s.c->stream));
                rc = ec3d_dist_step(s.c, st, it, tol);
                MHIP(hipEventRecord(b, s.c->stream));
                tm->ev.push_back(std::move(a));
                tm->ev.push_back(std::move(b));
                tm->kern.push_back(k);
            } else {
                rc = ec3d_dist_step(s.c, st, it, tol);
            }
            if (rc) return rc;
        }
        }
    }
    return 0;
}

int drain(Slab &s)
{
    s.at.store("drain:side stream");
    MHIP(hipStreamSynchronize(s.side));
    s.at.store("drain:compute stream");
    MHIP(hipStreamSynchronize(s.c->stream));
    s.at.store("idle");
    return 0;
}

// Peer access from this slab's device to every other device that holds a slab.  Runs on every slab's thread BEFORE
// anything is allocated (ec3d_multi_create), so that every allocation a peer will touch -- the work vectors the
// halo planes are pulled from, lsum, which the peers' kernels dereference -- is made with the mappings in place.
int enable_peers(ec3d_multi *m, Slab &s)
{
    MHIP(hipSetDevice(s.device));
    for (auto &o : m->slab) {
        if (o->device == s.device) continue;
        int can = 0;
        MHIP(hipDeviceCanAccessPeer(&can, s.device, o->device));
        if (!can) {
            ec3d_set_error("ec3d_multi: device " + std::to_string(s.device) + " cannot access device " +
                           std::to_string(o->device) + " (no peer path)");
            return 104;
        }
        hipError_t e = hipDeviceEnablePeerAccess(o->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
            ec3d_set_error(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
            return 100;
        }
        (void)hipGetLastError();
    }
    return 0;
}

// (re)create the per-slab context and the multi-rank plumbing around it
int slab_reset(ec3d_multi *m, Slab &s)
{
    MHIP(hipSetDevice(s.device));
    if (!s.c) {
        int rc = ec3d_create(&s.c, s.device);
        if (rc == 0) s.c->in_multi = true;
        if (rc) return rc;
        MHIP(s.side.create(hipStreamNonBlocking));
        for (int v = 0; v < NHALO; ++v)
            for (int i = 0; i < RING; ++i) {
                MHIP(s.ev_ready[v][i].create(hipEventDisableTiming));
                MHIP(s.ev_halo[v][i].create(hipEventDisableTiming));
            }
        for (int i = 0; i < RING; ++i) MHIP(s.ev_sum[i].create(hipEventDisableTiming));
        for (int i = 0; i < RING; ++i) MHIP(s.ev_hub[i].create(hipEventDisableTiming));
        for (int i = 0; i < 2; ++i) MHIP(s.ev_stop[i].create(hipEventDisableTiming));
        MHIP(s.stop_pinned.alloc(2));
        // The 8 sums every other GPU's kernels read in place, launch after launch: fine-grained (coherent across
        // devices) memory.  Peer access between all the devices involved was enabled BEFORE this allocation
        // (enable_peers, ec3d_multi_create).  Plain hipMalloc memory is only good enough when every slab sits
        // on this same device (rehearsals on a one-GPU box); across devices there is no silent fallback.
        bool several_devices = false;
        for (auto &o : m->slab) several_devices |= o->device != s.device;
        if (s.lsum.alloc_fine(P_NSLOT) == hipSuccess) {
            s.lsum_fine = true;
        } else {
            (void)hipGetLastError();
            if (several_devices) {
                ec3d_set_error("ec3d_multi: device " + std::to_string(s.device) + " cannot allocate fine-grained memory "
                               "(hipDeviceMallocFinegrained) for the partial sums the other GPUs "
                               "read in place; coarse-grained memory is not coherent across devices -- refusing to run "
                               "on several devices without it");
                return 107;
            }
            MHIP(s.lsum.alloc(P_NSLOT));
        }
        MHIP(hipMemset(s.lsum, 0, P_NSLOT * sizeof(double)));
        MHIP(s.ptr_table.alloc((size_t)m->n));
    }
    s.halo = HaloRuns{};
    s.pull_lo.clear(); s.pull_hi.clear();
    s.u_glob.clear();
    s.split_ok = false;
    s.plan = 0;
    return 0;
}

// what a rank tells the others of its slab (RankFacts, ec3d_slab_plan.hpp)
RankFacts facts_of(const Slab &sl)
{
    const ec3d_ctx *c = sl.c;
    RankFacts f{};
    f.fused_ok = (c->fuse23_ok && c->fuse51_ok && c->k4s_ok && c->pp_base && c->own_vectors()) ? 1.0 : 0.0;
    f.xd = (c->pp_base && c->own_vectors()) ? (double)c->xdefer : 1.0;
    f.xasync = (c->pp_base && c->own_vectors() && c->xasync_cap) ? 1.0 : 0.0;
    // (an A-V slab splits K2 / K5 by tile lists made from its halo runs: always possible where there is a neighbour)
    f.both_splits = (c->have_matrix && c->split_s.ok && (c->A.sav || ec3d_dist_can_split_planes(c))) ? 1.0 : 0.0;
    f.sav = c->A.sav ? 1.0 : 0.0;
    f.n_pad = (double)c->A.n_pad;
    f.fsplit = c->split_f.ok ? 1.0 : 0.0;
    halo_facts(sl.halo, f);
    return f;
}

// after every slab has its matrix: the halo copy lists or pieces, every rank's facts, the neighbours' agreement, the job's
// decision (all four stated in ec3d_slab_plan.hpp) and, on every slab's thread, what it means for that handle
int finish_setup(ec3d_multi *m, const SlabKnobs &knob)
{
    int rc = 0;
    std::string why;
    std::vector<RankFacts> facts((size_t)(m->nccl ? m->comm_world : m->n));
    if (m->nccl) { // one process per GPU: my pieces; every rank's facts all-gathered
        Slab &s = *m->slab[0];
        s.snd_lo = pieces_of(s.halo.send_lo);
        s.rcv_lo = pieces_of(s.halo.recv_lo);
        s.snd_hi = pieces_of(s.halo.send_hi);
        s.rcv_hi = pieces_of(s.halo.recv_hi);
        const RankFacts mine = facts_of(s);
        rc = run_all(m, [&](int) -> int {
            double *snd = m->agbuf + (size_t)m->comm_world * kFacts;
            MHIP(hipMemcpyAsync(snd, &mine, sizeof mine, hipMemcpyHostToDevice, s.c->stream));
            MNCCL(m, m->nccl->AllGather(snd, m->agbuf, kFacts, ncclDouble, m->comm_sum, s.c->stream));
            MHIP(hipMemcpyAsync(facts.data(), m->agbuf, facts.size() * sizeof(RankFacts), hipMemcpyDeviceToHost, s.c->stream));
            MHIP(hipStreamSynchronize(s.c->stream));
            return 0;
        }, true);
        if (rc) return rc;
    } else { // one process: my ghost rows <- the neighbours' rows; the facts read off the slabs
        for (int g = 0; g < m->n && !rc; ++g) {
            Slab &s = *m->slab[(size_t)g];
            if (g + 1 < m->n) rc = pair_up(s.halo.recv_hi, m->slab[(size_t)g + 1]->halo.send_lo, s.pull_hi, why);
            if (g > 0 && !rc) rc = pair_up(s.halo.recv_lo, m->slab[(size_t)g - 1]->halo.send_hi, s.pull_lo, why);
            facts[(size_t)g] = facts_of(s);
        }
    }
    if (!rc) rc = check_neighbours(facts, m->nccl != nullptr, why);
    if (rc) {
        ec3d_set_error(why);
        return rc;
    }
    const JobPlan job = decide_job(facts, m->kind, m->world, knob);
    m->chunk = job.chunk;
    std::vector<const double *> tab((size_t)m->n);
    for (int g = 0; g < m->n; ++g) tab[(size_t)g] = m->slab[(size_t)g]->lsum;
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        MHIP(hipMemcpy(s.ptr_table, tab.data(), tab.size() * sizeof(double *), hipMemcpyHostToDevice));
        ec3d_ctx *c = s.c;
        c->dist = true;
        c->nranks = m->nccl ? m->comm_world : m->world;
        c->lsum = s.lsum;
        c->gsum = m->nccl ? m->gsum : nullptr;          // one process per GPU: the all-gathered copy
        c->lsum_ptrs = m->nccl ? nullptr : s.ptr_table.get(); // one process: every rank's sums read in place
        c->slab_fused = job.fused;
        c->slab_xd = job.xd;
        c->slab_xasync = job.xasync;
        const SlabPlan sp = decide_slab(job, m->kind, m->world, s.rank, knob, ec3d_can_overlap(c) != 0);
        c->sweep_s.halo_store = sp.halo_store;
        c->split_f.bnd.halo_store = c->split_f.inte.halo_store = c->sweep_s.halo_store;
        if (c->pp_base) { // every rank cycles P and S through the same number of buffers
            const int D = ec3d_xdefer(c), depth = ec3d_xasync(c) ? 2 * D : D;
            c->pdepth = std::max(2, depth);
            c->sdepth = std::max(1, depth);
        }
        s.plan = sp.plan;
        s.overlap_ok = sp.overlap_ok;
        int32_t en = 0;
        int rc2 = 0;
        if (sp.split == SPLIT_PLANES) {
            rc2 = ec3d_dist_set_boundary_planes(c, &en);
        } else if (sp.split == SPLIT_ROWS) {
            std::vector<int64_t> lo, hi;
            boundary_rows(s.halo, lo, hi);
            if (!lo.empty()) rc2 = ec3d_dist_set_boundary_rows(c, (int32_t)lo.size(), lo.data(), hi.data(), &en);
        }
        s.split_ok = en != 0;
        return rc2;
    });
}

// What the four set-up entry points share.  The job's grid is recorded; every slab's thread makes its handle anew, takes
// its planes [k0, k1) and the ones it holds (an A-V slab, kind 2: two halo planes per interior side) and calls
// matrix_and_runs(slab) for the slab's matrix, sizes and halo runs; then the job is of `kind` and finish_setup agrees
// on its plan.  nnz < 0: the sum of the slabs' counts.
int setup_job(ec3d_multi *m, const SlabKnobs &knob, int kind, int64_t sdx, int64_t sdy, int64_t sdz, int64_t nU_glob,
              int64_t n_glob, int64_t nnz, const std::function<int(Slab &)> &matrix_and_runs)
{
    m->kind = 0;
    m->sdx = (int32_t)sdx; m->sdy = (int32_t)sdy; m->sdz = (int32_t)sdz;
    m->kdz = sdx * sdy;
    m->nC_glob = m->kdz * sdz;
    m->nU_glob = nU_glob;
    m->n_glob = n_glob;
    int rc = run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = slab_reset(m, s);
        if (rc2) return rc2;
        slab_bounds((int)sdz, s.rank, m->world, s.k0, s.k1);
        held_range((int)sdz, s.k0, s.k1, kind == 2 ? 2 : 0, s.e0, s.e1);
        return matrix_and_runs(s);
    });
    if (rc) return rc;
    m->kind = kind;
    m->nnz = std::max<int64_t>(nnz, 0);
    for (auto &s : m->slab)
        if (nnz < 0) m->nnz += s->c->A.nnz;
    return finish_setup(m, knob);
}

// sizes and halo runs of a slab of `rows` rows of the single-component operator
int cube_slab_layout(const ec3d_multi *m, Slab &s, int64_t rows)
{
    std::string why;
    s.n_local = rows;
    const int rc = cube_runs(s.rank, m->world, m->kdz, rows, s.c->ghost, s.halo, why);
    if (rc) ec3d_set_error(why);
    return rc;
}

// sizes, owned ranges and halo runs of an A-V slab whose matrix is in place, nU held U unknowns behind three blocks of the
// held planes' cells; upl[p] = held conducting cells before held plane p
void av_slab_layout(const ec3d_multi *m, Slab &s, const SlabKnobs &knob, int64_t nU, const std::vector<int64_t> &upl)
{
    s.nC_ext = (int64_t)(s.e1 - s.e0) * m->kdz;
    s.nU_ext = nU;
    s.n_local = 3 * s.nC_ext + nU;
    const AvSlab g{s.c->A.sav != 0, s.c->nCd, s.c->pitch, m->kdz, s.nC_ext, s.nU_ext, s.k0, s.k1, s.e0, s.e1};
    const AvLayout L = av_layout(g, upl, knob.u_always(), m->rehearse);
    std::copy(L.own_lo, L.own_lo + 4, s.own_lo);
    std::copy(L.own_hi, L.own_hi + 4, s.own_hi);
    s.halo = L.runs;
}

__global__ void k_fill(double *p, int64_t n, double v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// NaN into every row of work vector `vi` that the halo exchange is about to fill (the recv runs), on the slab's
// compute stream: a pull that comes late, copies the wrong rows or never happens then shows in the result instead
// of leaving behind whatever was uploaded there.  Only rows the exchange WRITES are touched: halo rows no owned row
// reads (the outer halo plane of the A blocks) keep their finite values, since a band coefficient of zero still
// multiplies its operand.
int poison_recv_rows(Slab &s, int vi)
{
    double *v = s.c->vec[vi];
    const double nan = std::nan("");
    for (const std::vector<Run> *rs : {&s.halo.recv_lo, &s.halo.recv_hi})
        for (const Run &r : *rs)
            for (int p = 0; p < r.planes; ++p) {
                if (r.payload <= 0) continue;
                k_fill<<<(unsigned)((r.payload + 255) / 256), 256, 0, s.c->stream>>>(v + r.start + (int64_t)p * r.pitch,
                                                                                        r.payload, nan);
                MHIP(hipGetLastError());
            }
    return 0;
}

int need(ec3d_multi *m, const char *who)
{
    if (!m || m->kind == 0) {
        ec3d_set_error(std::string(who) + ": no matrix (call ec3d_multi_assemble* first)");
        return 3;
    }
    return 0;
}

// host vector in the reference's global numbering -> this slab's work vector (owned AND halo entries)
int slab_upload(ec3d_multi *m, Slab &s, int which, const double *glob)
{
    ec3d_ctx *c = s.c;
    int rc = 0;
    if (m->kind == 1) {
        rc = ec3d_vec_h2d(c, c->vec[which], glob + (int64_t)s.k0 * m->kdz);
    } else {
        s.io.resize((size_t)s.n_local);
        for (int d = 0; d < 3; ++d)
            memcpy(s.io.data() + (size_t)d * s.nC_ext, glob + d * m->nC_glob + (int64_t)s.e0 * m->kdz,
                   (size_t)s.nC_ext * sizeof(double));
        double *u = s.io.data() + (size_t)3 * s.nC_ext;
        const double *gu = glob + 3 * m->nC_glob;
        for (int64_t q = 0; q < s.nU_ext; ++q) u[q] = gu[s.u_glob[(size_t)q]];
        rc = ec3d_vec_h2d(c, c->vec[which], s.io.data());
    }
    if (rc) return rc;
    MHIP(hipStreamSynchronize(c->stream));
    return 0;
}

// the OWNED entries of this slab's work vector -> the global host vector
int slab_download(ec3d_multi *m, Slab &s, int which, double *glob)
{
    ec3d_ctx *c = s.c;
    int rc = 0;
    if (m->kind == 1) {
        if ((rc = ec3d_vec_d2h(c, glob + (int64_t)s.k0 * m->kdz, c->vec[which]))) return rc;
        MHIP(hipStreamSynchronize(c->stream));
        return 0;
    }
    s.io.resize((size_t)s.n_local);
    if ((rc = ec3d_vec_d2h(c, s.io.data(), c->vec[which]))) return rc;
    MHIP(hipStreamSynchronize(c->stream));
    for (int d = 0; d < 3; ++d)
        memcpy(glob + d * m->nC_glob + (int64_t)s.k0 * m->kdz, s.io.data() + (size_t)s.own_lo[d],
               (size_t)(s.own_hi[d] - s.own_lo[d]) * sizeof(double));
    double *gu = glob + 3 * m->nC_glob;
    for (int64_t q = s.own_lo[3]; q < s.own_hi[3]; ++q) gu[s.u_glob[(size_t)(q - 3 * s.nC_ext)]] = s.io[(size_t)q];
    return 0;
}

// one reference solve on the resident slabs (src/solvers.f90:3-50); every rank returns the same iter
int slab_solve(ec3d_multi *m, Slab &s, double tol, int32_t itmax, int32_t *iter_out, int *hit_itmax)
{
    ec3d_ctx *c = s.c;
    const int64_t total = std::max<int64_t>(0, (int64_t)itmax + 1); // src/solvers.f90:25-29
    int rc = run_plan(m, s, begin_plan(s.plan), 0, tol, nullptr);
    if (rc) return rc;
    (void)ec3d_run_open(c, 1, total); // the itmax exit: the last iteration applies the pending X updates
    // every rank must look at the flag after the same iterations, so the chunk is a property of the job
    // (finish_setup: from the largest slab), not of this slab
    const int chunk = m->chunk;
    int64_t launched = 0;
    int ci = 0;
    bool stopped = false;
    // every rank derives the same decisions from the same sums, so all see the flag at the same chunk and
    // leave together; iterations enqueued past the exit return at once and touch nothing
    while (launched < total && !stopped) {
        const int64_t n = std::min<int64_t>(chunk, total - launched);
        for (int64_t i = 0; i < n; ++i)
            if ((rc = run_plan(m, s, iter_plan(s.plan), (int)(++launched), 0.0, nullptr))) return rc;
        if ((rc = ec3d_read_state_async(c, &s.stop_pinned[ci & 1]))) return rc;
        MHIP(hipEventRecord(s.ev_stop[ci & 1], c->stream));
        if (ci > 0) {
            s.at.store("solve:wait for the previous chunk's stop flag");
            MHIP(hipEventSynchronize(s.ev_stop[(ci - 1) & 1]));
            if (s.stop_pinned[(ci - 1) & 1] != INT_MAX) stopped = true;
        }
        ++ci;
    }
    if ((rc = drain(s))) return rc;
    int32_t si = 0;
    if ((rc = ec3d_read_state(c, &si, nullptr, nullptr))) return rc;
    if (si >= 0) { // an exit with X updates pending (deferred X update, K4 in SpMV form): applied now, on the owned rows
        if ((rc = ec3d_flush_x(c, si))) return rc;
        MHIP(hipStreamSynchronize(c->stream));
    }
    *iter_out = si >= 0 ? si : (int32_t)total;
    *hit_itmax = si < 0;
    return 0;
}
} // namespace

// ---------------------------------------------------------------------------------------------
extern "C" int ec3d_multi_create(ec3d_multi_handle *mh, int32_t nranks, const int32_t *devices)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        ec3d_set_error("ec3d_multi_create: no HIP device available (this library has no CPU path)");
        return 101;
    }
    if (nranks < 1 || nranks > 64) {
        ec3d_set_error("ec3d_multi_create: nranks must be 1..64");
        return 2;
    }
    if (!devices && nranks > ndev) {
        ec3d_set_error("ec3d_multi_create: needs " + std::to_string(nranks) + " devices, this machine has " +
                       std::to_string(ndev));
        return 103;
    }
    for (int r = 0; devices && r < nranks; ++r)
        if (devices[r] < 0 || devices[r] >= ndev) {
            ec3d_set_error("ec3d_multi_create: device ordinal " + std::to_string(devices[r]) + " out of range (" +
                           std::to_string(ndev) + " devices)");
            return 102;
        }
    ec3d_multi *m = new ec3d_multi();
    m->n = nranks;
    m->world = nranks;
    for (int r = 0; r < nranks; ++r) {
        m->slab.emplace_back(new Slab());
        m->slab.back()->rank = r;
        m->slab.back()->device = devices ? devices[r] : r;
    }
    m->pool.rc.assign((size_t)nranks, 0);
    for (int r = 0; r < nranks; ++r) m->pool.th.emplace_back(worker, m, r);
    int rc = run_all(m, [&](int r) { return enable_peers(m, *m->slab[(size_t)r]); }); // all of them, then allocate
    if (!rc) rc = run_all(m, [&](int r) { return slab_reset(m, *m->slab[(size_t)r]); });
    if (rc) {
        std::string keep = ec3d_last_error();
        ec3d_multi_destroy(m);
        ec3d_set_error(keep);
        return rc;
    }
    *mh = m;
    return 0;
}

// ---- one process per GPU ------------------------------------------------------------------------------------
extern "C" int ec3d_rccl_unique_id(void *id128)
{
    std::string why;
    const ec3d_rccl_api *api = ec3d_rccl_load(why);
    if (!api || !id128) {
        ec3d_set_error("ec3d_rccl_unique_id: " + (api ? std::string("no buffer") : why));
        return api ? 2 : 109;
    }
    static_assert(sizeof(ncclUniqueId) == 128, "the C ABI hands the id around as 128 bytes");
    ncclUniqueId id;
    ncclResult_t e = api->GetUniqueId(&id);
    if (e != ncclSuccess) {
        ec3d_set_error(std::string("ncclGetUniqueId: ") + api->GetErrorString(e));
        return 108;
    }
    memcpy(id128, &id, sizeof id);
    return 0;
}

extern "C" int ec3d_multi_create_rank(ec3d_multi_handle *mh, int32_t rank, int32_t nranks, int32_t device,
                                      const void *id_halo, const void *id_sum, int32_t as_rank, int32_t as_world)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        ec3d_set_error("ec3d_multi_create_rank: no HIP device available (this library has no CPU path)");
        return 101;
    }
    if (nranks < 1 || rank < 0 || rank >= nranks || device < 0 || device >= ndev || !id_halo || !id_sum) {
        ec3d_set_error("ec3d_multi_create_rank: need 0 <= rank < nranks, a device of this machine and two unique ids");
        return 2;
    }
    const bool rehearse = as_world > 0;
    if (rehearse && (nranks != 1 || as_rank < 0 || as_rank >= as_world)) {
        ec3d_set_error("ec3d_multi_create_rank: a rehearsal (as_world > 0) runs in a one-rank job, 0 <= as_rank < as_world");
        return 2;
    }
    std::string why;
    const ec3d_rccl_api *api = ec3d_rccl_load(why);
    if (!api) {
        ec3d_set_error("ec3d_multi_create_rank: " + why);
        return 109;
    }
    ec3d_multi *m = new ec3d_multi();
    m->n = 1;
    m->nccl = api;
    m->comm_rank = rank;
    m->comm_world = nranks;
    m->rehearse = rehearse;
    m->world = rehearse ? as_world : nranks;
    m->slab.emplace_back(new Slab());
    m->slab.back()->rank = rehearse ? as_rank : rank;
    m->slab.back()->device = device;
    m->pool.rc.assign(1, 0);
    m->pool.th.emplace_back(worker, m, 0);
    ncclUniqueId ih, is;
    memcpy(&ih, id_halo, sizeof ih);
    memcpy(&is, id_sum, sizeof is);
    int rc = run_all(m, [&](int) -> int {
        Slab &s = *m->slab[0];
        int rc2 = slab_reset(m, s);
        if (rc2) return rc2;
        // two communicators: the halo planes travel on the side stream while the compute stream -- which carries the
        // all-gathers of the sums -- runs the interior launch; every rank issues the calls of each in the same order
        MNCCL(m, api->CommInitRank(&m->comm_halo, nranks, ih, rank));
        MNCCL(m, api->CommInitRank(&m->comm_sum, nranks, is, rank));
        MHIP(m->gsum.alloc((size_t)nranks * P_NSLOT));
        MHIP(hipMemset(m->gsum, 0, (size_t)nranks * P_NSLOT * sizeof(double)));
        MHIP(m->agbuf.alloc((size_t)(nranks + 1) * kFacts));
        return 0;
    });
    if (rc) {
        std::string keep = ec3d_last_error();
        ec3d_multi_destroy(m);
        ec3d_set_error(keep);
        return rc;
    }
    *mh = m;
    return 0;
}

extern "C" int ec3d_multi_destroy(ec3d_multi_handle m)
{
    if (!m) return 0;
    (void)run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        (void)hipSetDevice(s.device);
        (void)hipDeviceSynchronize();
        if (s.c) (void)ec3d_destroy(s.c);
        s.c = nullptr;
        s.release(); // its side stream, events and buffers
        if (m->nccl) {
            if (m->comm_halo) (void)m->nccl->CommDestroy(m->comm_halo);
            if (m->comm_sum) (void)m->nccl->CommDestroy(m->comm_sum);
            m->gsum.reset();
            m->agbuf.reset();
        }
        return 0;
    });
    {
        std::lock_guard<std::mutex> lk(m->pool.m);
        m->pool.quit = true;
        m->pool.cv.notify_all();
    }
    for (auto &t : m->pool.th) t.join();
    delete m;
    return 0;
}

extern "C" int ec3d_multi_ranks(ec3d_multi_handle m) { return m ? m->world : 0; }

extern "C" int ec3d_multi_slab(ec3d_multi_handle m, int32_t rank, ec3d_handle *h, int32_t *k0, int32_t *k1)
{
    if (!m || rank < 0 || rank >= m->n) return 2;
    Slab &s = *m->slab[(size_t)rank];
    if (h) *h = s.c;
    if (k0) *k0 = s.k0;
    if (k1) *k1 = s.k1;
    return 0;
}

extern "C" int ec3d_multi_set_format(ec3d_multi_handle m, int dictionary, int structured)
{
    if (!m) return 2;
    for (auto &s : m->slab) {
        if (dictionary >= 0) s->c->use_dict = dictionary != 0;
        if (structured >= 0) s->c->use_sav = structured != 0;
    }
    return 0;
}

// ---- the single-component operator of BASELINE configs 2 and 4 (ec3d_assemble_poisson) on z-slabs -------
extern "C" int ec3d_multi_assemble_poisson(ec3d_multi_handle m, int32_t sdx, int32_t sdy, int32_t sdz,
                                           const double *BND, const double *delta)
{
    if (!m) return 2;
    if (sdz < m->world) {
        ec3d_set_error("ec3d_multi_assemble_poisson: fewer z-planes than ranks");
        return 2;
    }
    const SlabKnobs knob;
    const int64_t nC = (int64_t)sdx * sdy * sdz;
    return setup_job(m, knob, 1, sdx, sdy, sdz, 0, nC, -1, [&](Slab &s) -> int {
        const int rc = m->world == 1 ? ec3d_assemble_poisson(s.c, sdx, sdy, sdz, BND, delta)
                                     : ec3d_assemble_poisson_slab(s.c, sdx, sdy, sdz, s.k0, s.k1, BND, delta);
        return rc ? rc : cube_slab_layout(m, s, (int64_t)(s.k1 - s.k0) * m->kdz);
    });
}

// ---- the full A-V system (ec3d_assemble, src/EC3D.f90:465-1049) on z-slabs: global tables in, the library
//      cuts the extended slabs (two halo planes per interior side) and renumbers the U unknowns per slab
extern "C" int ec3d_multi_assemble(ec3d_multi_handle m, int32_t sdx, int32_t sdy, int32_t sdz, const int8_t *geoPHYS,
                                   const int32_t *geoPHYS_C, const double *valPHYS, int32_t nsub_glob,
                                   const double *BND, const double *delta, double dt)
{
    if (!m) return 2;
    const int H = 2;
    if (m->world > 1 && sdz < H * m->world) {
        ec3d_set_error("ec3d_multi_assemble: every rank needs at least two z-planes");
        return 2;
    }
    m->kind = 0;
    const int64_t kdz = (int64_t)sdx * sdy, nC_glob = kdz * sdz;
    int64_t nU = 0;
    for (int64_t q = 0; q < nC_glob; ++q) nU += geoPHYS_C[q] != 0;
    const int64_t n_glob = 3 * nC_glob + nU;
    for (int64_t q = 0; q < nC_glob; ++q)
        if (geoPHYS_C[q] != 0 && (geoPHYS_C[q] <= 3 * nC_glob || geoPHYS_C[q] > n_glob)) {
            ec3d_set_error("ec3d_multi_assemble: geoPHYS_C holds a U column id outside 3*nCells+1 .. n");
            return 2;
        }
    const SlabKnobs knob;
    // (neighbours must agree on the storage -- a slab that fell back to bands + tail next to a structured one would
    // exchange differently shaped blocks: finish_setup compares; nnz: per-slab counts include inert halo rows, not summed)
    return setup_job(m, knob, 2, sdx, sdy, sdz, nU, n_glob, 0, [&](Slab &s) -> int {
        const int64_t np = s.e1 - s.e0, nC = np * kdz;
        const int8_t *geo = geoPHYS + (int64_t)s.e0 * kdz;
        const int32_t *gc = geoPHYS_C + (int64_t)s.e0 * kdz;
        std::vector<int32_t> gc_ext((size_t)nC, 0);
        std::vector<int64_t> upl((size_t)np + 1, 0); // conducting cells before held plane p
        int64_t mloc = 0;
        for (int64_t p = 0; p < np; ++p) {
            upl[(size_t)p] = mloc;
            for (int64_t q = p * kdz; q < (p + 1) * kdz; ++q)
                if (gc[q] != 0) {
                    gc_ext[(size_t)q] = (int32_t)(3 * nC + 1 + mloc++);
                    s.u_glob.push_back((int32_t)(gc[q] - 3 * nC_glob - 1));
                }
        }
        upl[(size_t)np] = mloc;
        const int rc = m->world == 1
                           ? ec3d_assemble(s.c, sdx, sdy, sdz, geo, gc_ext.data(), valPHYS, nsub_glob, BND, delta, dt)
                           : ec3d_assemble_slab(s.c, sdx, sdy, sdz, s.e0, s.e1, s.k0, s.k1, geo, gc_ext.data(), valPHYS,
                                                nsub_glob, BND, delta, dt);
        if (rc) return rc;
        av_slab_layout(m, s, knob, mloc, upl);
        return 0;
    });
}

// ---- a single-component 7-point operator that arrives as CSR (BASELINE configs 2 and 4 through the drop-in symbol):
//      seven bands at (-kdz, -sdx, -1, 0, 1, sdx, kdz) and nothing else, n a whole number of planes.  Every rank takes
//      the band rows of its planes (same coefficients, same order), the ghost zones carry the neighbours' planes -- the
//      layout of ec3d_multi_assemble_poisson.  Returns -1 when the matrix is not of that kind.
static int multi_set_cube_csr(ec3d_multi *m, int32_t n, const double *valA, const int32_t *irow, const int32_t *jcol)
{
    HostMatrix M;
    if (ec3d_csr_to_host_matrix(n, valA, irow, jcol, M) != 0) return -1;
    int64_t sdx = 0, kdz = 0;
    if (!ec3d_host_matrix_is_cube(M, sdx, kdz)) return -1;
    const int64_t sdz = (int64_t)n / kdz;
    if (sdz < m->world) {
        ec3d_set_error("ec3d_multi_set_matrix_csr: fewer z-planes than ranks");
        return 2;
    }
    const SlabKnobs knob;
    return setup_job(m, knob, 1, sdx, kdz / sdx, sdz, 0, n, M.nnz, [&](Slab &s) -> int {
        const int64_t rows = (int64_t)(s.k1 - s.k0) * kdz, r0 = (int64_t)s.k0 * kdz;
        HostMatrix S;
        S.n = rows;
        S.n_pad = (rows + EC3D_TILE - 1) / EC3D_TILE * EC3D_TILE;
        S.nb = 7;
        for (int b = 0; b < 7; ++b) S.off[b] = M.off[b];
        S.bands.assign((size_t)7 * S.n_pad, 0.0);
        for (int b = 0; b < 7; ++b)
            memcpy(&S.bands[(size_t)b * S.n_pad], &M.bands[(size_t)b * M.n_pad + r0], (size_t)rows * sizeof(double));
        S.tail_id.assign((size_t)S.n_pad, -1);
        S.tile_flag.assign((size_t)(S.n_pad / EC3D_TILE), 0);
        S.chunk_ptr.assign(1, 0);
        S.nnz = 0;
        for (int64_t q = r0; q < r0 + rows; ++q) S.nnz += irow[q + 1] - irow[q];
        if (s.c->use_dict) ec3d_build_dictionary_host(S);
        const int rc = ec3d_upload_matrix(s.c, S, m->world > 1 ? kdz : 0);
        return rc ? rc : cube_slab_layout(m, s, rows);
    });
}

// ---- the reference's CSR triple (what sprsbcgstabwr_ receives): recognised as the A-V system on a grid
//      (ec3d_sav_csr.cpp), then cut into slabs of the structured form -----------------------------------------
extern "C" int ec3d_multi_set_matrix_csr(ec3d_multi_handle m, int32_t n, const double *valA, const int32_t *irow,
                                         const int32_t *jcol)
{
    if (!m) return 2;
    m->kind = 0;
    SavHost G;
    if (ec3d_csr_to_sav_host(n, valA, irow, jcol, G) != 0) {
        const int rc1 = multi_set_cube_csr(m, n, valA, irow, jcol); // a single-component 7-point operator?
        if (rc1 >= 0) return rc1;
        ec3d_set_error("ec3d_multi_set_matrix_csr: the matrix is not recognised as the reference's A-V system on a "
                       "grid (ec3d_probe_csr) nor as a single-component 7-point operator on one, so there are no "
                       "z-planes to cut it along; use one GPU");
        return 7;
    }
    const int64_t sdz = G.nCd / G.pitch;
    {
        std::string why;
        const int rc0 = ec3d_sav_cuttable(G, m->world, why);
        if (rc0) { // e.g. a cube whose plane count is a multiple of 3, read as three blocks of planes / 3 (too few planes
                   // per rank for that reading, or coupled across the blocks' faces): as ec3d_probe_csr_multi, any
                   // refusal of the A-V reading is followed by the single-component one
            const int rc1 = multi_set_cube_csr(m, n, valA, irow, jcol);
            if (rc1 >= 0) return rc1;
        }
        if (rc0) {
            ec3d_set_error("ec3d_multi_set_matrix_csr: " + why);
            return rc0;
        }
    }
    const SlabKnobs knob;
    return setup_job(m, knob, 2, G.sdx, G.plane / G.sdx, sdz, (int64_t)G.cond_cell.size(), n, G.nnz, [&](Slab &s) -> int {
        int rc = 0;
        const int64_t np = s.e1 - s.e0;
        if (m->world == 1) {
            if ((rc = ec3d_upload_sav(s.c, G))) return rc;
        } else {
            SavHost L;
            ec3d_sav_slice(G, s.e0, s.e1, s.k0, s.k1, L);
            if ((rc = ec3d_upload_sav(s.c, L))) return rc;
        }
        // held conducting cells: one contiguous run of the global scan-order list
        std::vector<int64_t> upl((size_t)np + 1, 0);
        int64_t first = -1, cnt = 0;
        for (size_t q = 0; q < G.cond_cell.size(); ++q) {
            const int64_t pl = G.cond_cell[q] / G.pitch;
            if (pl < s.e0 || pl >= s.e1) continue;
            if (first < 0) first = (int64_t)q;
            ++cnt;
            ++upl[(size_t)(pl - s.e0) + 1];
        }
        for (int64_t p = 0; p < np; ++p) upl[(size_t)p + 1] += upl[(size_t)p];
        s.u_glob.resize((size_t)cnt);
        for (int64_t q = 0; q < cnt; ++q) s.u_glob[(size_t)q] = (int32_t)(first + q);
        av_slab_layout(m, s, knob, cnt, upl);
        return 0;
    });
}

extern "C" int ec3d_multi_upload(ec3d_multi_handle m, int which, const double *host)
{
    int rc = need(m, "ec3d_multi_upload");
    if (rc) return rc;
    if (which < 0 || which >= EC3D_NVEC) return 2;
    return run_all(m, [&](int r) { return slab_upload(m, *m->slab[(size_t)r], which, host); });
}

extern "C" int ec3d_multi_download(ec3d_multi_handle m, int which, double *host)
{
    int rc = need(m, "ec3d_multi_download");
    if (rc) return rc;
    if (which < 0 || which >= EC3D_NVEC) return 2;
    return run_all(m, [&](int r) { return slab_download(m, *m->slab[(size_t)r], which, host); });
}

extern "C" int ec3d_multi_size(ec3d_multi_handle m, int64_t *n)
{
    int rc = need(m, "ec3d_multi_size");
    if (rc) return rc;
    *n = m->n_glob;
    return 0;
}

extern "C" int ec3d_multi_solve_resident(ec3d_multi_handle m, double tolerance, int32_t itmax, int32_t *iter)
{
    int rc = need(m, "ec3d_multi_solve_resident");
    if (rc) return rc;
    std::vector<int32_t> its((size_t)m->n, -1);
    std::vector<int> hit((size_t)m->n, 0);
    rc = run_all(m, [&](int r) {
        return slab_solve(m, *m->slab[(size_t)r], tolerance, itmax, &its[(size_t)r], &hit[(size_t)r]);
    }, true);
    if (rc) return rc;
    for (int r = 1; r < m->n; ++r)
        if (its[(size_t)r] != its[0]) {
            ec3d_set_error("ec3d_multi_solve: ranks disagree on the iteration count (" + std::to_string(its[0]) + " vs " +
                           std::to_string(its[(size_t)r]) + ")");
            return 106;
        }
    *iter = its[0];
    if (hit[0]) {
        // itmax exit: the reference prints norm2(R) and returns (src/solvers.f90:25-28); ||R||^2 = the ranks'
        // last R.R sums added in rank order
        double s = 0.0;
        if (m->nccl) { // one process per GPU: every rank's last sums are in the gathered copy
            std::vector<double> all((size_t)m->comm_world * P_NSLOT);
            (void)hipSetDevice(m->slab[0]->device);
            EC3D_HIP(hipMemcpy(all.data(), m->gsum, all.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int g = 0; g < m->comm_world; ++g) s += all[(size_t)g * P_NSLOT + P_RR];
        }
        for (auto &sl : m->slab) {
            if (m->nccl) break;
            double v = 0.0;
            (void)hipSetDevice(sl->device);
            EC3D_HIP(hipMemcpy(&v, sl->lsum + P_RR, sizeof v, hipMemcpyDeviceToHost));
            s += v;
        }
        if (ec3d_itmax_print_hold) {
            *ec3d_itmax_print_hold = std::sqrt(s);
        } else if (!m->nccl || m->comm_rank == 0) { // one process per GPU: the line appears once, as the reference's does
            ec3d_print_rnorm(std::sqrt(s));
            fflush(stdout);
        }
    }
    return 0;
}

extern "C" int ec3d_multi_solve(ec3d_multi_handle m, const double *b, double *x, double tolerance, int32_t itmax,
                                int32_t *iter)
{
    int rc = need(m, "ec3d_multi_solve");
    if (rc) return rc;
    if ((rc = run_all(m, [&](int r) -> int {
             Slab &s = *m->slab[(size_t)r];
             int rc2 = slab_upload(m, s, EC3D_VEC_B, b);
             return rc2 ? rc2 : slab_upload(m, s, EC3D_VEC_X, x);
         })))
        return rc;
    if ((rc = ec3d_multi_solve_resident(m, tolerance, itmax, iter))) return rc;
    return run_all(m, [&](int r) { return slab_download(m, *m->slab[(size_t)r], EC3D_VEC_X, x); });
}

// ---- the time loop around the solve on slabs (src/EC3D.f90:275-404, :412-433; SlabSolver.rhs_step) ------
extern "C" int ec3d_multi_rhs_step(ec3d_multi_handle m, int32_t moving, int32_t nsrc, const int32_t *src_index,
                                   const double *src_value)
{
    int rc = need(m, "ec3d_multi_rhs_step");
    if (rc) return rc;
    if (m->kind != 2) {
        ec3d_set_error("ec3d_multi_rhs_step: needs a matrix from ec3d_multi_assemble");
        return 3;
    }
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        // the U-row right-hand sides read A one plane away: refresh the X halo first
        int rc2 = halo_start(m, s, CH_X);
        if (rc2) return rc2;
        if ((rc2 = halo_wait(s, CH_X))) return rc2;
        // sources outside the held planes are dropped, the rest renumbered locally (1-based ids)
        std::vector<int32_t> idx;
        std::vector<double> val;
        for (int32_t q = 0; q < nsrc; ++q) {
            const int64_t g0 = (int64_t)src_index[q] - 1, d = g0 / m->nC_glob, cell = g0 % m->nC_glob;
            const int64_t plane = cell / m->kdz;
            if (d > 2 || plane < s.e0 || plane >= s.e1) continue;
            idx.push_back((int32_t)(d * s.nC_ext + (cell - (int64_t)s.e0 * m->kdz) + 1));
            val.push_back(src_value[q]);
        }
        int32_t dummy_i = 0;
        double dummy_v = 0.0;
        if ((rc2 = ec3d_rhs_step(s.c, moving, (int32_t)idx.size(), idx.empty() ? &dummy_i : idx.data(),
                                 val.empty() ? &dummy_v : val.data())))
            return rc2;
        return drain(s);
    }, true);
}

extern "C" int ec3d_multi_post_update(ec3d_multi_handle m)
{
    int rc = need(m, "ec3d_multi_post_update");
    if (rc) return rc;
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = ec3d_post_update(s.c);
        return rc2 ? rc2 : drain(s);
    });
}

extern "C" int ec3d_multi_vtk_fields(ec3d_multi_handle m, const double *delta, float *field_A, float *field_eddy,
                                     float *field_source, float *field_B)
{
    int rc = need(m, "ec3d_multi_vtk_fields");
    if (rc) return rc;
    if (m->kind != 2) {
        ec3d_set_error("ec3d_multi_vtk_fields: needs a matrix from ec3d_multi_assemble");
        return 3;
    }
    if (field_eddy) memset(field_eddy, 0, (size_t)3 * m->nC_glob * sizeof(float)); // slabs without conductor skip it
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = halo_start(m, s, CH_X); // the curl reads the neighbours' planes
        if (rc2) return rc2;
        if ((rc2 = halo_wait(s, CH_X))) return rc2;
        const size_t off = (size_t)3 * s.k0 * m->kdz;
        if ((rc2 = ec3d_vtk_fields(s.c, delta, field_A + off, field_eddy ? field_eddy + off : nullptr, field_source + off,
                                   field_B + off)))
            return rc2;
        return drain(s);
    }, true);
}

// Field output overlapped with the next time step, over the slabs (ec3d_vtk_fields_begin / _wait on every slab's own
// handle: its field kernel behind its post-update, its copy into its own pinned buffers on its own side stream).  The
// slabs take their slots in step, so one slot number names the same output step on all of them; _wait hands out ONE
// slab's part -- cells k0*sdx*sdy .. k1*sdx*sdy of every vector, which are consecutive in field_N.vtk
// (src/utilites.f90:222-289 writes cell by cell, z outermost).
extern "C" int ec3d_multi_vtk_fields_begin(ec3d_multi_handle m, const double *delta, int32_t big_endian, int32_t *slot)
{
    int rc = need(m, "ec3d_multi_vtk_fields_begin");
    if (rc) return rc;
    if (m->kind != 2 || !slot) {
        ec3d_set_error("ec3d_multi_vtk_fields_begin: needs a matrix from ec3d_multi_assemble and a slot to return");
        return m->kind != 2 ? 3 : 2;
    }
    std::vector<int32_t> got((size_t)m->n, -1);
    rc = run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = halo_start(m, s, CH_X); // the curl reads the neighbours' planes
        if (rc2) return rc2;
        if ((rc2 = halo_wait(s, CH_X))) return rc2;
        return ec3d_vtk_fields_begin(s.c, delta, big_endian, &got[(size_t)r]); // enqueued only: nothing waits here
    }, true);
    if (rc) return rc;
    for (int r = 1; r < m->n; ++r)
        if (got[(size_t)r] != got[0]) {
            ec3d_set_error("ec3d_multi_vtk_fields_begin: the slabs' output slots are out of step");
            return 4;
        }
    *slot = got[0];
    return 0;
}

extern "C" int ec3d_multi_vtk_fields_wait(ec3d_multi_handle m, int32_t slot, int32_t rank, const float **field_A,
                                          const float **field_eddy, const float **field_source, const float **field_B,
                                          int64_t *cell0, int64_t *ncells)
{
    int rc = need(m, "ec3d_multi_vtk_fields_wait");
    if (rc) return rc;
    if (rank < 0 || rank >= m->n) {
        ec3d_set_error("ec3d_multi_vtk_fields_wait: no such slab");
        return 2;
    }
    Slab &s = *m->slab[(size_t)rank];
    if (cell0) *cell0 = (int64_t)s.k0 * m->kdz;
    return ec3d_vtk_fields_wait(s.c, slot, field_A, field_eddy, field_source, field_B, ncells);
}

// ---- bench "steps": exits disabled, launches only ---------------------------------------------------------
extern "C" int ec3d_multi_iterate_begin(ec3d_multi_handle m)
{
    int rc = need(m, "ec3d_multi_iterate_begin");
    if (rc) return rc;
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = run_plan(m, s, begin_plan(s.plan), 0, -1.0, nullptr);
        return rc2 ? rc2 : drain(s);
    }, true);
}

namespace {
// kernel_ms[5]: stage averages of local slab `timed_rank`; sync_ms[2] / sync_n[2]: per iteration, the time the compute stream of
// that slab stood at the reduction points / at the waits for halo planes, and how many of each an iteration has
int multi_iterate(ec3d_multi *m, int32_t first_iter, int32_t count, int timed_rank, double *kernel_ms, double *sync_ms,
                  int32_t *sync_n)
{
    int rc = need(m, "ec3d_multi_iterate");
    if (rc) return rc;
    // as ec3d_iterate; slab 0's cursor speaks for the job (the other slabs' threads keep theirs in step with it)
    for (size_t r = 0; r < m->slab.size(); ++r)
        if ((rc = ec3d_run_open(m->slab[r]->c, first_iter, (int64_t)first_iter + count - 1, r == 0 ? "ec3d_multi_iterate" : nullptr)))
            return rc;
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        StageTimer tm;
        tm.sync_points = sync_ms != nullptr;
        StageTimer *tp = (kernel_ms && r == timed_rank) ? &tm : nullptr;
        int rc2 = 0;
        const uint64_t calls0 = t_api_calls;
        for (int it = first_iter; it < first_iter + count; ++it)
            if ((rc2 = run_plan(m, s, iter_plan(s.plan), it, 0.0, tp))) return rc2;
        s.api_calls = t_api_calls - calls0;
        s.api_iters = (uint64_t)std::max(0, count);
        if (!kernel_ms) return 0; // asynchronous: ec3d_multi_synchronize() joins
        if ((rc2 = drain(s))) return rc2;
        if (tp) {
            for (int k = 0; k < 5; ++k) kernel_ms[k] = 0.0;
            if (sync_ms) sync_ms[0] = sync_ms[1] = 0.0;
            if (sync_n) sync_n[0] = sync_n[1] = 0;
            for (size_t i = 0; i < tm.kern.size(); ++i) {
                float ms = 0.f;
                MHIP(hipEventElapsedTime(&ms, tm.ev[2 * i], tm.ev[2 * i + 1]));
                const int k = tm.kern[i];
                if (k < 5) {
                    kernel_ms[k] += (double)ms / std::max(1, count);
                } else if (sync_ms) {
                    sync_ms[k - T_GATHER] += (double)ms / std::max(1, count);
                    if (sync_n) ++sync_n[k - T_GATHER];
                }
            }
            if (sync_n)
                for (int q = 0; q < 2; ++q) sync_n[q] /= std::max(1, count);
        }
        return 0;
    }, true);
}
} // namespace

extern "C" int ec3d_multi_iterate(ec3d_multi_handle m, int32_t first_iter, int32_t count, double *kernel_ms)
{
    return multi_iterate(m, first_iter, count, 0, kernel_ms, nullptr, nullptr);
}

extern "C" int ec3d_multi_iterate_timed(ec3d_multi_handle m, int32_t first_iter, int32_t count, int32_t rank, double *kernel_ms,
                                        double *sync_ms, int32_t *sync_n)
{
    if (!m || rank < 0 || rank >= m->n || !kernel_ms || !sync_ms || !sync_n) return 2;
    return multi_iterate(m, first_iter, count, rank, kernel_ms, sync_ms, sync_n);
}

// which RCCL this one-process-per-GPU handle talks through, and what IT says the job is: ranks of the communicator
// (ncclCommCount on the communicator the sums travel on), library version (ncclGetVersion), file the entry points came from
extern "C" int ec3d_multi_rccl_info(ec3d_multi_handle m, int32_t *nranks, int32_t *version, char *path, int32_t path_cap)
{
    if (!m || !m->nccl) {
        ec3d_set_error("ec3d_multi_rccl_info: not a one-process-per-GPU handle (ec3d_multi_create_rank)");
        return 3;
    }
    int n = -1, v = 0;
    if (m->nccl->CommCount && m->comm_sum) MNCCL(m, m->nccl->CommCount(m->comm_sum, &n));
    if (m->nccl->GetVersion) MNCCL(m, m->nccl->GetVersion(&v));
    if (nranks) *nranks = n;
    if (version) *version = v;
    if (path && path_cap > 0) {
        strncpy(path, m->nccl->path, (size_t)path_cap - 1);
        path[path_cap - 1] = 0;
    }
    return 0;
}

// HIP runtime calls (launches, event records / waits, copies) rank `rank`'s thread issued per iteration in the last
// ec3d_multi_iterate: the host-side price of an iteration, which has to stay below its device time
extern "C" int ec3d_multi_api_calls(ec3d_multi_handle m, int32_t rank, double *per_iteration)
{
    if (!m || rank < 0 || rank >= m->n || !per_iteration) return 2;
    const Slab &s = *m->slab[(size_t)rank];
    *per_iteration = s.api_iters ? (double)s.api_calls / (double)s.api_iters : 0.0;
    return 0;
}

extern "C" int ec3d_multi_plan(ec3d_multi_handle m, int32_t *plan, int32_t *x_every)
{
    int rc = need(m, "ec3d_multi_plan");
    if (rc) return rc;
    const Slab &s = *m->slab[0];
    if (plan) *plan = s.plan;
    if (x_every) *x_every = ec3d_xdefer(s.c);
    return 0;
}

extern "C" int ec3d_multi_halo_rows(ec3d_multi_handle m, int32_t rank, int64_t *sent, int64_t *received)
{
    int rc = need(m, "ec3d_multi_halo_rows");
    if (rc) return rc;
    if (rank < 0 || rank >= m->n) return 2;
    const Slab &s = *m->slab[(size_t)rank];
    if (sent) *sent = rows_of(s.halo.send_lo) + rows_of(s.halo.send_hi);
    if (received) *received = rows_of(s.halo.recv_lo) + rows_of(s.halo.recv_hi);
    return 0;
}

extern "C" int ec3d_multi_synchronize(ec3d_multi_handle m)
{
    if (!m) return 2;
    // watched: this is where the asynchronous ec3d_multi_iterate (bench.py's timed region) is joined -- every rank sits
    // in hipStreamSynchronize behind cross-slab event waits, the very stall the watchdog exists for
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        if (!s.c) return 0;
        MHIP(hipSetDevice(s.device));
        return drain(s);
    }, true);
}

// ||B - A X|| / ||B|| over all slabs (as ec3d_true_residual): X halo refreshed, the residual stage on every
// slab, the ranks' two sums added on the host in rank order.
extern "C" int ec3d_multi_true_residual(ec3d_multi_handle m, double *rel, double *bnorm)
{
    int rc = need(m, "ec3d_multi_true_residual");
    if (rc) return rc;
    std::vector<double> bb((size_t)std::max(m->world, m->comm_world), 0.0), rr((size_t)std::max(m->world, m->comm_world), 0.0);
    rc = run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = halo_start(m, s, CH_X);
        if (rc2) return rc2;
        if ((rc2 = halo_wait(s, CH_X))) return rc2;
        if ((rc2 = ec3d_dist_step(s.c, EC3D_STAGE_RESID, 0, 0.0))) return rc2;
        if (m->nccl && (rc2 = gather(m, s))) return rc2;
        if ((rc2 = drain(s))) return rc2;
        if (m->nccl) { // every rank's two sums, rank order
            std::vector<double> all((size_t)m->comm_world * P_NSLOT);
            MHIP(hipMemcpy(all.data(), m->gsum, all.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int g = 0; g < m->comm_world; ++g) {
                bb[(size_t)g] = all[(size_t)g * P_NSLOT + P_BB];
                rr[(size_t)g] = all[(size_t)g * P_NSLOT + P_RR_INIT];
            }
            return 0;
        }
        double v[P_NSLOT];
        MHIP(hipMemcpy(v, s.lsum, sizeof v, hipMemcpyDeviceToHost));
        bb[(size_t)r] = v[P_BB];
        rr[(size_t)r] = v[P_RR_INIT];
        return 0;
    }, true);
    if (rc) return rc;
    double sb = 0.0, sr = 0.0;
    for (size_t r = 0; r < bb.size(); ++r) {
        sb += bb[r];
        sr += rr[r];
    }
    if (bnorm) *bnorm = std::sqrt(sb);
    *rel = sb > 0.0 ? std::sqrt(sr / sb) : std::sqrt(sr);
    return 0;
}

// y = A*x over the slabs (src/solvers.f90:54-61), host vectors in the global numbering: x goes to every slab's P,
// the rows the halo exchange fills are set to NaN, the P halo planes are exchanged the way an iteration does it,
// every slab multiplies, the owned parts of AP come back.  Parity probe of the slab operators AND of the exchange:
// a result equal to the undivided operator's means every halo row arrived, in time, from the right place.
extern "C" int ec3d_multi_spmv(ec3d_multi_handle m, const double *x, double *y)
{
    int rc = need(m, "ec3d_multi_spmv");
    if (rc) return rc;
    return run_all(m, [&](int r) -> int {
        Slab &s = *m->slab[(size_t)r];
        int rc2 = slab_upload(m, s, EC3D_VEC_P, x);
        if (rc2) return rc2;
        // the probe must depend on the transport: what the exchange is to deliver is NaN until it does
        if (m->world > 1 && (rc2 = poison_recv_rows(s, EC3D_VEC_P))) return rc2;
        if ((rc2 = halo_start(m, s, CH_P))) return rc2;
        if ((rc2 = halo_wait(s, CH_P))) return rc2;
        ec3d_launch_spmv(s.c->A.view(), s.c->sweep_s, s.c->vec[EC3D_VEC_P], s.c->vec[EC3D_VEC_AP], s.c->stream);
        MHIP(hipGetLastError());
        if ((rc2 = drain(s))) return rc2;
        return slab_download(m, s, EC3D_VEC_AP, y);
    }, true);
}
