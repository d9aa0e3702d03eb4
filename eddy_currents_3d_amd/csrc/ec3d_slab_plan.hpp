// ec3d_slab_plan.hpp — everything a z-slab job (ec3d_multi.hip) decides without a device (host only: no HIP call, no kernel,
// no handle, no thread): the op tables every rank's thread walks and the stage it launches for each entry; which planes a
// rank owns and holds; the runs of halo rows a slab sends and receives, how two neighbours' runs pair into copies or
// send / receive pieces, and the checks that refuse a job whose neighbours disagree (over RCCL a disagreement is a hang,
// not an error); the environment knobs; what the whole job can do, from the facts every rank contributes, and what that
// makes of each slab.  ec3d_multi.hip keeps the threads, streams, events, RCCL calls and the calls that need a handle.
// tests/test_slab_plan_host.py checks all of it on the CPU, and pins the tables of plans 0 .. 2 to those of
// eddy_currents_3d_amd/dist.py.
#pragma once
#include "../../include/ec3d_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <string>
#include <vector>

namespace ec3d_slab {
enum { CH_P = 0, CH_S = 1, CH_X = 2, CH_AP = 3, CH_R = 4, NHALO = 5, CH_SUM = 5, CH_HUB = 6, NCH = 7 };
inline const int kVecOf[NHALO] = {EC3D_VEC_P, EC3D_VEC_S, EC3D_VEC_X, EC3D_VEC_AP, EC3D_VEC_R};

// a run of halo planes inside one work vector: `planes` pieces of `payload` doubles, `pitch` apart
struct Run {
    int64_t start = 0, pitch = 0, payload = 0;
    int planes = 0;
    int64_t lo() const { return start; }
    int64_t hi() const { return start + (int64_t)(planes - 1) * pitch + std::max(payload, planes > 1 ? pitch : payload); }
};
struct Copy {
    int64_t dst, src, cnt;
};
struct Piece {
    int64_t off, cnt;
};
// towards rank-1 / rank+1, same order on both sides
struct HaloRuns {
    std::vector<Run> send_lo, recv_lo, send_hi, recv_hi;
};

// ---- plans -----------------------------------------------------------------------------------------------------------------
enum { OP_HALO = 0, OP_HALO_START, OP_HALO_WAIT, OP_GATHER, OP_STEP, OP_SKIP_IF_AP };
struct Op {
    int kind, arg;
    int dit = 0; // halo ops: the exchanged vector is that of iteration it + dit (P after K5 is the NEXT iteration's)
};
#define ST(x) Op{OP_STEP, EC3D_STAGE_##x}
inline const std::vector<Op> kBegin = {{OP_HALO, CH_X}, ST(RESID), {OP_GATHER, 0}, ST(SETUP)};
// (run with it = 0: the first iteration's P)
inline const std::vector<Op> kBeginVsplit = {{OP_HALO, CH_X}, ST(RESID), {OP_GATHER, 0}, ST(SETUP), {OP_HALO, CH_P, 1}};
// three reduction points per iteration (K3 is launched before ||S|| is known)
inline const std::vector<Op> kIter = {{OP_HALO, CH_P}, ST(K1), {OP_GATHER, 0}, ST(K2), {OP_HALO, CH_S},
                                      ST(K3), {OP_GATHER, 0}, ST(K4), {OP_GATHER, 0}, ST(K5)};
// exchange hidden behind the interior planes of K1/K3 (single-component slabs on a z-marching grid)
inline const std::vector<Op> kIterOverlap = {{OP_HALO_START, CH_P}, ST(K1_INT), {OP_HALO_WAIT, CH_P}, ST(K1_BND), {OP_GATHER, 0},
                                             ST(K2), {OP_HALO_START, CH_S}, ST(K3_INT), {OP_HALO_WAIT, CH_S}, ST(K3_BND),
                                             {OP_GATHER, 0}, ST(K4), {OP_GATHER, 0}, ST(K5)};
// the same from the producers' side (A-V slabs, any storage): K2/K5 boundary tiles first
inline const std::vector<Op> kIterVsplit = {{OP_HALO_WAIT, CH_P}, ST(K1), {OP_GATHER, 0}, ST(K2_BND), {OP_HALO_START, CH_S},
                                            ST(K2_INT), {OP_HALO_WAIT, CH_S}, ST(K3), {OP_GATHER, 0}, ST(K4), {OP_GATHER, 0},
                                            ST(K5_BND), {OP_HALO_START, CH_P, 1}, ST(K5_INT)};
// both at once (plan 5, single-component slabs): the producers K2 / K5 run the boundary planes first and start the
// exchange, the consumers K1 / K3 run their interior planes before they wait for it -- the planes have the producer's
// interior launch AND the consumer's to arrive behind, instead of one of the two.  Same exchanges in the same order as
// kIterVsplit (the first P travels from the begin plan on).
inline const std::vector<Op> kBeginBoth = {{OP_HALO, CH_X}, ST(RESID), {OP_GATHER, 0}, ST(SETUP), {OP_HALO_START, CH_P, 1}};
inline const std::vector<Op> kIterBoth = {ST(K1_INT), {OP_HALO_WAIT, CH_P}, ST(K1_BND), {OP_GATHER, 0}, ST(K2_BND),
                                          {OP_HALO_START, CH_S}, ST(K2_INT), ST(K3_INT), {OP_HALO_WAIT, CH_S}, ST(K3_BND),
                                          {OP_GATHER, 0}, ST(K4), {OP_GATHER, 0}, ST(K5_BND), {OP_HALO_START, CH_P, 1}, ST(K5_INT)};
// The three-launch iteration on slabs of the single-component operator (every rank >= 32 Mi rows; ec3d_ctx::slab_fused):
// K2 inside K3, K4 as an SpMV kernel, K5 inside the next iteration's K1.  S and P are formed on the halo planes by the
// kernels that read them there (and stored into the ghost rows: Sweep::halo_store), so what travels is AP -- after
// K5-in-K1, for the S = R - alpha*AP of K2-in-K3 and the next P on the halo planes -- and R -- after K4 --: two exchanges
// and three reduction points per iteration, as before.  P and R are exchanged once before the first iteration; the lone K1
// (with its reduction point and the exchange of its AP) runs when AP = A P of the iteration does not exist yet.
inline const std::vector<Op> kBeginFused = {{OP_HALO, CH_X}, ST(RESID), {OP_GATHER, 0}, ST(SETUP), {OP_HALO, CH_P, 1}, {OP_HALO, CH_R}};
inline const std::vector<Op> kIterFused = {{OP_SKIP_IF_AP, 3}, ST(K1), {OP_GATHER, 0}, {OP_HALO, CH_AP}, ST(K3), {OP_GATHER, 0}, ST(K4),
                                           {OP_GATHER, 0}, {OP_HALO, CH_R}, ST(K5), {OP_GATHER, 0}, {OP_HALO, CH_AP, 1}};
// the same with the two exchanges hidden: the PRODUCERS of R and AP run planes 0 and np-1 first, the exchange starts, the
// interior planes follow while the planes travel; the consumer's side waits in front of the launch that reads the halo.
// Exchanges and reduction points come in the same order as in kIterFused, so ranks may mix the two.
inline const std::vector<Op> kIterFusedOverlap = {{OP_SKIP_IF_AP, 3}, ST(K1), {OP_GATHER, 0}, {OP_HALO, CH_AP}, {OP_HALO_WAIT, CH_AP},
                                                  ST(K3), {OP_GATHER, 0}, ST(K4F_BND), {OP_HALO_START, CH_R}, ST(K4F_INT), {OP_GATHER, 0},
                                                  {OP_HALO_WAIT, CH_R}, ST(K5F_BND), {OP_HALO_START, CH_AP, 1}, ST(K5F_INT),
                                                  {OP_GATHER, 0}};
#undef ST

// plan: 0 plain, 1 overlap (K1/K3 interior + boundary), 2 vsplit (K2/K5 boundary first), 3 three launches (kIterFused), 4 three
// launches with the producers of R and AP split around the exchange, 5 = 1 and 2 together (kIterBoth)
inline const std::vector<Op> &begin_plan(int plan)
{
    return plan == 5 ? kBeginBoth : plan >= 3 ? kBeginFused : plan == 2 ? kBeginVsplit : kBegin;
}
inline const std::vector<Op> &iter_plan(int plan)
{
    return plan == 5 ? kIterBoth : plan == 4 ? kIterFusedOverlap : plan == 3 ? kIterFused : plan == 2 ? kIterVsplit
           : plan == 1 ? kIterOverlap : kIter;
}

// a slab too thin for interior + boundary launches of K1 / K3 inside plan 5: the whole kernel where the boundary launch stands
inline int unsplit_spmv_stage(int st)
{
    switch (st) {
    case EC3D_STAGE_K1_BND: return EC3D_STAGE_K1;
    case EC3D_STAGE_K3_BND: return EC3D_STAGE_K3;
    case EC3D_STAGE_K1_INT:
    case EC3D_STAGE_K3_INT: return -1;
    default: return st;
    }
}

inline int unsplit_stage(int st)
{
    switch (st) {
    case EC3D_STAGE_K2_BND: return EC3D_STAGE_K2;
    case EC3D_STAGE_K5_BND: return EC3D_STAGE_K5;
    case EC3D_STAGE_K2_INT:
    case EC3D_STAGE_K5_INT: return -1;
    default: return st;
    }
}

// the stage a slab launches where its plan's table says `st` (-1: nothing): split_ok, K2 / K5 can run as boundary + interior
// launch on this slab; overlap_ok, K1 / K3 as interior + boundary launch
inline int launched_stage(int plan, bool split_ok, bool overlap_ok, int st)
{
    if ((plan == 2 || plan == 5) && !split_ok) st = unsplit_stage(st);
    if (plan == 5 && !overlap_ok) st = unsplit_spmv_stage(st);
    return st;
}

// kernel (0..4 = K1..K5) a stage's time is booked under; -1: none
inline int kernel_of_stage(int st)
{
    switch (st) {
    case EC3D_STAGE_K1: case EC3D_STAGE_K1_INT: case EC3D_STAGE_K1_BND: return 0;
    case EC3D_STAGE_K2: case EC3D_STAGE_K2_INT: case EC3D_STAGE_K2_BND: return 1;
    case EC3D_STAGE_K3: case EC3D_STAGE_K3_INT: case EC3D_STAGE_K3_BND: return 2;
    case EC3D_STAGE_K4: case EC3D_STAGE_K4F_BND: case EC3D_STAGE_K4F_INT: return 3;
    case EC3D_STAGE_K5: case EC3D_STAGE_K5_INT: case EC3D_STAGE_K5_BND: case EC3D_STAGE_K5F_BND: case EC3D_STAGE_K5F_INT: return 4;
    default: return -1;
    }
}

// ---- slab geometry ---------------------------------------------------------------------------------------------------------
// owned planes [k0, k1) of rank `rank`: as even as possible, lower ranks take the remainder
inline void slab_bounds(int sdz, int rank, int world, int32_t &k0, int32_t &k1)
{
    const int base = sdz / world, rem = sdz % world;
    k0 = rank * base + std::min(rank, rem);
    k1 = k0 + base + (rank < rem ? 1 : 0);
}
// held planes [e0, e1): the owned ones and H halo planes per interior side (single-component slabs keep theirs in the
// ghost zones of the work vectors: H = 0)
inline void held_range(int sdz, int32_t k0, int32_t k1, int H, int32_t &e0, int32_t &e1)
{
    e0 = std::max(0, k0 - H);
    e1 = std::min((int32_t)sdz, k1 + H);
}

// ---- halo runs -------------------------------------------------------------------------------------------------------------
// A slab of `rows` rows of the single-component operator: one plane of kdz rows each way, the received ones in the ghost
// zones in front of row 0 and behind row `rows` -- which must hold a plane (`ghost` rows each).
inline int cube_runs(int rank, int world, int64_t kdz, int64_t rows, int64_t ghost, HaloRuns &out, std::string &err)
{
    out = HaloRuns{};
    if (ghost < kdz && world > 1) {
        err = "ec3d_multi: ghost zone smaller than a plane";
        return 105;
    }
    if (rank > 0) {
        out.send_lo.push_back(Run{0, kdz, kdz, 1});
        out.recv_lo.push_back(Run{-kdz, kdz, kdz, 1});
    }
    if (rank + 1 < world) {
        out.send_hi.push_back(Run{rows - kdz, kdz, kdz, 1});
        out.recv_hi.push_back(Run{rows, kdz, kdz, 1});
    }
    return 0;
}

// An A-V slab whose matrix is in place: local reference order [Ax_ext | Ay_ext | Az_ext | U_ext] of nC_ext cells per A block
// and nU_ext held U unknowns.  structured: the device holds four grid-shaped blocks of nCd rows, planes `pitch` apart; else
// (bands + tail) the reference order itself.
struct AvSlab {
    bool structured;
    int64_t nCd, pitch, kdz, nC_ext, nU_ext;
    int32_t k0, k1, e0, e1;
};
struct AvLayout {
    int64_t own_lo[4], own_hi[4]; // owned rows, local reference numbering
    HaloRuns runs;                // DEVICE rows
};
// upl[p] = held conducting cells before held plane p (np + 1 entries).  u_always: every U plane travels (the default;
// EC3D_AV_SEND_EMPTY_U=0 is the opt-in that leaves conductor-free ones at home).
inline AvLayout av_layout(const AvSlab &g, const std::vector<int64_t> &upl, bool u_always, bool rehearse)
{
    const int H = 2;
    AvLayout L{};
    HaloRuns &s = L.runs;
    const int64_t kdz = g.kdz, nC = g.nC_ext, mloc = g.nU_ext;
    const int64_t p0 = g.k0 - g.e0, p1 = g.k1 - g.e0;
    for (int d = 0; d < 3; ++d) {
        L.own_lo[d] = d * nC + p0 * kdz;
        L.own_hi[d] = d * nC + p1 * kdz;
    }
    L.own_lo[3] = 3 * nC + upl[(size_t)p0];
    L.own_hi[3] = 3 * nC + upl[(size_t)p1];
    // The 7-point stencil and the U rows read A one plane away; only the one-sided A-U stencils
    // (src/EC3D.f90:697-706) reach two planes, and they read U
    struct Blk { int64_t base, pitch, payload; int h; };
    std::vector<Blk> blocks;
    const bool structured = g.structured;
    if (structured) {
        for (int d = 0; d < 4; ++d) blocks.push_back(Blk{d * g.nCd, g.pitch, kdz, d < 3 ? 1 : H});
    } else {
        for (int d = 0; d < 3; ++d) blocks.push_back(Blk{d * nC, kdz, kdz, 1});
    }
    // Structured form: the U block is grid-shaped, but only cells of a conductor hold an unknown -- every other row of it
    // is inert and stays exactly zero in every vector.  Two planes of U that hold no conductor cell therefore need not
    // travel: the ghost rows they would fill are zero already (most cuts of a real model lie in air: BASELINE config 5 on
    // 8 ranks has the conductor at ONE of its seven cuts).  Both sides of a cut decide from the same planes' cell counts.
    // OPT-IN (EC3D_AV_SEND_EMPTY_U=0) until a job of two real devices has run once: by default every U plane travels.
    auto u_cells = [&](int64_t a, int64_t b) { return upl[(size_t)std::min<int64_t>(b, (int64_t)upl.size() - 1)] - upl[(size_t)std::max<int64_t>(a, 0)]; };
    // (a rehearsal sends to itself: what it sends towards a cut must pair with what it receives from there, so a side's U
    // planes travel when EITHER of the two pairs of planes around the cut holds a conductor cell)
    auto travels = [&](const Blk &b, int64_t first_plane, int64_t cut) {
        if (!structured || b.h != H || u_always) return true;
        return rehearse ? u_cells(cut - H, cut + H) > 0 : u_cells(first_plane, first_plane + H) > 0;
    };
    if (g.e0 < g.k0) {
        for (const Blk &b : blocks) {
            if (travels(b, p0, p0)) s.send_lo.push_back(Run{b.base + p0 * b.pitch, b.pitch, b.payload, b.h});
            if (travels(b, p0 - b.h, p0)) s.recv_lo.push_back(Run{b.base + (p0 - b.h) * b.pitch, b.pitch, b.payload, b.h});
        }
        if (!structured) { // compact U block: the U cells of my first two owned planes / my lower halo planes
            const int64_t ulo = upl[(size_t)p0], cnt_s = upl[(size_t)(p0 + H)] - ulo;
            s.send_lo.push_back(Run{3 * nC + ulo, cnt_s, cnt_s, 1});
            s.recv_lo.push_back(Run{3 * nC, ulo, ulo, 1});
        }
    }
    if (g.k1 < g.e1) {
        for (const Blk &b : blocks) {
            if (travels(b, p1 - b.h, p1)) s.send_hi.push_back(Run{b.base + (p1 - b.h) * b.pitch, b.pitch, b.payload, b.h});
            if (travels(b, p1, p1)) s.recv_hi.push_back(Run{b.base + p1 * b.pitch, b.pitch, b.payload, b.h});
        }
        if (!structured) {
            const int64_t uend = upl[(size_t)p1], cnt_s = uend - upl[(size_t)(p1 - H)], cnt_r = mloc - uend;
            s.send_hi.push_back(Run{3 * nC + uend - cnt_s, cnt_s, cnt_s, 1});
            s.recv_hi.push_back(Run{3 * nC + uend, cnt_r, cnt_r, 1});
        }
    }
    return L;
}

// rows a list of runs moves
inline int64_t rows_of(const std::vector<Run> &rs)
{
    int64_t t = 0;
    for (const Run &r : rs) t += r.payload * (int64_t)r.planes;
    return t;
}

// [lo, hi) of every run that moves something: the rows K2 / K5 of an A-V slab launch first (ec3d_dist_set_boundary_rows)
inline void boundary_rows(const HaloRuns &h, std::vector<int64_t> &lo, std::vector<int64_t> &hi)
{
    lo.clear();
    hi.clear();
    for (const std::vector<Run> *rs : {&h.send_lo, &h.recv_lo, &h.send_hi, &h.recv_hi})
        for (const Run &r : *rs)
            if (r.payload > 0) {
                lo.push_back(r.lo());
                hi.push_back(r.hi());
            }
}

// ---- pairing, pieces, digest -----------------------------------------------------------------------------------------------
// copy lists: my recv run i towards rank+1 <- rank+1's send run i towards me (and the mirror image)
inline int pair_up(const std::vector<Run> &recv, const std::vector<Run> &send, std::vector<Copy> &out, std::string &err)
{
    out.clear();
    if (recv.size() != send.size()) {
        err = "ec3d_multi: neighbouring slabs disagree on the halo layout";
        return 105;
    }
    for (size_t i = 0; i < recv.size(); ++i) {
        const Run &r = recv[i], &t = send[i];
        if (r.planes != t.planes || r.payload != t.payload) {
            err = "ec3d_multi: neighbouring slabs disagree on the halo size";
            return 105;
        }
        if (r.payload == 0) continue;
        if (r.pitch == t.pitch || r.planes == 1) { // one contiguous piece (plane padding included)
            const int64_t cnt = r.planes == 1 ? r.payload : (int64_t)r.planes * r.pitch;
            out.push_back(Copy{r.start, t.start, cnt});
        } else {
            for (int p = 0; p < r.planes; ++p) out.push_back(Copy{r.start + p * r.pitch, t.start + p * t.pitch, r.payload});
        }
    }
    return 0;
}

// one process per GPU: contiguous pieces of my own runs (the neighbour's matching lists come out of the same rules on
// the same grid and storage format, which the ranks compare: check_neighbours)
inline std::vector<Piece> pieces_of(const std::vector<Run> &runs)
{
    std::vector<Piece> out;
    for (const Run &r : runs) {
        if (r.payload == 0) continue;
        out.push_back(Piece{r.start, r.planes == 1 ? r.payload : (int64_t)r.planes * r.pitch});
    }
    return out;
}

// FNV-1a over (count, then every piece's length in order), folded to 52 bits: exact in a double
inline double digest(const std::vector<Piece> &ps)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { for (int b = 0; b < 8; ++b) { h ^= (v >> (8 * b)) & 0xFFu; h *= 1099511628211ull; } };
    mix((uint64_t)ps.size());
    for (const Piece &q : ps) mix((uint64_t)q.cnt);
    return (double)((h ^ (h >> 52)) & ((1ull << 52) - 1));
}

// What every rank has to know of every other: can it run the three-launch iteration, the depth of its rings, its
// storage format, its size, what it sends to its neighbours.  One process: read off the slabs; one process per GPU:
// kFacts doubles per rank, all-gathered once.
// (h_*: a digest of the SEQUENCE of piece lengths of that direction -- one process per GPU: the k-th ncclSend of a
// rank must meet the k-th ncclRecv of its neighbour with the same count, and a mismatch there is a hang, not an error)
constexpr int kFacts = 15;
struct RankFacts { double fused_ok, xd, sav, n_pad, snd_lo, rcv_lo, snd_hi, rcv_hi, xasync, both_splits, fsplit,
                   h_snd_lo, h_rcv_lo, h_snd_hi, h_rcv_hi; };
static_assert(sizeof(RankFacts) == kFacts * sizeof(double), "kFacts doubles");

// the part of a rank's facts that its halo runs decide
inline void halo_facts(const HaloRuns &h, RankFacts &f)
{
    f.snd_lo = (double)rows_of(h.send_lo); f.rcv_lo = (double)rows_of(h.recv_lo);
    f.snd_hi = (double)rows_of(h.send_hi); f.rcv_hi = (double)rows_of(h.recv_hi);
    f.h_snd_lo = digest(pieces_of(h.send_lo)); f.h_rcv_lo = digest(pieces_of(h.recv_lo));
    f.h_snd_hi = digest(pieces_of(h.send_hi)); f.h_rcv_hi = digest(pieces_of(h.recv_hi));
}

// every pair of neighbours in rank order; `pieces`: one process per GPU, the send / receive pairs have to meet
inline int check_neighbours(const std::vector<RankFacts> &facts, bool pieces, std::string &err)
{
    for (size_t g = 0; g + 1 < facts.size(); ++g) {
        if (facts[g].sav != facts[g + 1].sav) {
            err = "ec3d_multi: slabs chose different storage formats; call ec3d_multi_set_format(h, -1, 0) to use "
                  "bands + tail everywhere";
            return 105;
        }
        if (facts[g].snd_hi != facts[g + 1].rcv_lo || facts[g].rcv_hi != facts[g + 1].snd_lo) {
            err = "ec3d_multi: neighbouring slabs disagree on the halo size";
            return 105;
        }
        if (pieces && (facts[g].h_snd_hi != facts[g + 1].h_rcv_lo || facts[g].h_rcv_hi != facts[g + 1].h_snd_lo)) {
            err = "ec3d_multi: ranks " + std::to_string(g) + " and " + std::to_string(g + 1) +
                  " cut their halo into different pieces (same total): the send / receive pairs would not meet";
            return 105;
        }
    }
    return 0;
}

// ---- knobs -----------------------------------------------------------------------------------------------------------------
// Every environment knob that steers a slab job's set-up.  Constructing one reads them all, once: a set-up call does so on
// the calling thread, not once per process -- tests and tools change the environment between handles.  An unset knob stays
// unset: each use keeps its own default, clamping and precedence.
struct SlabKnobs {
    static std::optional<int> env(const char *name)
    {
        const char *e = getenv(name);
        return e ? std::optional<int>(atoi(e)) : std::nullopt;
    }
    std::optional<int> fuse = env("EC3D_SLAB_FUSE"), xdefer = env("EC3D_SLAB_XDEFER"), xasync = env("EC3D_XASYNC");
    std::optional<int> plan = env("EC3D_SLAB_PLAN"), fsplit = env("EC3D_SLAB_FSPLIT"), send_empty_u = env("EC3D_AV_SEND_EMPTY_U");
    bool u_always() const { return !(send_empty_u && *send_empty_u == 0); } // av_layout: every U plane travels
};

// ---- the job's decision ----------------------------------------------------------------------------------------------------
constexpr int kXdMax = 4; // EC3D_XD_MAX (ec3d_internal.hpp): deepest deferral of the X update
struct JobPlan {
    bool fused, xasync, both, fsplit;
    int xd;
    int chunk; // iterations between two looks at the stop flag: ONE value for the job (ranks leave together)
};
// What the whole job can do (the plan is a property of the job: the exchanges of the three-launch iteration differ
// from those of the five-launch one, and the rings of the deferred X update decide where an exchanged P or S lives).
//   fused: the single-component operator, EVERY slab on 2-D tiles with both fusions, the SpMV-form K4 and the spare
//          buffers in place (choose_sweep's size rule per slab: from 32 Mi rows; EC3D_FUSE23 / EC3D_FUSE51 / EC3D_K4S
//          force it on small grids).  EC3D_SLAB_FUSE=0 keeps five launches.
//   xd:    the smallest depth any slab allocated rings for (ec3d_spare_pair: 4 from 4.5 Mi streamed rows).
//          EC3D_SLAB_XDEFER=1 switches it off, 2 .. 4 caps it.
//          (a one-slab job keeps its slab's own depth: five launches, X every D-th iteration from 4.5 Mi rows, like any slab)
//   xasync: the groups of X updates on a stream of their own (ec3d_xasync) when every slab holds rings of two groups
//          (ec3d_spare_pair: a z-slab with the X update deferred does; EC3D_XASYNC=0 never) -- the ring depth decides
//          where an exchanged P or S lives, so it is the job's, like xd.  Only with the X update deferred, and
//          three-launch slabs keep the applying K4 (measured, the second launch costs them more than it fills) unless
//          EC3D_XASYNC=2.
//   both:  five launches with the exchange behind TWO of them (plan 5: K2 / K5 boundary planes first and K1 / K3 interior
//          planes first) when every slab can split both ways and the largest holds fewer than 10 Mi rows.  Measured
//          through the rank rehearsal against plan 1 (profiles/r05_plan5_both_splits.log): 2 Mi rows per rank 0.158 ->
//          0.149 ms per iteration, 6.75 Mi 0.268 -> 0.261, 16 Mi 0.480 -> 0.493 (there the four extra launches, each
//          beside a send / recv kernel, cost more than the waiting they remove).  The START of the P exchange differs
//          from plans 0 / 1 (behind K5's boundary launch, an iteration ahead), so the choice is the job's.
//          A-V slabs of the structured form (five planes per neighbour travel, one interior launch of a vector kernel
//          does not cover them): plan 5 against plan 2 -- config 5 on 8 / 4 / 2 ranks 0.306 -> 0.287 / 0.383 -> 0.343 /
//          0.504 -> 0.484 ms per iteration, config 3 on 2 / 4 ranks 0.277 -> 0.259 / 0.255 -> 0.249
//          (profiles/r05_plan5_av_slabs.log): at every size.
//          Plan 5 is OPT-IN (EC3D_SLAB_PLAN=5, the same on every rank) until a job of two real devices has verified it
//          bit for bit: everything measured for it (-3 ... -5 % below 10 Mi rows per rank, -10 % on A-V slabs) was measured
//          with the "neighbour" on the same card; `both` says where the one-card measurements would have picked it, and
//          nothing reads it yet.
//   fsplit: plans 3 and 4 issue the all-gather and the send / recv group in opposite host order: the job's choice.
//   chunk: about 0.4 ms of device work between two looks at the stop flag (as ec3d_solve.hip does), from the largest slab.
// kind: 1 the single-component operator, 2 the A-V system.
inline JobPlan decide_job(const std::vector<RankFacts> &facts, int kind, int world, const SlabKnobs &knob)
{
    JobPlan j{kind == 1 && world > 1, world > 1, world > 1, true, kXdMax, 1};
    double job_rows = 0;
    for (const RankFacts &f : facts) {
        j.fused = j.fused && f.fused_ok != 0.0;
        j.xd = std::min(j.xd, (int)f.xd);
        j.xasync = j.xasync && f.xasync != 0.0;
        j.both = j.both && f.both_splits != 0.0;
        j.fsplit = j.fsplit && f.fsplit != 0.0;
        job_rows = std::max(job_rows, f.n_pad);
    }
    j.both = j.both && (kind == 2 || job_rows < 10.0 * 1048576.0); // (A-V slabs: measured a gain at every size)
    if (knob.fuse) j.fused = j.fused && *knob.fuse != 0;
    if (knob.xdefer) j.xd = std::min(j.xd, std::max(1, *knob.xdefer));
    j.xasync = j.xasync && j.xd > 1 && (!j.fused || (knob.xasync && *knob.xasync == 2));
    const double est_us = job_rows * 264.0 / 4.0e6 + 12.0 + 20.0 * (world > 1);
    j.chunk = (int)std::min<double>(32.0, std::max<double>(1.0, 400.0 / est_us));
    return j;
}

enum { SPLIT_NONE = 0, SPLIT_PLANES, SPLIT_ROWS };
struct SlabPlan {
    int plan = 0;
    bool overlap_ok = false; // K1 / K3 can run as interior + boundary launch on this slab (asked inside plan 5 only)
    int halo_store = 0;      // Sweep::halo_store: bit 0 / 1, a neighbour below / above whose ghost rows the kernels fill
    int split = SPLIT_NONE;  // the boundary launch of K2 / K5 to ask the handle for: whole planes (ec3d_dist_set_boundary_planes:
                             // the single-component operator, window sweeps) or the rows of the halo runs (_rows)
};
// What the job's decision makes of rank `rank`; can_overlap: ec3d_can_overlap of its handle.
// EC3D_SLAB_PLAN (the SAME value on every rank: plan 2 orders its exchanges differently) picks the five-launch plan of
// a single-component job: 0 exchange in front of K1 / K3, 1 K1 / K3 split around it, 2 K2 / K5 boundary tiles first;
// 5 asks for plan 5 where plan 2 would run.  EC3D_SLAB_FSPLIT=0 keeps plan 3 where the job could run plan 4.
inline SlabPlan decide_slab(const JobPlan &job, int kind, int world, int rank, const SlabKnobs &knob, bool can_overlap)
{
    SlabPlan s;
    s.halo_store = job.fused ? ((rank > 0 ? 1 : 0) | (rank + 1 < world ? 2 : 0)) : 0;
    const int want_plan = knob.plan ? *knob.plan : -1;
    if (kind == 1 && !((want_plan == 2 || want_plan == 5) && !job.fused && world > 1)) {
        const bool no_fsplit = knob.fsplit && *knob.fsplit == 0;
        s.plan = job.fused ? ((job.fsplit && !no_fsplit) ? 4 : 3) : (can_overlap && want_plan != 0) ? 1 : 0;
    } else if (kind == 2 && want_plan == 0) {
        s.plan = 0; // (measurement: the A-V job with the exchange in front of K1 / K3, no split launches)
    } else if (world > 1) {
        // the ORDER of exchanges is a property of the job: every A-V rank uses the producer-side
        // plan; a rank whose slab is all boundary runs the whole kernels in that order
        s.plan = want_plan == 5 ? 5 : 2;
        s.overlap_ok = s.plan == 5 && can_overlap;
        s.split = kind == 1 ? SPLIT_PLANES : SPLIT_ROWS;
    }
    return s;
}
} // namespace ec3d_slab
