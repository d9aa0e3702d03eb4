// Stand-alone host program of tests/test_slab_plan_host.py: runs what csrc/ec3d_slab_plan.hpp states of a z-slab job -- the
// plans, the slabs' bounds, the halo runs and their pairing, the refusals, the knobs, the job's decision -- and prints, per
// case, what it gave and what came back:
//   case KIND NAME
//   KEY v v v ...        integers; a key that starts with "msg" is followed by text; "row" may repeat within a case
// Built with the address and undefined-behaviour sanitizers.
#include "../../eddy_currents_3d_amd/csrc/ec3d_slab_plan.hpp"

#include <climits>
#include <cstdio>

using namespace ec3d_slab;

namespace {
using Ints = std::vector<long long>;

void line(const std::string &key, const Ints &v)
{
    std::printf("%s", key.c_str());
    for (long long x : v) std::printf(" %lld", x);
    std::printf("\n");
}
void begin_case(const char *kind, const std::string &name) { std::printf("case %s %s\n", kind, name.c_str()); }
std::string R(const char *key, int rank) { return std::string(key) + "_" + std::to_string(rank); }

Ints flat(const std::vector<Op> &ops)
{
    Ints v;
    for (const Op &o : ops) v.insert(v.end(), {o.kind, o.arg, o.dit});
    return v;
}
Ints flat(const std::vector<Run> &rs)
{
    Ints v;
    for (const Run &r : rs) v.insert(v.end(), {r.start, r.pitch, r.payload, r.planes, r.lo(), r.hi()});
    return v;
}
Ints flat(const std::vector<Copy> &cs)
{
    Ints v;
    for (const Copy &c : cs) v.insert(v.end(), {c.dst, c.src, c.cnt});
    return v;
}
Ints flat(const std::vector<Piece> &ps)
{
    Ints v;
    for (const Piece &p : ps) v.insert(v.end(), {p.off, p.cnt});
    return v;
}
void print_runs(const HaloRuns &h, int rank)
{
    line(R("send_lo", rank), flat(h.send_lo));
    line(R("recv_lo", rank), flat(h.recv_lo));
    line(R("send_hi", rank), flat(h.send_hi));
    line(R("recv_hi", rank), flat(h.recv_hi));
}
void print_pieces(const HaloRuns &h, int rank)
{
    line(R("snd_lo", rank), flat(pieces_of(h.send_lo)));
    line(R("rcv_lo", rank), flat(pieces_of(h.recv_lo)));
    line(R("snd_hi", rank), flat(pieces_of(h.send_hi)));
    line(R("rcv_hi", rank), flat(pieces_of(h.recv_hi)));
}
Ints flat(const RankFacts &f)
{
    const double *d = &f.fused_ok;
    Ints v;
    for (int i = 0; i < kFacts; ++i) v.push_back((long long)d[i]);
    return v;
}

// the pulls of every slab of a one-process job, as finish_setup pairs them; the facts and what the neighbour check says
void pair_and_check(const std::vector<HaloRuns> &h, bool sav)
{
    const int n = (int)h.size();
    std::vector<RankFacts> facts((size_t)n);
    for (int g = 0; g < n; ++g) {
        std::vector<Copy> hi, lo;
        std::string why;
        int rc_hi = 0, rc_lo = 0;
        if (g + 1 < n) rc_hi = pair_up(h[(size_t)g].recv_hi, h[(size_t)g + 1].send_lo, hi, why);
        if (g > 0) rc_lo = pair_up(h[(size_t)g].recv_lo, h[(size_t)g - 1].send_hi, lo, why);
        line(R("pair_rc", g), {rc_hi, rc_lo});
        line(R("pull_hi", g), flat(hi));
        line(R("pull_lo", g), flat(lo));
        RankFacts f{};
        f.sav = sav;
        halo_facts(h[(size_t)g], f);
        facts[(size_t)g] = f;
        line(R("facts", g), flat(f));
    }
    std::string why;
    line("check", {check_neighbours(facts, false, why), check_neighbours(facts, true, why)});
}

void plan_cases()
{
    for (int p = 0; p <= 5; ++p) {
        begin_case("plan", std::to_string(p));
        line("begin", flat(begin_plan(p)));
        line("iter", flat(iter_plan(p)));
        // built once: the same object at every call
        line("same_object", {&begin_plan(p) == &begin_plan(p) && &iter_plan(p) == &iter_plan(p)});
    }
    begin_case("stage", "maps");
    Ints a, b, c;
    for (int st = 0; st < 19; ++st) {
        a.push_back(unsplit_stage(st));
        b.push_back(unsplit_spmv_stage(st));
        c.push_back(kernel_of_stage(st));
    }
    line("unsplit", a);
    line("unsplit_spmv", b);
    line("kernel", c);
    Ints vec(kVecOf, kVecOf + NHALO);
    line("vec_of", vec);
    line("channels", {CH_P, CH_S, CH_X, CH_AP, CH_R, NHALO, CH_SUM, CH_HUB, NCH});
    line("ops", {OP_HALO, OP_HALO_START, OP_HALO_WAIT, OP_GATHER, OP_STEP, OP_SKIP_IF_AP});
    for (int p = 0; p <= 5; ++p)
        for (int s = 0; s < 2; ++s)
            for (int o = 0; o < 2; ++o) {
                begin_case("launched", std::to_string(p) + "_" + std::to_string(s) + "_" + std::to_string(o));
                line("in", {p, s, o});
                Ints out;
                for (int st = 0; st < 19; ++st) out.push_back(launched_stage(p, s != 0, o != 0, st));
                line("out", out);
            }
}

void bounds_cases()
{
    for (int sdz = 1; sdz <= 70; ++sdz)
        for (int world = 1; world <= 8 && world <= sdz; ++world) {
            begin_case("bounds", std::to_string(sdz) + "_" + std::to_string(world));
            line("in", {sdz, world});
            Ints k, e0, e2;
            for (int r = 0; r < world; ++r) {
                int32_t k0 = -1, k1 = -1, a = -1, b = -1;
                slab_bounds(sdz, r, world, k0, k1);
                k.insert(k.end(), {k0, k1});
                held_range(sdz, k0, k1, 0, a, b);
                e0.insert(e0.end(), {a, b});
                held_range(sdz, k0, k1, 2, a, b);
                e2.insert(e2.end(), {a, b});
            }
            line("k", k);
            line("held0", e0);
            line("held2", e2);
        }
}

void msg_line(const char *key, int rc, const std::string &why)
{
    std::printf("%s %d %s\n", key, rc, why.c_str());
}

void cube_case(int world, int sdz, int64_t kdz, int64_t ghost)
{
    begin_case("cube", "w" + std::to_string(world) + "_z" + std::to_string(sdz) + "_g" + std::to_string(ghost));
    line("in", {world, sdz, kdz, ghost});
    std::vector<HaloRuns> h((size_t)world);
    Ints rcs;
    for (int r = 0; r < world; ++r) {
        int32_t k0, k1;
        slab_bounds(sdz, r, world, k0, k1);
        std::string why;
        const int rc = cube_runs(r, world, kdz, (int64_t)(k1 - k0) * kdz, ghost, h[(size_t)r], why);
        rcs.push_back(rc);
        msg_line(R("msg", r).c_str(), rc, why);
        print_runs(h[(size_t)r], r);
        print_pieces(h[(size_t)r], r);
    }
    line("rc", rcs);
    pair_and_check(h, false);
}

// conducting cells of every plane of the grid, by where the conductor lies relative to the cuts
enum Mask { ACROSS, ONE_SIDE, AWAY, EVERYWHERE, NMASK };
const char *mask_name[NMASK] = {"across", "oneside", "away", "everywhere"};
std::vector<int64_t> mask_cells(Mask m, int sdz, int world)
{
    std::vector<int> cut;
    for (int r = 1; r < world; ++r) {
        int32_t k0, k1;
        slab_bounds(sdz, r, world, k0, k1);
        cut.push_back(k0);
    }
    std::vector<int64_t> cells((size_t)sdz, 0);
    for (int z = 0; z < sdz; ++z) {
        bool on = m == EVERYWHERE || m == AWAY;
        for (size_t i = 0; i < cut.size(); ++i) {
            const int d = z - cut[i]; // planes cut - 2, cut - 1 lie below the cut, cut, cut + 1 above it
            if (m == ACROSS && d >= -2 && d < 2) on = true;
            if (m == ONE_SIDE && (i % 2 ? (d >= 0 && d < 2) : (d >= -2 && d < 0))) on = true;
            if (m == AWAY && d >= -2 && d < 2) on = false;
        }
        if (on) cells[(size_t)z] = 1 + z % 3;
    }
    return cells;
}

void av_case(Mask mask, int world, bool structured, bool u_always, bool rehearse)
{
    const int sdz = 23;
    const int64_t kdz = 6, pitch = structured ? 8 : 6;
    begin_case("av", std::string(mask_name[mask]) + "_w" + std::to_string(world) + (structured ? "_sav" : "_csr") +
                         (u_always ? "_all" : "_optin") + (rehearse ? "_rehearse" : ""));
    line("in", {world, structured, u_always, rehearse, sdz, kdz, pitch});
    const std::vector<int64_t> cells = mask_cells(mask, sdz, world);
    line("cells", Ints(cells.begin(), cells.end()));
    std::vector<HaloRuns> h((size_t)world);
    for (int r = 0; r < world; ++r) {
        AvSlab g{};
        slab_bounds(sdz, r, world, g.k0, g.k1);
        held_range(sdz, g.k0, g.k1, 2, g.e0, g.e1);
        const int np = g.e1 - g.e0;
        std::vector<int64_t> upl((size_t)np + 1, 0);
        for (int p = 0; p < np; ++p) upl[(size_t)p + 1] = upl[(size_t)p] + cells[(size_t)(g.e0 + p)];
        g.structured = structured;
        g.kdz = kdz;
        g.pitch = structured ? pitch : 0;
        g.nCd = structured ? np * pitch : 0;
        g.nC_ext = np * kdz;
        g.nU_ext = upl[(size_t)np];
        const AvLayout L = av_layout(g, upl, u_always, rehearse);
        line(R("geo", r), {g.k0, g.k1, g.e0, g.e1, g.nC_ext, g.nU_ext, g.nCd});
        line(R("upl", r), Ints(upl.begin(), upl.end()));
        Ints own(L.own_lo, L.own_lo + 4);
        own.insert(own.end(), L.own_hi, L.own_hi + 4);
        line(R("own", r), own);
        print_runs(L.runs, r);
        print_pieces(L.runs, r);
        std::vector<int64_t> blo, bhi;
        boundary_rows(L.runs, blo, bhi);
        line(R("bnd_lo", r), Ints(blo.begin(), blo.end()));
        line(R("bnd_hi", r), Ints(bhi.begin(), bhi.end()));
        h[(size_t)r] = L.runs;
    }
    if (!rehearse) pair_and_check(h, structured);
}

void refusal_cases()
{
    // two slabs of the single-component operator, 3 planes of 10 rows each, then one side altered
    HaloRuns a, b;
    std::string why;
    cube_runs(0, 2, 10, 30, 10, a, why);
    cube_runs(1, 2, 10, 30, 10, b, why);
    std::vector<Copy> out;
    begin_case("refuse", "pair_up");
    msg_line("msg_ok", pair_up(a.recv_hi, b.send_lo, out, why), why);
    {
        HaloRuns b2 = b;
        b2.send_lo.push_back(Run{10, 10, 10, 1}); // one run more than the neighbour expects
        why.clear();
        msg_line("msg_layout", pair_up(a.recv_hi, b2.send_lo, out, why), why);
    }
    {
        HaloRuns b2 = b;
        b2.send_lo[0].payload = 9;
        why.clear();
        msg_line("msg_size", pair_up(a.recv_hi, b2.send_lo, out, why), why);
        b2 = b;
        b2.send_lo[0].planes = 2;
        why.clear();
        msg_line("msg_planes", pair_up(a.recv_hi, b2.send_lo, out, why), why);
    }
    begin_case("refuse", "facts");
    std::vector<RankFacts> f(3);
    for (RankFacts &x : f) x = RankFacts{};
    // a middle rank between two others: 20 rows each way, cut into two pieces of 10
    const std::vector<Piece> two = {{0, 10}, {40, 10}}, uneven = {{0, 5}, {40, 15}}, one = {{0, 20}};
    for (RankFacts &x : f) {
        x.snd_lo = x.rcv_lo = x.snd_hi = x.rcv_hi = 20;
        x.h_snd_lo = x.h_rcv_lo = x.h_snd_hi = x.h_rcv_hi = digest(two);
    }
    f[0].snd_lo = f[0].rcv_lo = f[2].snd_hi = f[2].rcv_hi = 0;
    why.clear();
    msg_line("msg_ok", check_neighbours(f, true, why), why);
    {
        std::vector<RankFacts> g = f;
        g[2].sav = 1;
        why.clear();
        msg_line("msg_format", check_neighbours(g, true, why), why);
    }
    {
        std::vector<RankFacts> g = f;
        g[1].rcv_lo = 19;
        why.clear();
        msg_line("msg_size", check_neighbours(g, false, why), why);
    }
    {
        std::vector<RankFacts> g = f;
        g[2].h_rcv_lo = digest(uneven); // the same 20 rows, cut elsewhere
        why.clear();
        msg_line("msg_pieces", check_neighbours(g, true, why), why);
        why.clear();
        msg_line("msg_pieces_one_process", check_neighbours(g, false, why), why); // pulls: no pieces to meet
    }
    begin_case("digest", "lists");
    line("two", flat(two));
    line("uneven", flat(uneven));
    line("one", flat(one));
    line("empty", {});
    line("digests", {(long long)digest(two), (long long)digest(uneven), (long long)digest(one), (long long)digest({}),
                     (long long)digest(std::vector<Piece>(two))});
    const std::vector<Piece> big = {{0, (int64_t)1 << 40}, {7, 3}, {9, ((int64_t)1 << 33) + 5}};
    line("big", flat(big));
    line("digest_big", {(long long)digest(big)});
}

const int UNSET = INT_MIN;
void set_knob(std::optional<int> &k, int v) { k = v == UNSET ? std::nullopt : std::optional<int>(v); }
Ints flat(const SlabKnobs &k)
{
    auto v = [](const std::optional<int> &o) { return (long long)(o ? *o : UNSET); };
    return {v(k.fuse), v(k.xdefer), v(k.xasync), v(k.plan), v(k.fsplit), v(k.send_empty_u), k.u_always()};
}

void knob_cases()
{
    const char *names[6] = {"EC3D_SLAB_FUSE", "EC3D_SLAB_XDEFER", "EC3D_XASYNC", "EC3D_SLAB_PLAN", "EC3D_SLAB_FSPLIT",
                            "EC3D_AV_SEND_EMPTY_U"};
    for (const char *n : names) unsetenv(n);
    begin_case("knobs", "unset");
    line("got", flat(SlabKnobs()));
    for (int i = 0; i < 6; ++i) setenv(names[i], std::to_string(i + 2).c_str(), 1);
    begin_case("knobs", "two_to_seven"); // a second handle in the same process reads the environment anew
    line("got", flat(SlabKnobs()));
    for (const char *n : names) setenv(n, "0", 1);
    begin_case("knobs", "zero");
    line("got", flat(SlabKnobs()));
    for (const char *n : names) setenv(n, "", 1);
    begin_case("knobs", "empty"); // set and empty: atoi gives 0, as at every use before
    line("got", flat(SlabKnobs()));
    for (const char *n : names) unsetenv(n);
}

SlabKnobs no_knobs()
{
    SlabKnobs k;
    k.fuse = k.xdefer = k.xasync = k.plan = k.fsplit = k.send_empty_u = std::nullopt;
    return k;
}

RankFacts able(double n_pad)
{
    RankFacts f{};
    f.fused_ok = f.xasync = f.both_splits = f.fsplit = 1;
    f.xd = 4;
    f.n_pad = n_pad;
    return f;
}

void print_decision(const std::vector<RankFacts> &facts, int kind, int world, const SlabKnobs &knob)
{
    const JobPlan j = decide_job(facts, kind, world, knob);
    line("job", {j.fused, j.xd, j.xasync, j.both, j.fsplit, j.chunk});
    for (int r = 0; r < world; ++r)
        for (int can = 0; can < 2; ++can) {
            const SlabPlan s = decide_slab(j, kind, world, r, knob, can != 0);
            line(R("slab", r) + "_" + std::to_string(can), {s.plan, s.overlap_ok, s.halo_store, s.split});
        }
}

void decision_cases()
{
    const double Mi = 1048576.0;
    struct Flip { const char *name; double RankFacts::*field; double value; };
    const Flip flips[] = {{"able", &RankFacts::sav, 0},          {"nofuse", &RankFacts::fused_ok, 0},
                          {"xd1", &RankFacts::xd, 1},            {"xd2", &RankFacts::xd, 2},
                          {"noxasync", &RankFacts::xasync, 0},   {"noboth", &RankFacts::both_splits, 0},
                          {"nofsplit", &RankFacts::fsplit, 0},   {"below10Mi", &RankFacts::n_pad, 10 * Mi - 512},
                          {"at10Mi", &RankFacts::n_pad, 10 * Mi}};
    struct Knob { const char *name; std::optional<int> SlabKnobs::*field; std::vector<int> values; };
    const Knob knobs[] = {{"fuse", &SlabKnobs::fuse, {UNSET, 0, 1}},       {"xdefer", &SlabKnobs::xdefer, {-3, 0, 1, 2, 3, 4, 9}},
                          {"xasync", &SlabKnobs::xasync, {0, 1, 2}},       {"plan", &SlabKnobs::plan, {0, 1, 2, 3, 4, 5}},
                          {"fsplit", &SlabKnobs::fsplit, {0, 1}}};
    for (int kind = 1; kind <= 2; ++kind)
        for (int world : {1, 2, 4})
            for (const Flip &fl : flips)
                for (int who = world - 1; who >= 0; who -= std::max(1, world - 1)) { // the rank whose fact differs: last, first
                    if (who == 0 && world > 1 && fl.field == &RankFacts::sav) continue;
                    for (const Knob &kn : knobs)
                        for (int v : kn.values) {
                            std::vector<RankFacts> facts((size_t)world, able(Mi));
                            facts[(size_t)who].*fl.field = fl.value;
                            SlabKnobs knob = no_knobs();
                            set_knob(knob.*kn.field, v);
                            begin_case("decide", "k" + std::to_string(kind) + "_w" + std::to_string(world) + "_" + fl.name + "_r" +
                                                     std::to_string(who) + "_" + kn.name + (v == UNSET ? "unset" : std::to_string(v)));
                            line("in", {kind, world});
                            for (int r = 0; r < world; ++r) line(R("facts", r), flat(facts[(size_t)r]));
                            line("knobs", flat(knob));
                            print_decision(facts, kind, world, knob);
                        }
                }
    // a rehearsed rank: the facts of the one real rank decide for a job of four
    for (int kind = 1; kind <= 2; ++kind) {
        begin_case("decide", "k" + std::to_string(kind) + "_rehearsal_of_4");
        line("in", {kind, 4});
        const std::vector<RankFacts> facts(1, able(Mi));
        line("facts_0", flat(facts[0]));
        line("knobs", flat(no_knobs()));
        print_decision(facts, kind, 4, no_knobs());
    }
    for (int world : {1, 2})
        for (int lg : {19, 24, 27}) {
            begin_case("decide", "chunk_w" + std::to_string(world) + "_2p" + std::to_string(lg));
            line("in", {1, world});
            const std::vector<RankFacts> facts((size_t)world, able((double)((int64_t)1 << lg)));
            for (int r = 0; r < world; ++r) line(R("facts", r), flat(facts[(size_t)r]));
            line("knobs", flat(no_knobs()));
            print_decision(facts, 1, world, no_knobs());
        }
    // which plans the ranks of ONE job can be handed: every subset of ranks that cannot run the three-launch iteration
    // crossed with every subset whose producers cannot split, each rank with and without interior + boundary launches
    begin_case("sets", "all");
    for (int kind = 1; kind <= 2; ++kind)
        for (int world = 1; world <= 5; ++world)
            for (int plan : {UNSET, 0, 1, 2, 5})
                for (int fsplit : {UNSET, 0})
                    for (int nofuse = 0; nofuse < (1 << world); ++nofuse)
                        for (int nosplit = 0; nosplit < (1 << world); ++nosplit) {
                            std::vector<RankFacts> facts((size_t)world, able(Mi));
                            for (int r = 0; r < world; ++r) {
                                if (nofuse >> r & 1) facts[(size_t)r].fused_ok = 0;
                                if (nosplit >> r & 1) facts[(size_t)r].fsplit = 0;
                            }
                            SlabKnobs knob = no_knobs();
                            set_knob(knob.plan, plan);
                            set_knob(knob.fsplit, fsplit);
                            const JobPlan j = decide_job(facts, kind, world, knob);
                            Ints row = {kind, world, plan, fsplit, nofuse, nosplit};
                            for (int r = 0; r < world; ++r)
                                for (int can = 0; can < 2; ++can) row.push_back(decide_slab(j, kind, world, r, knob, can != 0).plan);
                            line("row", row);
                        }
}
} // namespace

int main()
{
    plan_cases();
    bounds_cases();
    for (int world = 2; world <= 5; ++world) cube_case(world, 11, 12, 12);
    cube_case(3, 50, 12, 512);
    cube_case(4, 50, 12, 512);
    cube_case(1, 5, 12, 0);   // one slab: no neighbour, no ghost zone needed
    cube_case(2, 2, 12, 11);  // a ghost zone one row short of a plane
    for (int m = 0; m < NMASK; ++m)
        for (int world = 2; world <= 5; ++world)
            for (int structured = 0; structured < 2; ++structured)
                for (int u_always = 0; u_always < 2; ++u_always)
                    for (int rehearse = 0; rehearse < 2; ++rehearse)
                        av_case((Mask)m, world, structured != 0, u_always != 0, rehearse != 0);
    refusal_cases();
    knob_cases();
    decision_cases();
    return 0;
}
