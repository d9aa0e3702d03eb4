// Stand-alone host program of tests/test_split_sweeps_host.py: makes the sweeps of small z-slab handles as choose_sweep
// would, hands them to the split rules of csrc/ec3d_split_sweeps.hpp and prints, per handle, what went in and what came back:
//   case KIND NAME
//   KEY v v v ...        integers: a sweep's fields (order: FIELDS in the test), a list, or a visit order
// Sweeps: sw k2 k5 ss (unsplit), then per split X in s (K1 / K3), f (2-D tiles), v (K2 / K5 by planes), r (K2 / K5 by rows):
// X_ok, X_bnd, X_inte, X_parts, the lists that came back, and the visit order of both launches (LAUNCH_off: first entry of
// every workgroup, LAUNCH_tiles).  Built with the address and undefined-behaviour sanitizers.
#include "../../eddy_currents_3d_amd/csrc/ec3d_split_sweeps.hpp"

#include <cstdio>
#include <string>

namespace {

template <class T> void line(const std::string &key, const std::vector<T> &v)
{
    std::printf("%s", key.c_str());
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

void sweep_line(const std::string &key, const Sweep &s)
{
    line<long long>(key, {s.ntiles, s.n, s.nblk, s.S, s.nt, s.vec_depth, s.pstride, s.zm_tpp, s.zm_pps, s.patch_npx, s.patch_sdx,
                          s.rp_px, s.rp_py, s.rp_npx, s.rp_sdy, s.rp_sdx, s.rp_pitch, s.nown, s.win_nt, s.win_blk, s.win_t0,
                          s.zm_pl0, s.zm_npl, s.zm_plstep, s.bnd_last, s.halo_store, s.part_off, s.ulist_n, s.il_planes,
                          s.il_nw, s.pair, s.ulist != nullptr, s.il_umask != nullptr, s.il_seg != nullptr, s.rp_flag != nullptr,
                          s.own_lo[0], s.own_lo[1], s.own_lo[2], s.own_lo[3], s.own_hi[0], s.own_hi[1], s.own_hi[2], s.own_hi[3]});
}

void visit_lines(const std::string &key, const Sweep &s, const std::vector<int32_t> &ul)
{
    std::vector<std::vector<int32_t>> v;
    ec3d_visit_of(s, ul, {}, {}, v);
    std::vector<int32_t> off{0}, tiles;
    for (auto &w : v) {
        tiles.insert(tiles.end(), w.begin(), w.end());
        off.push_back((int32_t)tiles.size());
    }
    line(key + "_off", off);
    line(key + "_tiles", tiles);
}

// lb, li: the lists that came back with the split; unsplit: the list of the sweep both members hold while it is refused
void split_lines(const std::string &x, const SplitSweep &k, const std::vector<int32_t> &lb, const std::vector<int32_t> &li,
                 const std::vector<int32_t> &unsplit)
{
    line<long long>(x + "_ok", {k.ok});
    sweep_line(x + "_bnd", k.bnd);
    sweep_line(x + "_inte", k.inte);
    line<long long>(x + "_parts", {k.parts()});
    line(x + "_lb", lb);
    line(x + "_li", li);
    visit_lines(x + "_vb", k.bnd, k.ok ? lb : unsplit);
    visit_lines(x + "_vi", k.inte, k.ok ? li : unsplit);
}

// the vector kernels' sweep as choose_sweep's vec_sweep makes it
Sweep vec_sweep(const Sweep &sw, int nblk, int map, int depth)
{
    Sweep k = sw;
    int64_t nb = std::min<int64_t>(sw.ntiles, nblk);
    k.S = 0;
    if (nb >= 8) {
        nb -= nb % 8;
        if (map) k.S = (int)(nb / 8);
    }
    k.nblk = (int)std::max<int64_t>(nb, 1);
    k.vec_depth = depth;
    return k;
}

// the z-marching sweep of `nplanes` planes of tpp tiles on about `want` workgroups (a request: ec3d_set_workgroups);
// literal: as many segments as `want` asks for, however few planes there are (workgroups past the last plane visit nothing)
void zmarch(Sweep &ss, int64_t tpp, int64_t nplanes, int want, bool literal = false)
{
    const int64_t cols = ec3d_cols8(tpp), max_seg = literal ? want : std::max<int64_t>(1, nplanes / 2);
    const int64_t nseg = ec3d_zm_segments(want, cols, max_seg, true);
    ss.zm_tpp = (int)tpp;
    ss.zm_pps = (int)((nplanes + nseg - 1) / nseg);
    ss.nblk = (int)(cols * nseg);
    ss.S = 0;
}

struct Handle {
    Sweep sw{}, k2{}, k5{}, ss{};
    int64_t halo = 0;
    int nown = 0;
    bool sav = false;
    std::vector<int32_t> ulist, us; // the U tiles as assembled, and in the SpMV kernels' order
    std::vector<int64_t> lo, hi;    // boundary row ranges of the rank driver
};

void print_handle(const char *kind, const std::string &name, Handle &h)
{
    std::printf("case %s %s\n", kind, name.c_str());
    std::vector<int32_t> ii, ib, vb, vi;
    SplitSweep s = ec3d_split_spmv_planes(h.sw, h.ss, h.halo, h.nown);
    if (!s.ok && h.sav) s = ec3d_split_spmv_av(h.sw, h.ss, h.halo, h.ulist, ii, ib);
    const SplitSweep f = ec3d_split_tiles2d(h.sw, h.ss, h.halo, h.nown);
    const SplitSweep v = ec3d_split_vec_planes(h.k2, h.ss, h.sav, h.halo, h.nown);
    const SplitSweep r = ec3d_split_vec_rows(h.sw, h.ulist, (int)h.lo.size(), h.lo.data(), h.hi.data(), vb, vi);
    const int ps = ec3d_partial_stride(h.sw, h.k2, h.k5, h.ss, s, f, v.ok ? v : r);
    line<long long>("in", {h.halo, h.nown, h.sav, ec3d_vec_planes_splittable(h.k2, h.ss, h.sav, h.halo, h.nown)});
    line<long long>("stride", {ps, kVecBndCap});
    line("ulist", h.ulist);
    line("us", h.us);
    line("lo", h.lo);
    line("hi", h.hi);
    sweep_line("sw", h.sw);
    sweep_line("k2", h.k2);
    sweep_line("k5", h.k5);
    sweep_line("ss", h.ss);
    visit_lines("ss", h.ss, h.us);
    visit_lines("k2", h.k2, h.ulist);
    visit_lines("sw", h.sw, h.ulist);
    split_lines("s", s, ib, ii, h.us);
    split_lines("f", f, {}, {}, h.us);
    split_lines("v", v, {}, {}, h.ulist);
    split_lines("r", r, vb, vi, h.ulist);
}

// slab of the single-component operator: np planes of tpp tiles held, `extra` tiles of padding behind them
Handle single(int tpp, int np, int want, bool patch, int extra = 0, bool literal = false)
{
    Handle h;
    h.sw.bnd_last = -1;
    h.sw.ntiles = (int64_t)np * tpp + extra;
    h.sw.n = h.sw.ntiles * EC3D_TILE;
    h.halo = (int64_t)tpp * EC3D_TILE;
    const Sweep base = h.sw;
    const int map = want != 48; // the plain tile order at 48 workgroups, the XCD-aware window elsewhere
    h.k2 = vec_sweep(base, want, map, 1);
    h.k5 = vec_sweep(base, std::min(want, 256), 0, 2);
    h.ss = vec_sweep(base, want, 1, 1);
    h.sw = vec_sweep(base, want, map, 1);
    zmarch(h.ss, tpp, (h.sw.ntiles + tpp - 1) / tpp, want, literal);
    if (patch && h.ss.zm_tpp > 0) {
        h.ss.patch_npx = tpp % 2 ? 1 : 2;
        h.ss.patch_sdx = (int64_t)h.ss.patch_npx * EC3D_PX;
    }
    // the rank driver's ranges: the first and the last plane held
    h.lo = {0, (int64_t)(np - 1) * tpp * EC3D_TILE};
    h.hi = {(int64_t)tpp * EC3D_TILE, (int64_t)np * tpp * EC3D_TILE};
    return h;
}

// slab of the structured A-V form: blocks of p0 + npo + 2 planes of tpp tiles, of which the npo from p0 on are owned; U tiles
// at (owned plane, column) with (plane + column) % 3 != 1, and `stray` (>= 0: a tile appended to that list)
Handle av(int tpp, int npo, int p0, int want, int32_t stray = -1)
{
    Handle h;
    const int64_t blk = (int64_t)(p0 + npo + 2) * tpp;
    h.sav = true;
    h.nown = 4;
    h.halo = (int64_t)tpp * EC3D_TILE;
    h.sw.bnd_last = -1;
    h.sw.n = 4 * blk * EC3D_TILE;
    h.sw.win_blk = blk;
    h.sw.win_t0 = (int64_t)p0 * tpp;
    h.sw.win_nt = (int64_t)npo * tpp;
    h.sw.ntiles = 3 * h.sw.win_nt;
    for (int q = 0; q < 4; ++q) { // (the handle's ownership ranges travel with every sweep, unused by a windowed one)
        h.sw.own_lo[q] = (q * blk + h.sw.win_t0) * EC3D_TILE;
        h.sw.own_hi[q] = h.sw.own_lo[q] + h.sw.win_nt * EC3D_TILE;
    }
    for (int pl = 0; pl < npo; ++pl)
        for (int col = 0; col < tpp; ++col)
            if ((pl + col) % 3 != 1) h.ulist.push_back((int32_t)(3 * blk + (int64_t)(p0 + pl) * tpp + col));
    if (stray >= 0) h.ulist.push_back(stray);
    h.sw.ulist_n = (int)h.ulist.size();
    const Sweep base = h.sw;
    h.k2 = vec_sweep(base, want, 1, 1);
    h.k5 = vec_sweep(base, want, 1, 1);
    h.ss = vec_sweep(base, want, 1, 1);
    h.sw = vec_sweep(base, want, 1, 1);
    zmarch(h.ss, tpp, 3 * npo, want);
    h.us = ec3d_xcd_local_order(h.ulist, tpp, h.ss.nblk);
    h.ss.ulist_n = (int)h.us.size();
    // the rank driver's ranges: the two owned planes next to each cut, in every block
    for (int d = 0; d < 4; ++d)
        for (int64_t pl : {(int64_t)p0, (int64_t)p0 + npo - 2}) {
            h.lo.push_back((d * blk + pl * tpp) * EC3D_TILE);
            h.hi.push_back((d * blk + (pl + 2) * tpp) * EC3D_TILE);
        }
    return h;
}

} // namespace

int main()
{
    for (int tpp : {1, 2, 3, 8, 12, 32})
        for (int np : {2, 3, 9, 10, 11, 24})
            for (int want : {8, 48, 1536})
                for (int patch : {1, 0}) {
                    if (!patch && want != 48) continue;
                    Handle h = single(tpp, np, want, patch != 0);
                    print_handle("single", "t" + std::to_string(tpp) + "_p" + std::to_string(np) + "_w" + std::to_string(want) +
                                               (patch ? "_2d" : "_lin"), h);
                }
    for (int np : {11, 24})
        for (int want : {8, 48, 1536}) { // an SpMV grid of exactly 8, 48 and 1536 workgroups
            Handle h = single(8, np, want, true, 0, true);
            print_handle("single", "literal_p" + std::to_string(np) + "_w" + std::to_string(want), h);
        }
    // SpMV grids of half a column row more than whole ones (no request makes choose_sweep plan one; its last four workgroups
    // visit nothing): where rounding to the nearest number of segments and rounding down part
    for (int want : {8, 48}) {
        Handle h = single(3, 24, want, true);
        h.ss.nblk += 4;
        print_handle("single", "odd_grid_w" + std::to_string(want), h);
    }
    {
        Handle h = av(3, 12, 0, 48);
        h.ss.nblk += 4;
        h.us = h.ulist; // (the XCD-local order wants a multiple of 8)
        h.ss.ulist_n = (int)h.us.size();
        print_handle("av", "odd_grid_w48", h);
    }
    {
        Handle h = single(3, 11, 48, true);
        h.halo = 0;
        print_handle("single", "no_halo", h);
        h = single(3, 11, 48, true);
        h.nown = 4;
        print_handle("single", "ownership_ranges", h);
        h = single(3, 11, 48, true, 1);
        print_handle("single", "ragged_last_plane", h);
        h = single(3, 11, 48, true);
        h.lo = {0};
        h.hi = {h.sw.n};
        print_handle("single", "rows_all_boundary", h);
        h = single(3, 11, 48, true);
        h.lo.clear();
        h.hi.clear();
        print_handle("single", "rows_no_range", h);
    }
    for (int tpp : {1, 3, 8, 12})
        for (int npo : {5, 6, 7, 12})
            for (int p0 : {0, 2})
                for (int want : {8, 48, 1536}) {
                    Handle h = av(tpp, npo, p0, want);
                    print_handle("av", "t" + std::to_string(tpp) + "_n" + std::to_string(npo) + "_p" + std::to_string(p0) + "_w" +
                                           std::to_string(want), h);
                }
    {
        Handle h = av(3, 7, 2, 48, (int32_t)(3 * 11 * 3 + 9 * 3 + 1)); // a U tile in the halo plane above the window
        print_handle("av", "u_tile_in_the_halo", h);
        h = av(3, 7, 2, 48);
        h.ss.rp_px = 64;
        print_handle("av", "on_2d_tiles", h);
        h = av(3, 7, 2, 48);
        h.halo = 0;
        print_handle("av", "no_halo", h);
        h = av(3, 7, 2, 48);
        h.sw.win_t0 += 1;
        print_handle("av", "window_off_a_plane", h);
    }
    return 0;
}
