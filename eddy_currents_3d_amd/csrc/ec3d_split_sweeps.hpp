// ec3d_split_sweeps.hpp — the launch pairs of a z-slab (host only: no HIP call, no kernels, no handle).  A slab runs
// several kernels as a boundary launch plus an interior launch, so that the halo exchange overlaps the interior; every such
// pair is a SplitSweep (ec3d_internal.hpp) derived here from the unsplit sweeps and a few integers:
//   ec3d_split_spmv_planes  K1 / K3 of the single-component slab              (ec3d_get_visit_order 3 / 4)
//   ec3d_split_spmv_av      K1 / K3 of the structured A-V slab with a window  (3 / 4)
//   ec3d_split_tiles2d      the 2-D-tile kernels of the three-launch iteration (7 / 8)
//   ec3d_split_vec_planes   K2 / K5 as plane windows                          (5 / 6)
//   ec3d_split_vec_rows     K2 / K5 from tile lists                           (5 / 6)
// together with the stride of the partial-sum buffer that has room for all of them and the visit order of any sweep.
// choose_sweep (ec3d_context.hip) and ec3d_dist_set_boundary_* (ec3d_dist.hip) decide WHEN each is asked for, upload the
// lists that come back and put the device pointers in; the arithmetic lives here so that it runs without a GPU.
// tests/test_split_sweeps_host.py checks every field against a Python restatement.
#pragma once
#include "ec3d_internal.hpp"
#include "ec3d_sweep_lists.hpp"

// most workgroups of the boundary launch of a split vector kernel (K2, K5) and of a split SpMV kernel (K1, K3)
constexpr int kVecBndCap = 256, kSpmvBndCap = 768;

// columns of a z-marching grid as the 8 XCD labels are dealt them (runs of cols / 8; with tpp % 8 != 0 the last is short)
inline int64_t ec3d_cols8(int64_t tpp) { return (tpp + 7) / 8 * 8; }
// workgroups of a launch on an XCD-aware map: whole multiples of 8, at least 8
inline int ec3d_nblk8(int64_t want) { return (int)std::max<int64_t>(8, want / 8 * 8); }
// z-march of `planes` planes on about as many workgroups as the unsplit launch runs (whole columns of segments; nearest:
// rounded, else rounded down), no segment shorter than min_pps planes
inline void ec3d_march_grid(Sweep &s, int64_t want_nblk, int64_t planes, int64_t min_pps, bool nearest)
{
    const int64_t cols = ec3d_cols8(s.zm_tpp);
    int64_t nseg = std::max<int64_t>(1, (want_nblk + (nearest ? cols / 2 : 0)) / cols);
    nseg = std::min<int64_t>(nseg, std::max<int64_t>(1, planes / min_pps));
    s.zm_pps = (int)((planes + nseg - 1) / nseg);
    s.nblk = (int)(cols * nseg);
}
// planes a slab of the single-component operator holds (sw: the vector kernels' sweep, ss: the z-marching one), 0 when it is
// not one or its rows are no whole number of planes
inline int64_t ec3d_slab_planes(const Sweep &sw, const Sweep &ss, int64_t halo, int nown)
{
    if (halo <= 0 || nown != 0 || ss.zm_tpp <= 0) return 0;
    const int64_t np = sw.ntiles / ss.zm_tpp;
    return np * ss.zm_tpp == sw.ntiles ? np : 0;
}

// z-slab of the single-component operator on a z-marching grid: K1 / K3 as an interior launch (planes 1 .. np-2,
// independent of the halo) and a boundary launch (planes 0 and np-1); from 10 planes held
inline SplitSweep ec3d_split_spmv_planes(const Sweep &sw, const Sweep &ss, int64_t halo, int nown)
{
    SplitSweep k{ss, ss, false};
    const int64_t np = ec3d_slab_planes(sw, ss, halo, nown);
    if (np < 10) return k;
    k.inte.zm_pl0 = 1;
    k.inte.zm_npl = (int)(np - 2);
    ec3d_march_grid(k.inte, ss.nblk, np - 2, 8, true);
    k.inte.part_off = 0;
    k.bnd.bnd_last = (int)(np - 1);
    k.bnd.patch_npx = 0; // the boundary planes go through the plain kernels: 512 consecutive cells per tile
    k.bnd.nblk = (int)std::min<int64_t>(2 * (int64_t)ss.zm_tpp, kSpmvBndCap);
    k.bnd.part_off = k.inte.nblk;
    k.ok = true;
    return k;
}

// z-slab of the STRUCTURED A-V form with tile-aligned planes (sw: the windowed sweep): K1 / K3 as interior + boundary launch
// too.  The A rows and the U rows read A one plane away, the one-sided A-U stencils (src/EC3D.f90:697-706) read U two planes
// away, so the two owned planes next to each cut are "boundary" in all four blocks.  Interior launch: the z-march over the
// window narrowed by two planes at both ends in every A block, then the U tiles of those planes (ii, in the XCD-local
// order).  Boundary launch: no front sweep at all -- the tiles of the four outer planes of the three A blocks and the U
// tiles there, as ONE list (ib; a listed tile starts its march afresh, which is what a tile of a lone plane needs anyway).
// ulist: the handle's U tiles.  The caller uploads ii and ib and points inte.ulist / bnd.ulist at them.  Refused below
// 2 H + 2 owned planes, on 2-D tiles, and when a U tile lies outside the owned planes.
inline SplitSweep ec3d_split_spmv_av(const Sweep &sw, const Sweep &ss, int64_t halo, const std::vector<int32_t> &ulist,
                                     std::vector<int32_t> &ii, std::vector<int32_t> &ib)
{
    SplitSweep k{ss, ss, false};
    ii.clear();
    ib.clear();
    if (halo <= 0 || sw.win_nt <= 0 || ss.zm_tpp <= 0 || ss.rp_px != 0) return k;
    const int64_t tpp = ss.zm_tpp, npo = sw.win_nt / tpp, H = 2, p0 = sw.win_t0 / tpp, npi = npo - 2 * H;
    if (npo * tpp != sw.win_nt || p0 * tpp != sw.win_t0 || npo < 2 * H + 2) return k;
    std::vector<int32_t> ui, ub;
    if (!ec3d_slab_split_lists(ulist, tpp, sw.win_blk, p0, npo, H, ui, ub, ib)) return k;
    k.inte.win_t0 = sw.win_t0 + H * tpp;
    k.inte.win_nt = npi * tpp;
    k.inte.ntiles = 3 * k.inte.win_nt;
    ec3d_march_grid(k.inte, ss.nblk, 3 * npi, 2, false);
    k.inte.part_off = 0;
    if (!ui.empty()) ii = ec3d_xcd_local_order(ui, tpp, k.inte.nblk);
    k.inte.ulist = nullptr;
    k.inte.ulist_n = (int)ii.size();
    k.bnd.ntiles = 0; // (no front sweep: ec3d_tile_of / walk_zm find no plane whose tile exists)
    k.bnd.win_nt = 0;
    k.bnd.ulist = nullptr;
    k.bnd.ulist_n = (int)ib.size();
    k.bnd.nblk = ec3d_nblk8(std::min<int64_t>((int64_t)ib.size(), kSpmvBndCap));
    k.bnd.part_off = k.inte.nblk;
    k.ok = true;
    return k;
}

// z-slab of the single-component operator on 2-D tiles: the 2-D-tile kernels in two launches too -- planes 0 and np-1 (one
// plane per workgroup: zm_plstep), then planes 1 .. np-2 -- for the producers of the exchanged vectors in the three-launch
// iteration (K4 in SpMV form makes R, K5-in-K1 the next AP; ec3d_multi.hip plan 4); from 3 planes held
inline SplitSweep ec3d_split_tiles2d(const Sweep &sw, const Sweep &ss, int64_t halo, int nown)
{
    SplitSweep k{ss, ss, false};
    const int64_t np = ss.patch_npx > 0 ? ec3d_slab_planes(sw, ss, halo, nown) : 0;
    if (np < 3) return k;
    k.bnd.zm_pl0 = 0;
    k.bnd.zm_plstep = (int)(np - 1);
    k.bnd.zm_npl = 2;
    k.bnd.zm_pps = 1;
    k.bnd.nblk = (int)(ec3d_cols8(ss.zm_tpp) * 2);
    k.bnd.part_off = 0;
    k.inte.zm_pl0 = 1;
    k.inte.zm_npl = (int)(np - 2);
    ec3d_march_grid(k.inte, ss.nblk, np - 2, 2, true);
    k.inte.part_off = k.bnd.nblk;
    k.ok = true;
    return k;
}

// K2 / K5 of a z-slab of the SINGLE-COMPONENT operator whose planes are whole tiles, without tile lists: the boundary launch
// takes the first and the last owned plane, the interior launch the planes between, both as windows of the ordinary strided
// sweep (Sweep::win_*: logical tile t of the boundary launch is tile t of plane 0 for t < tpp, of plane np-1 after; the
// interior launch starts at plane 1) -- a list-driven K2 / K5 costs 15-30 us more at 16 Mi rows than the strided one.
// k2: K2's sweep; from 3 planes held.
inline bool ec3d_vec_planes_splittable(const Sweep &k2, const Sweep &ss, bool sav, int64_t halo, int nown)
{
    return !sav && k2.ulist_n == 0 && k2.win_nt == 0 && ec3d_slab_planes(k2, ss, halo, nown) >= 3;
}
inline SplitSweep ec3d_split_vec_planes(const Sweep &k2, const Sweep &ss, bool sav, int64_t halo, int nown)
{
    SplitSweep k{k2, k2, false};
    if (!ec3d_vec_planes_splittable(k2, ss, sav, halo, nown)) return k;
    const int64_t tpp = ss.zm_tpp, total = k2.ntiles;
    k.bnd.ntiles = 2 * tpp;
    k.bnd.win_nt = tpp;
    k.bnd.win_blk = total - tpp;
    k.bnd.win_t0 = 0;
    k.bnd.S = 0;
    k.bnd.vec_depth = 1;
    k.bnd.nblk = ec3d_nblk8(std::min<int64_t>(2 * tpp, kVecBndCap));
    k.bnd.part_off = 0;
    k.inte.ntiles = total - 2 * tpp;
    k.inte.win_nt = k.inte.ntiles;
    k.inte.win_blk = total;
    k.inte.win_t0 = tpp;
    k.inte.nblk = std::min(k2.nblk, ec3d_nblk8(k.inte.ntiles));
    k.inte.S = k2.S > 0 ? k.inte.nblk / 8 : 0;
    k.inte.part_off = k.bnd.nblk;
    k.ok = true;
    return k;
}

// K2 / K5 from tile lists: of the tiles the vector kernels visit (sw: their sweep, ulist: the host copy of its U list) those
// that hold a row of one of the ranges [lo[q], hi[q]) go to the boundary launch (vb), the others to the interior launch
// (vi).  The caller uploads both and points bnd.ulist / inte.ulist at them.  Refused when either list is empty (a single
// rank, or a slab that is all boundary).
inline SplitSweep ec3d_split_vec_rows(const Sweep &sw, const std::vector<int32_t> &ulist, int nranges, const int64_t *lo,
                                      const int64_t *hi, std::vector<int32_t> &vb, std::vector<int32_t> &vi)
{
    SplitSweep k{sw, sw, false};
    vb.clear();
    vi.clear();
    std::vector<int32_t> visit((size_t)sw.ntiles);
    for (int64_t t = 0; t < sw.ntiles; ++t) visit[(size_t)t] = (int32_t)ec3d_phys_tile(sw, t);
    visit.insert(visit.end(), ulist.begin(), ulist.end());
    for (int32_t t : visit) {
        const int64_t r0 = (int64_t)t * EC3D_TILE, r1 = r0 + EC3D_TILE;
        bool bnd = false;
        for (int q = 0; q < nranges && !bnd; ++q) bnd = lo[q] < r1 && hi[q] > r0;
        (bnd ? vb : vi).push_back(t);
    }
    if (vb.empty() || vi.empty()) return k;
    auto list_sweep = [&](Sweep &s, size_t len, int max_blk, int part_off) {
        s.ntiles = 0; // list only
        s.ulist = nullptr;
        s.ulist_n = (int)len;
        s.nblk = (int)std::min<size_t>(len, (size_t)max_blk);
        s.S = 0;
        s.part_off = part_off;
    };
    list_sweep(k.bnd, vb.size(), kVecBndCap, 0);
    list_sweep(k.inte, vi.size(), sw.nblk, k.bnd.nblk);
    k.ok = true;
    return k;
}

// Doubles between two slots of the partial-sum buffer: room for every producer's workgroups, a split producer's two launches
// side by side.  sw, k2, k5: the vector kernels' sweeps, ss: the SpMV kernels'.  A vector kernel may be split after the
// stride is fixed (ec3d_dist_set_boundary_*): its interior launch runs no more workgroups than the unsplit kernel, its
// boundary launch at most kVecBndCap.
inline int ec3d_partial_stride(const Sweep &sw, const Sweep &k2, const Sweep &k5, const Sweep &ss, const SplitSweep &spmv,
                               const SplitSweep &tiles2d, const SplitSweep &vec)
{
    const int vmax = std::max(sw.nblk, std::max(k2.nblk, k5.nblk));
    int ps = std::max(vmax + kVecBndCap, ss.nblk);
    for (const SplitSweep *k : {&spmv, &tiles2d, &vec})
        if (k->ok) ps = std::max(ps, k->parts());
    return ps;
}

// The tiles every workgroup of a launch visits, in order -- exactly what EC3D_SWEEP_BEGIN_ does on the device (same
// ec3d_tile_of, same list rules).  The oracle's "GPU order" twin takes this as data.  ul: host copy of sw.ulist (ulist_n
// entries); il_seg, il_umask: host copies of the interleaved z-march's lists (read only when sw.il_planes > 0).
inline void ec3d_visit_of(const Sweep &sw, const std::vector<int32_t> &ul, const std::vector<int32_t> &il_seg,
                          const std::vector<uint32_t> &il_umask, std::vector<std::vector<int32_t>> &out)
{
    if (sw.il_planes > 0) { // the interleaved z-march of the structured form: walk_zm_il, step by step
        const int64_t tpp = sw.zm_tpp, P = sw.il_planes, blk_t = P * tpp;
        for (int b = 0; b < sw.nblk; ++b) {
            std::vector<int32_t> v;
            const int64_t col = il_seg[(size_t)b * 4];
            for (int64_t k = il_seg[(size_t)b * 4 + 1]; k < il_seg[(size_t)b * 4 + 2]; ++k) {
                const int64_t t0 = k * tpp + col;
                for (int d = 0; d < 3; ++d) v.push_back((int32_t)(t0 + d * blk_t));
                if (ec3d_il_bit(il_umask.data(), sw.il_nw, col, k)) v.push_back((int32_t)(t0 + 3 * blk_t));
            }
            out.push_back(std::move(v));
        }
        return;
    }
    for (int b = 0; b < sw.nblk; ++b) {
        std::vector<int32_t> v;
        for (int64_t it = 0;; ++it) {
            const int64_t tile = ec3d_tile_of(sw, b, it);
            if (tile < 0) break;
            v.push_back((int32_t)tile);
        }
        // a hole (-1) of the XCD-local list ends the workgroup's share
        for (int64_t l = b; l < sw.ulist_n && ul[(size_t)l] >= 0; l += sw.nblk) v.push_back(ul[(size_t)l]);
        out.push_back(std::move(v));
    }
}
