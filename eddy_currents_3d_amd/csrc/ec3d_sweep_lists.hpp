// ec3d_sweep_lists.hpp — the tile lists choose_sweep (ec3d_context.hip) builds on the host for the SpMV kernels of the
// structured A-V form, and the two small rules that go with them (host only: no HIP call, no kernels, no handle): the
// shape of the runtime-shaped 2-D tiles and their per-tile tables, the z segments of a z-marching grid, the U mask and
// the work list of the interleaved z-march, the XCD-local order of a list of U tiles, and the interior / boundary lists
// of a z-slab; and which launches of the 2-D tiles run paired patch columns (ec3d_patch_pair_virtual is the one function
// here that the kernels call too).  choose_sweep decides WHEN each is used and uploads the result; the arithmetic lives
// here so that it runs without a GPU.  tests/test_sweep_lists_host.py checks every list against a numpy restatement.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

// Runtime-shaped 2-D tiles for the structured A-V form (sav_patch_step in ec3d_kernels.hip): the patch shape for a
// grid of sdx x sdy cells per plane and tiles of `tile` rows (512).  px must be even (a thread owns two consecutive
// cells) and divide sdx (no ragged patch columns), px * py <= 512, py >= 2; the last patch ROW may be ragged.  Score =
// the share of the 512 thread-cells of a tile that are real cells; at least 32 cells per patch row (256-byte pieces of
// a vector) unless the grid itself is narrower; ties go to the px nearest 128 (the shape the cube kernels were tuned on).
inline double ec3d_pick_patch_shape(int64_t sdx, int64_t sdy, int64_t tile, int &px_out, int &py_out)
{
    double best = 0.0;
    px_out = py_out = 0;
    if (sdx % 2) return 0.0;
    for (int64_t px = 4; px <= std::min<int64_t>(sdx, 256); px += 2) {
        if (sdx % px) continue;
        if (px < 32 && px != sdx) continue;
        const int64_t py = tile / px;
        if (py < 2) continue;
        const int64_t npy = (sdy + py - 1) / py;
        const double eff = (double)(px * py) / tile * (double)sdy / (double)(npy * py);
        const bool better = eff > best + 1e-9 ||
                            (eff > best - 1e-9 && std::llabs(px - 128) < std::llabs((int64_t)px_out - 128));
        if (better) {
            best = std::max(best, eff);
            px_out = (int)px;
            py_out = (int)py;
        }
    }
    return best;
}

// per patch tile of the three A blocks: does it hold a coupled row?  and the patch tiles of the U block that hold an
// unknown (ascending): from the class bytes `cls` of the 4 * planes stacked planes of `pitch` rows each.  A rows are
// coupled in classes [sav_a0, sav_u0), U rows hold an unknown in classes [sav_u0, sav_zero).
inline void ec3d_patch_tables(const uint8_t *cls, int64_t planes, int64_t pitch, int64_t sdx, int64_t sdy, int px, int py,
                              int sav_a0, int sav_u0, int sav_zero, std::vector<uint8_t> &flag, std::vector<int32_t> &ulist)
{
    const int64_t npx = sdx / px, npy = (sdy + py - 1) / py, tpp = npx * npy;
    flag.assign((size_t)(3 * planes * tpp) + 4, 0); // + 4: read by dwords
    ulist.clear();
    for (int64_t P = 0; P < 4 * planes; ++P)
        for (int64_t q = 0; q < tpp; ++q) {
            const int64_t pyi = q / npx, pxi = q % npx;
            bool any = false;
            for (int64_t y = pyi * py; y < std::min<int64_t>(sdy, (pyi + 1) * py) && !any; ++y) {
                const uint8_t *row = &cls[(size_t)(P * pitch + y * sdx + pxi * px)];
                for (int x = 0; x < px; ++x) {
                    const int k = row[x];
                    if (P < 3 * planes ? (k >= sav_a0 && k < sav_u0) : (k >= sav_u0 && k < sav_zero)) {
                        any = true;
                        break;
                    }
                }
            }
            if (!any) continue;
            if (P < 3 * planes) flag[(size_t)(P * tpp + q)] = 1;
            else ulist.push_back((int32_t)(P * tpp + q));
        }
}

// The 2-D tiles of the single-component operator in the dictionary form (patch_pair in ec3d_kernels.hip): does a class
// array of n rows with the band offsets off[0 .. nb) divide into px x py patches, plane by plane?  planes = n / kdz,
// tpp = patches per plane (padded rows of a plane included: they carry class bytes like any other row).
inline bool ec3d_class_runs_shape(int nb, const int64_t *off, int64_t n, int px, int py, int64_t &planes, int64_t &tpp)
{
    planes = tpp = 0;
    if (nb != 7) return false;
    const int64_t sdx = off[5], kdz = off[6];
    if (sdx <= 0 || kdz <= 0 || sdx % px || kdz % sdx || (kdz / sdx) % py || n <= 0 || n % kdz) return false;
    planes = n / kdz;
    tpp = kdz / ((int64_t)px * py);
    return true;
}
// "Same classes as the tile below", one byte per patch tile (tile = plane * tpp + q, patch q of a plane is
// (q % npx, q / npx) as in ec3d_row_of): flag = 1 exactly when plane > 0 and all px * py class bytes of the patch equal
// those kdz rows below.  A z-marching workgroup that steps onto such a tile keeps the class pairs it holds.  The class
// array stays the only source of truth: the flags say nothing it does not.  Behind the planes * tpp flags come tpp + 4
// zeros: the kernels read the flag of the tile ABOVE the one they are at (a step ahead), by dwords.
inline void ec3d_class_runs(const uint8_t *cls, int64_t planes, int64_t kdz, int64_t sdx, int px, int py,
                            std::vector<uint8_t> &flag)
{
    const int64_t npx = sdx / px, tpp = kdz / ((int64_t)px * py);
    flag.assign((size_t)(planes * tpp + tpp + 4), 0);
    for (int64_t k = 1; k < planes; ++k)
        for (int64_t q = 0; q < tpp; ++q) {
            const int64_t pyi = q / npx, pxi = q % npx;
            bool same = true;
            for (int y = 0; y < py && same; ++y) {
                const uint8_t *row = &cls[(size_t)(k * kdz + (pyi * py + y) * sdx + pxi * px)];
                same = std::equal(row, row + px, row - kdz);
            }
            flag[(size_t)(k * tpp + q)] = same ? 1 : 0;
        }
}

// Paired patch columns (patch_pair with eight patch rows, ec3d_kernels.hip): one 512-thread workgroup hosts two of the
// z-marching launch's workgroups -- "virtual" workgroups from here on -- whose patches are y-neighbours, so that the rows
// on either side of their common boundary travel through the LDS exchange instead of being requested as rim rows.
// Virtual workgroup v is what workgroup v of the unpaired launch is (walk_zm): XCD label v % 8, column
// (v % 8) * cpx + (v / 8) % cpx with cpx = tpp / 8, z segment (v / 8) / cpx; patch q of a plane lies at (q % npx, q / npx).
// The rule: 2-D tiles, an undivided handle (no z-slab, no rank driver), every XCD label's run of cpx columns made of
// whole patch rows and an even number of them (so no pair straddles two runs), nseg segments of pps planes each that
// cover the nplanes planes exactly (both halves of a pair march the same planes, and so do all pairs of a segment).
// A launch the rule refuses runs unpaired.
#if defined(__HIPCC__)
#define EC3D_PAIR_HD __host__ __device__
#else
#define EC3D_PAIR_HD
#endif
inline bool ec3d_patch_pairs_ok(int64_t tpp, int64_t npx, int64_t nplanes, int64_t pps, int64_t nblk, bool slab, bool dist)
{
    if (slab || dist || tpp <= 0 || npx <= 0 || pps <= 0 || nblk <= 0) return false;
    if (tpp % 8) return false; // the last XCD run would be short
    const int64_t cpx = tpp / 8;
    if (cpx % (2 * npx)) return false; // an odd number of patch rows in an XCD run, or a run that starts inside one
    if (nblk % tpp) return false;
    const int64_t nseg = nblk / tpp;
    return nseg * pps == nplanes; // segments of equal length, none empty
}
// The virtual workgroup that half `half` (0, 1) of physical workgroup `phys` hosts.  Physical workgroup phys keeps the XCD
// label phys % 8; within the label the pairs are numbered as their lower halves are among the unpaired workgroups
// (segment outermost, then patch row pair, then patch column), the upper half lying npx columns further on.
EC3D_PAIR_HD inline int ec3d_patch_pair_virtual(int tpp, int npx, int phys, int half)
{
    const int cpx = tpp >> 3, hc = cpx >> 1;
    const int c = phys & 7, sgp = phys >> 3;
    const int seg = sgp / hc, jj = sgp - seg * hc;
    const int pr = jj / npx, px = jj - pr * npx;
    return 8 * (seg * cpx + (2 * pr + half) * npx + px) + c;
}
// launch kinds that can pair (bits of Sweep::pair; bit k = kind k of ec3d_get_patch_rows): the bare SpMV, K2-in-K3 (S
// formed), K5-in-K1 (P formed), K4 in SpMV form without the X update, and the setup residual, K1 and K3
enum { EC3D_PAIR_SPMV = 1, EC3D_PAIR_K23 = 2, EC3D_PAIR_K51 = 4, EC3D_PAIR_K4S = 8, EC3D_PAIR_K13 = 16, EC3D_PAIR_ALL = 31 };
// the kinds that pair when nobody asks (vectors beyond the caches): those that won their A/B at 512^3, docs/rounds/r08.md
enum { EC3D_PAIR_DEFAULT_BIG = EC3D_PAIR_SPMV | EC3D_PAIR_K23 };
// K5-in-K1 forming AP_old inside the patch (Sweep::k51_ap): what an unset EC3D_K51_AP means from 32 Mi rows (docs/rounds/r09.md)
enum { EC3D_K51_AP_DEFAULT_BIG = 1 };

// z segments per column of a z-marching grid of `cols` columns that wants want_s workgroups, at most max_seg
inline int64_t ec3d_zm_segments(int64_t want_s, int64_t cols, int64_t max_seg, bool explicit_request)
{
    int64_t nseg = 1;
    if (explicit_request) {
        nseg = std::max<int64_t>(1, (want_s + cols / 2) / cols); // explicit request: nearest
    } else {
        const int64_t fit = want_s / cols; // most segments that still fit one round
        nseg = (fit >= 1 && 6 * cols * fit >= 5 * want_s) ? fit : (3 * want_s + 2 * cols - 1) / (2 * cols);
    }
    return std::min<int64_t>(nseg, max_seg);
}

// The U mask of the interleaved z-march (Sweep::il_umask): nw = ceil(P / 32) words per column, bit k of a column's words =
// a U tile is visited at plane k.  The one place that knows the layout.
inline uint32_t ec3d_il_bit(const uint32_t *um, int nw, int64_t col, int64_t k)
{
    return (um[(size_t)(col * nw + k / 32)] >> (k % 32)) & 1u;
}

// The mask from the list of U tiles (tile ids of the four stacked blocks of P planes of tpp tiles).  tile_flag (or
// null): per tile of the three A blocks, ntiles of them, whether it holds a coupled row.  False when a U tile lies
// outside the U block or a coupled A tile lies where no U tile is visited.
inline bool ec3d_il_umask(const std::vector<int32_t> &ulist, int64_t tpp, int64_t P, const uint8_t *tile_flag, int64_t ntiles,
                          std::vector<uint32_t> &um, int &nw)
{
    nw = (int)((P + 31) / 32);
    um.assign((size_t)(tpp * nw), 0u);
    for (int32_t t : ulist) {
        const int64_t k = (int64_t)t / tpp - 3 * P, col = (int64_t)t % tpp;
        if (k < 0 || k >= P) return false;
        um[(size_t)(col * nw + k / 32)] |= 1u << (k % 32);
    }
    // a coupled A tile must lie where a U tile is visited (its rows' cells carry U unknowns): checked, not assumed
    if (tile_flag)
        for (int64_t t = 0; t < ntiles; ++t)
            if (tile_flag[(size_t)t] && !ec3d_il_bit(um.data(), nw, t % tpp, (t / tpp) % P)) return false;
    return true;
}

// The work list of the interleaved z-march: four int32 per workgroup (column, first plane, end plane, 0), `per` rows
// of 8 workgroups (one per XCD label).  Two workgroups per CU are resident (a step holds the band operands of four
// tiles), all of them from the launch's start to its end, so the launch lasts as long as its heaviest workgroup:
// planes are dealt by weight -- a plane with a U tile (four tiles, the coupling slots of every row) counts il_w percent
// of one without -- column by column, the segments of a column of equal weight, the number of segments of a column in
// proportion to its weight.
inline void ec3d_il_work_list(const std::vector<uint32_t> &um, int nw, int64_t tpp, int64_t P, int64_t want_il, int il_w,
                              int64_t min_pps, std::vector<int32_t> &seg, size_t &per)
{
    const int64_t cpx = (tpp + 7) / 8;
    auto bit = [&](int64_t col, int64_t k) { return ec3d_il_bit(um.data(), nw, col, k); };
    std::vector<int64_t> wcol((size_t)tpp, 0);
    int64_t wtot = 0;
    for (int64_t col = 0; col < tpp; ++col) {
        for (int64_t k = 0; k < P; ++k) wcol[(size_t)col] += bit(col, k) ? il_w : 100;
        wtot += wcol[(size_t)col];
    }
    const double target = (double)wtot / (double)want_il;
    std::vector<std::vector<int32_t>> perx(8); // per XCD label: (col, k0, k1) triples in dispatch order
    int64_t max_seg = 0;
    std::vector<std::vector<std::array<int32_t, 2>>> cuts((size_t)tpp);
    for (int64_t col = 0; col < tpp; ++col) {
        int64_t ns = std::max<int64_t>(1, (int64_t)std::llround((double)wcol[(size_t)col] / target));
        ns = std::min<int64_t>(ns, std::max<int64_t>(1, P / min_pps));
        int64_t k0 = 0, acc = 0;
        for (int64_t sgi = 0; sgi < ns; ++sgi) {
            const int64_t goal = wcol[(size_t)col] * (sgi + 1) / ns;
            int64_t k1 = k0;
            while (k1 < P && (acc < goal || sgi + 1 == ns)) { acc += bit(col, k1) ? il_w : 100; ++k1; }
            cuts[(size_t)col].push_back({(int32_t)k0, (int32_t)k1});
            k0 = k1;
        }
        max_seg = std::max<int64_t>(max_seg, ns);
    }
    // dispatch order within an XCD: segment index outermost, so that the workgroups that start together work
    // on neighbouring columns at about the same planes (their +-sdx lines meet in that XCD's L2)
    for (int x = 0; x < 8; ++x)
        for (int64_t sgi = 0; sgi < max_seg; ++sgi)
            for (int64_t col = x * cpx; col < std::min<int64_t>((x + 1) * cpx, tpp); ++col)
                if (sgi < (int64_t)cuts[(size_t)col].size()) {
                    perx[(size_t)x].push_back((int32_t)col);
                    perx[(size_t)x].push_back(cuts[(size_t)col][(size_t)sgi][0]);
                    perx[(size_t)x].push_back(cuts[(size_t)col][(size_t)sgi][1]);
                }
    per = 0;
    for (int x = 0; x < 8; ++x) per = std::max(per, perx[(size_t)x].size() / 3);
    seg.assign(per * 8 * 4, 0);
    for (int x = 0; x < 8; ++x)
        for (size_t j = 0; j < perx[(size_t)x].size() / 3; ++j)
            for (int q = 0; q < 3; ++q) seg[(j * 8 + (size_t)x) * 4 + (size_t)q] = perx[(size_t)x][j * 3 + (size_t)q];
}

// The XCD-local order of a list of U tiles for a grid of G workgroups (G % 8 == 0): the tiles, sorted by column
// (tile % tpp), are cut into eight equal shares, one per XCD label; a share is taken plane by plane, consecutive tiles
// by consecutive workgroups of that XCD at the same time, so in-plane and plane-to-plane neighbours meet in that XCD's
// L2.  Entry j * G + i * 8 + x is tile j * (G / 8) + i of share x; holes (-1) end a workgroup's list (b, b + G, ...).
inline std::vector<int32_t> ec3d_xcd_local_order(const std::vector<int32_t> &tiles, int64_t tpp, int64_t G)
{
    const int64_t Gx = G / 8, L = (int64_t)tiles.size();
    std::vector<int32_t> byc(tiles);
    std::stable_sort(byc.begin(), byc.end(), [&](int32_t a, int32_t b) { return a % tpp < b % tpp; });
    int64_t K = 0;
    std::vector<std::vector<int32_t>> share(8);
    for (int x = 0; x < 8; ++x) {
        share[x].assign(byc.begin() + L * x / 8, byc.begin() + L * (x + 1) / 8);
        std::sort(share[x].begin(), share[x].end()); // tile id ascending = plane by plane, column by column
        K = std::max<int64_t>(K, ((int64_t)share[x].size() + Gx - 1) / Gx);
    }
    std::vector<int32_t> perm((size_t)(K * G), -1);
    for (int x = 0; x < 8; ++x)
        for (size_t i = 0; i < share[x].size(); ++i)
            perm[(size_t)(((int64_t)i / Gx) * G + ((int64_t)i % Gx) * 8 + x)] = share[x][i];
    return perm;
}

// z-slab of the structured form whose window is the npo owned planes from plane p0 of every block (blk tiles per
// block, tpp per plane), split H planes from each cut.  ui / ub: the U tiles of the interior / boundary planes, in the
// list's order.  bl, the boundary launch's list: the A tiles of planes 0, 1, npo-2, npo-1 of every block, plane by
// plane, then the U tiles there.  False (and no bl) when a U tile lies outside the owned window.
inline bool ec3d_slab_split_lists(const std::vector<int32_t> &ulist, int64_t tpp, int64_t blk, int64_t p0, int64_t npo, int64_t H,
                                  std::vector<int32_t> &ui, std::vector<int32_t> &ub, std::vector<int32_t> &bl)
{
    ui.clear();
    ub.clear();
    bl.clear();
    bool owned_only = true;
    for (int32_t t : ulist) {
        const int64_t pl = ((int64_t)t - 3 * blk) / tpp - p0; // owned plane of the U block this tile lies in
        if (t < 3 * blk || pl < 0 || pl >= npo) owned_only = false;
        else if (pl >= H && pl < npo - H) ui.push_back(t);
        else ub.push_back(t);
    }
    if (!owned_only) return false;
    for (int d = 0; d < 3; ++d)
        for (int64_t pl : {(int64_t)0, (int64_t)1, npo - 2, npo - 1})
            for (int64_t q = 0; q < tpp; ++q) bl.push_back((int32_t)(d * blk + (p0 + pl) * tpp + q));
    bl.insert(bl.end(), ub.begin(), ub.end());
    return true;
}
