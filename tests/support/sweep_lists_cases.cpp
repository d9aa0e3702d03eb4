// Stand-alone host program of tests/test_sweep_lists_host.py: runs the list builders of csrc/ec3d_sweep_lists.hpp on
// the smallest shapes at which they can go wrong and prints, per case, what it gave them and what came back:
//   case KIND NAME
//   KEY v v v ...        one line per input and per output list, integers (doubles as %a)
// KIND is xcd, il, ilgrid, slab, patch, shape or zm.  Built with the address and undefined-behaviour sanitizers.
#include "../../eddy_currents_3d_amd/csrc/ec3d_sweep_lists.hpp"

#include <cstdio>
#include <string>

namespace {

template <class T> void line(const char *key, const std::vector<T> &v)
{
    std::printf("%s", key);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
void line(const char *key, std::initializer_list<long long> v) { line(key, std::vector<long long>(v)); }

uint32_t lcg_state = 12345u;
uint32_t lcg() { return (lcg_state = lcg_state * 1664525u + 1013904223u) >> 8; }

// L distinct U tiles of a block of 48 planes of tpp tiles behind three A blocks; ascending, or in the order drawn
void xcd_case(int tpp, int G, int L, bool ascending)
{
    const int planes = 48;
    std::vector<int32_t> pool, tiles;
    for (int t = 0; t < planes * tpp; ++t) pool.push_back((int32_t)(3 * planes * tpp + t));
    for (int i = 0; i < L; ++i) {
        const size_t j = (size_t)i + lcg() % (pool.size() - (size_t)i);
        std::swap(pool[(size_t)i], pool[j]);
        tiles.push_back(pool[(size_t)i]);
    }
    if (ascending) std::sort(tiles.begin(), tiles.end());
    std::printf("case xcd tpp%d_G%d_L%d_%s\n", tpp, G, L, ascending ? "asc" : "drawn");
    line("in", {tpp, G});
    line("tiles", tiles);
    line("perm", ec3d_xcd_local_order(tiles, tpp, G));
}

enum Mask { NONE, ALL, ONE_COLUMN, CHECKER };
bool masked(Mask m, int tpp, int col, int k)
{
    return m == ALL || (m == ONE_COLUMN && col == tpp / 2) || (m == CHECKER && ((col + k) & 1));
}

// what ec3d_il_umask and ec3d_il_work_list make of a list of U tiles (tile_flag given to the builder when flags != 0)
void il_lists(const char *kind, const std::string &name, int tpp, int P, int want_il, int flags, const std::vector<int32_t> &ulist,
              const std::vector<uint8_t> &tf)
{
    std::printf("case %s %s\n", kind, name.c_str());
    const int il_w = 160, min_pps = 2;
    line("in", {tpp, P, want_il, il_w, min_pps, flags});
    line("ulist", ulist);
    line("tile_flag", tf);
    std::vector<uint32_t> um;
    int nw = -1;
    const bool ok = ec3d_il_umask(ulist, tpp, P, flags ? tf.data() : nullptr, (int64_t)tf.size(), um, nw);
    line("ok", {ok, nw});
    if (!ok) return;
    line("um", um);
    std::vector<int32_t> bits;
    for (int col = 0; col < tpp; ++col)
        for (int k = 0; k < P; ++k) bits.push_back((int32_t)ec3d_il_bit(um.data(), nw, col, k));
    line("bits", bits);
    std::vector<int32_t> seg;
    size_t per = 0;
    ec3d_il_work_list(um, nw, tpp, P, want_il, il_w, min_pps, seg, per);
    line("per", {(long long)per});
    line("seg", seg);
}

// flags: 0 no tile_flag; 1 the A_y tile coupled wherever a U tile is; 2 as 1 and one coupled A_z tile where no U tile
// is; ustray: a tile appended to the list of U tiles (-1: none)
void il_case(const std::string &name, int tpp, int P, int want_il, Mask m, int flags, int32_t ustray = -1)
{
    std::vector<int32_t> ulist;
    std::vector<uint8_t> tf((size_t)(3 * P * tpp), 0);
    for (int k = 0; k < P; ++k)
        for (int col = 0; col < tpp; ++col)
            if (masked(m, tpp, col, k)) {
                ulist.push_back((int32_t)((3 * P + k) * tpp + col));
                tf[(size_t)((P + k) * tpp + col)] = 1;
            }
    if (flags == 2)
        for (int t = 2 * P * tpp; t < 3 * P * tpp; ++t)
            if (!tf[(size_t)(t - P * tpp)]) { tf[(size_t)t] = 1; break; }
    if (ustray >= 0) ulist.push_back(ustray);
    il_lists("il", name, tpp, P, want_il, flags, ulist, tf);
}

// The masks of grids whose plane is SEVERAL tiles (tests/av_grids.py holds the same boxes as voxels): conductor boxes
// [a, b) per axis in a grid of sdx x sdy x P cells whose planes are `pitch` rows apart; the U tile of (column, plane) is
// listed when one of its 512 rows is a conducting cell, and the three A tiles there are coupled.
struct Box { int x0, x1, y0, y1, z0, z1; };
void il_grid_case(const char *name, int sdx, int sdy, int P, int pitch, int want_il, const std::vector<Box> &boxes,
                  const std::vector<Box> &holes)
{
    const int tpp = pitch / 512;
    auto in = [](const Box &b, int x, int y, int z) { return x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1 && z >= b.z0 && z < b.z1; };
    std::vector<uint8_t> u((size_t)(P * tpp), 0);
    for (int z = 0; z < P; ++z)
        for (int y = 0; y < sdy; ++y)
            for (int x = 0; x < sdx; ++x) {
                bool on = false;
                for (const Box &b : boxes) on = on || in(b, x, y, z);
                for (const Box &h : holes) on = on && !in(h, x, y, z);
                if (on) u[(size_t)(z * tpp + (y * sdx + x) / 512)] = 1;
            }
    std::vector<int32_t> ulist;
    std::vector<uint8_t> tf((size_t)(3 * P * tpp), 0);
    for (int t = 0; t < P * tpp; ++t)
        if (u[(size_t)t]) {
            ulist.push_back((int32_t)(3 * P * tpp + t));
            for (int d = 0; d < 3; ++d) tf[(size_t)(d * P * tpp + t)] = 1;
        }
    il_lists("ilgrid", name, tpp, P, want_il, 1, ulist, tf);
    line("grid", {sdx, sdy, pitch});
}

// U tiles at (plane, column) pairs of the U block of a slab whose blocks hold p0 + npo + 3 planes of 3 tiles
void slab_case(const char *name, int p0, int npo, std::vector<std::array<int, 2>> at)
{
    const int64_t tpp = 3, H = 2, blk = (p0 + npo + 3) * tpp;
    std::vector<int32_t> ulist, ui, ub, bl;
    for (auto a : at) ulist.push_back((int32_t)(3 * blk + a[0] * tpp + a[1]));
    std::printf("case slab %s\n", name);
    line("in", {tpp, blk, p0, npo, H});
    line("ulist", ulist);
    const bool owned_only = ec3d_slab_split_lists(ulist, tpp, blk, p0, npo, H, ui, ub, bl);
    line("owned_only", {owned_only});
    line("ui", ui);
    line("ub", ub);
    line("bl", bl);
}

// a 16 x 6 plane in rows of pitch 128, two planes per block; classes: 0, 1 uncoupled A, 2, 3 coupled A, 4, 5 U with an
// unknown, 6 zero.  The padding rows of a plane hold classes that would count if they were read.
void patch_case(const char *name, int px, int py, bool marks)
{
    const int64_t sdx = 16, sdy = 6, pitch = 128, planes = 2;
    std::vector<uint8_t> cls((size_t)(4 * planes * pitch), 0);
    for (int64_t P = 0; P < 4 * planes; ++P)
        for (int64_t r = 0; r < pitch; ++r)
            cls[(size_t)(P * pitch + r)] = (uint8_t)(r >= sdx * sdy ? (P < 3 * planes ? 3 : 4) : P < 3 * planes ? (int)(r % 2) : 6);
    if (marks) {
        cls[(size_t)((1 * planes + 1) * pitch + 2 * sdx + 9)] = 2;  // A_y, plane 1, cell (9, 2): coupled
        cls[(size_t)((3 * planes + 0) * pitch + 5 * sdx + 3)] = 5;  // U, plane 0, cell (3, 5): in the short patch row
        cls[(size_t)((3 * planes + 1) * pitch + 0 * sdx + 15)] = 4; // U, plane 1, cell (15, 0)
    }
    std::vector<uint8_t> flag;
    std::vector<int32_t> ulist;
    ec3d_patch_tables(cls.data(), planes, pitch, sdx, sdy, px, py, 2, 4, 6, flag, ulist);
    std::printf("case patch %s\n", name);
    line("in", {planes, pitch, sdx, sdy, px, py, 2, 4, 6});
    line("cls", cls);
    line("flag", flag);
    line("ulist", ulist);
}

} // namespace

int main()
{
    int n = 0;
    for (int tpp : {1, 3, 8, 9})
        for (int G : {8, 16, 40})
            for (int L : {1, 7, 8, 9, 41}) xcd_case(tpp, G, L, n++ % 2 == 0);
    const char *mask_name[] = {"none", "all", "onecol", "checker"};
    for (int tpp : {1, 5, 8, 9})
        for (int P : {2, 3, 31, 32, 33, 65})
            for (int want_il : {8, 40, 512})
                for (Mask m : {NONE, ALL, ONE_COLUMN, CHECKER})
                    il_case("tpp" + std::to_string(tpp) + "_P" + std::to_string(P) + "_w" + std::to_string(want_il) + "_" +
                                mask_name[m], tpp, P, want_il, m, m == ALL ? 0 : 1);
    il_case("coupled_without_u", 5, 33, 40, CHECKER, 2);
    il_case("u_tile_in_az", 5, 33, 40, ONE_COLUMN, 1, (3 * 33 - 1) * 5 + 2);
    il_case("u_tile_behind_the_block", 5, 33, 40, ONE_COLUMN, 1, 4 * 33 * 5);
    // 64 x 72 x 40: 9 columns, two domains with four planes of air between them, a through hole, nothing in column 0
    il_grid_case("S1", 64, 72, 40, 4608, 16, {{9, 52, 10, 60, 3, 14}, {20, 60, 18, 66, 18, 37}}, {{28, 36, 30, 38, 3, 14}});
    il_grid_case("S1_one_block", 64, 72, 40, 4608, 16, {{9, 60, 10, 60, 3, 37}}, {});     // columns 0 and 8 empty
    il_grid_case("S2", 1024, 8, 34, 8192, 40, {{400, 640, 2, 6, 3, 31}}, {});            // 16 columns of half a grid row
    il_grid_case("S3", 40, 30, 33, 1536, 8, {{5, 34, 4, 26, 3, 30}}, {});                // 1200 cells in 1536 rows
    for (int p0 : {0, 3})
        for (int npo : {6, 7}) {
            std::vector<std::array<int, 2>> at;
            for (int pl = 0; pl < npo; ++pl)
                for (int col = 0; col < 3; ++col)
                    if ((pl + col) % 3 != 1) at.push_back({p0 + pl, col});
            slab_case(("p" + std::to_string(p0) + "_n" + std::to_string(npo)).c_str(), p0, npo, at);
        }
    slab_case("above_the_window", 3, 6, {{3, 0}, {5, 1}, {9, 2}});
    slab_case("below_the_window", 3, 6, {{2, 2}, {5, 1}});
    slab_case("in_an_a_block", 0, 7, {{-1, 2}, {3, 1}});
    patch_case("marks_8x4", 8, 4, true);
    patch_case("empty_8x4", 8, 4, false);
    patch_case("marks_4x4", 4, 4, true);
    const int shapes[][2] = {{16, 15}, {18, 16}, {102, 102}, {256, 256}, {15, 16}, {101, 102}};
    for (auto &s : shapes) {
        int px = -1, py = -1;
        const double eff = ec3d_pick_patch_shape(s[0], s[1], 512, px, py);
        std::printf("case shape %dx%d\nin %d %d\nout %d %d\neff %a\n", s[0], s[1], s[0], s[1], px, py, eff);
    }
    for (int explicit_request : {0, 1})
        for (int cols : {8, 520})
            for (int want_s : {768, 1024, 1536})
                for (int max_seg : {1000, 2}) {
                    std::printf("case zm e%d_c%d_w%d_m%d\n", explicit_request, cols, want_s, max_seg);
                    line("in", {want_s, cols, max_seg, explicit_request});
                    line("nseg", {(long long)ec3d_zm_segments(want_s, cols, max_seg, explicit_request != 0)});
                }
    return 0;
}
