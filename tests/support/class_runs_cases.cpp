// Stand-alone host program of tests/test_class_runs_host.py: runs ec3d_class_runs / ec3d_class_runs_shape of
// csrc/ec3d_sweep_lists.hpp and prints, per case, what it gave them and what came back:
//   case KIND NAME
//   KEY v v v ...        one line per input and per output list, integers
// KIND is runs or shape.  Built with the address and undefined-behaviour sanitizers.
#include "../../eddy_currents_3d_amd/csrc/ec3d_sweep_lists.hpp"

#include <cstdio>
#include <functional>
#include <string>

namespace {

template <class T> void line(const char *key, const std::vector<T> &v)
{
    std::printf("%s", key);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
void line(const char *key, std::initializer_list<long long> v) { line(key, std::vector<long long>(v)); }

uint32_t lcg_state = 2463534242u;
uint32_t lcg() { return (lcg_state = lcg_state * 1664525u + 1013904223u) >> 8; }

// a grid of sdx x sdy cells per plane, the plane padded to sdy_pad rows (kdz = sdx * sdy_pad), `planes` planes of random
// class bytes drawn plane by plane; `edit` then changes the array
void runs_case(const std::string &name, int sdx, int sdy, int sdy_pad, int planes, int px, int py, bool equal_planes,
               const std::function<void(std::vector<uint8_t> &, int64_t kdz)> &edit)
{
    const int64_t kdz = (int64_t)sdx * sdy_pad;
    std::vector<uint8_t> cls((size_t)(kdz * planes));
    for (int64_t i = 0; i < kdz; ++i) cls[(size_t)i] = (uint8_t)(lcg() % 29);
    for (int k = 1; k < planes; ++k)
        for (int64_t i = 0; i < kdz; ++i)
            cls[(size_t)(k * kdz + i)] = equal_planes ? cls[(size_t)i] : (uint8_t)(lcg() % 29);
    edit(cls, kdz);
    std::vector<uint8_t> flag;
    ec3d_class_runs(cls.data(), planes, kdz, sdx, px, py, flag);
    std::printf("case runs %s\n", name.c_str());
    line("in", {sdx, sdy, sdy_pad, planes, px, py});
    line("cls", cls);
    line("flag", flag);
}

void shape_case(const std::string &name, std::vector<int64_t> off, int64_t n, int px, int py)
{
    int64_t planes = -1, tpp = -1;
    const bool ok = ec3d_class_runs_shape((int)off.size(), off.data(), n, px, py, planes, tpp);
    std::printf("case shape %s\n", name.c_str());
    line("off", off);
    line("in", {(long long)n, px, py});
    line("out", {ok ? 1 : 0, (long long)planes, (long long)tpp});
}

std::vector<int64_t> seven(int64_t sdx, int64_t kdz) { return {-kdz, -sdx, -1, 0, 1, sdx, kdz}; }

} // namespace

int main()
{
    const auto nothing = [](std::vector<uint8_t> &, int64_t) {};
    for (int shape = 0; shape < 2; ++shape) {
        // a small patch shape (8 x 2, 2 x 3 patches per plane) and the kernels' own (128 x 4 on 256 x 8: 2 x 2 patches)
        const int sdx = shape ? 256 : 16, sdy = shape ? 7 : 5, pad = shape ? 8 : 6, px = shape ? 128 : 8, py = shape ? 4 : 2;
        const std::string s = shape ? "_128x4" : "_8x2";
        runs_case("all_equal" + s, sdx, sdy, pad, 5, px, py, true, nothing);
        runs_case("all_different" + s, sdx, sdy, pad, 5, px, py, false, nothing);
        // plane 2, cell (px + 1, py) -- patch (1, 1): tile (1, 1) of planes 2 and 3 differs from the one below
        runs_case("one_cell" + s, sdx, sdy, pad, 5, px, py, true, [&](std::vector<uint8_t> &c, int64_t kdz) {
            c[(size_t)(2 * kdz + py * sdx + px + 1)] ^= 0x40;
        });
        // the last cell of a patch's last row, and the first of its first
        runs_case("patch_corners" + s, sdx, sdy, pad, 6, px, py, true, [&](std::vector<uint8_t> &c, int64_t kdz) {
            c[(size_t)(1 * kdz + (py - 1) * sdx + px - 1)] ^= 0x40;
            c[(size_t)(4 * kdz + py * sdx + px)] ^= 0x40;
        });
        // a padded row (y = sdy .. pad-1 holds no cell of the grid): it counts like any other
        runs_case("padded_row" + s, sdx, sdy, pad, 4, px, py, true, [&](std::vector<uint8_t> &c, int64_t kdz) {
            c[(size_t)(3 * kdz + (pad - 1) * sdx + 3)] ^= 0x40;
        });
        runs_case("last_plane" + s, sdx, sdy, pad, 4, px, py, true, [&](std::vector<uint8_t> &c, int64_t kdz) {
            c[(size_t)(3 * kdz + 2)] ^= 0x40;
        });
        runs_case("single_plane" + s, sdx, sdy, pad, 1, px, py, true, nothing);
        runs_case("two_planes_equal" + s, sdx, sdy, pad, 2, px, py, true, nothing);
        runs_case("two_planes_different" + s, sdx, sdy, pad, 2, px, py, false, nothing);
    }
    shape_case("cube", seven(256, 256 * 8), 256 * 8 * 9, 128, 4);
    shape_case("one_plane", seven(128, 128 * 4), 128 * 4, 128, 4);
    shape_case("narrow_rows", seven(64, 64 * 8), 64 * 8 * 9, 128, 4);
    shape_case("rows_not_px", seven(192, 192 * 8), 192 * 8 * 9, 128, 4);
    shape_case("rows_per_plane_not_py", seven(128, 128 * 6), 128 * 6 * 9, 128, 4);
    shape_case("plane_not_rows", seven(128, 128 * 4 + 64), (128 * 4 + 64) * 8, 128, 4);
    shape_case("part_of_a_plane", seven(128, 128 * 4), 128 * 4 * 5 + 256, 128, 4);
    shape_case("no_rows", seven(128, 128 * 4), 0, 128, 4);
    shape_case("five_bands", {-512, -128, 0, 128, 512}, 512 * 5, 128, 4);
    return 0;
}
