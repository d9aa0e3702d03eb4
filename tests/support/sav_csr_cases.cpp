// Stand-alone host program of tests/test_av_csr_host.py: the A-V recogniser (csrc/ec3d_sav_csr.cpp) on CSR matrices the
// test wrote to a file, under the address and undefined-behaviour sanitizers.  Usage: sav_csr_cases FILE.  The file
// holds, per case (native byte order):
//   int64 n, nnz, nslice;  int32 irow[n + 1], jcol[nnz];  double valA[nnz];  nslice x int64 {ranks, rank, e0, e1, k0, k1}
// For every case it prints one line
//   case I structured S classes C pitch P cut R R ...      (R: the rank counts among the slices that can be cut)
// after it has checked, when the matrix was recognised,
//   * that the class-coded form, expanded back to CSR by the form's DEFINITION (header comment of ec3d_sav_csr.cpp and
//     of ec3d_internal.hpp's MatView: slot -> device offset -> reference unknown through cond_cell and the pitch; A rows
//     are slots 0..6 then 7..11, U rows slots 7..15 then 0..6; the all-zero class marks padding), equals the input entry
//     for entry and bit for bit, explicit zeros removed from the input (the form cannot hold them);
//   * that every slice (ec3d_sav_slice) holds the global class bytes on its owned planes, the zero class on halo planes
//     and padding, cond_cell as one contiguous run of the global list from u_first, and a ulist naming exactly the tiles
//     behind the three A blocks that hold a coupled or U class.
// A failed check prints "FAIL ..." and makes the exit status 1.
#include "../../eddy_currents_3d_amd/csrc/ec3d_sav_csr.cpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>

namespace {

int failures = 0;
int case_no = 0;

void fail(const char *what, long long a = 0, long long b = 0)
{
    std::printf("FAIL case %d: %s (%lld, %lld)\n", case_no, what, a, b);
    ++failures;
}

template <class T> bool read_n(FILE *f, std::vector<T> &v, size_t k)
{
    v.resize(k);
    return k == 0 || std::fread(v.data(), sizeof(T), k, f) == k;
}

uint64_t bits(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

// reference unknown of every device row (-1: none), from the dimensions, the pitch and cond_cell alone
std::vector<int64_t> ref_of_dev(const SavHost &S, int64_t n)
{
    const int64_t sdz = S.nCd / S.pitch, nC = S.plane * sdz;
    std::vector<int64_t> ref((size_t)S.n_pad, -1);
    for (int d = 0; d < 3; ++d)
        for (int64_t k = 0; k < sdz; ++k)
            for (int64_t c = 0; c < S.plane; ++c) ref[(size_t)(d * S.nCd + k * S.pitch + c)] = d * nC + k * S.plane + c;
    for (size_t m = 0; m < S.cond_cell.size(); ++m) {
        const int64_t cell = S.cond_cell[m];
        if (cell < 0 || cell >= S.nCd || cell % S.pitch >= S.plane) {
            fail("cond_cell outside the grid", (long long)m, cell);
            continue;
        }
        if (ref[(size_t)(3 * S.nCd + cell)] != -1) fail("cond_cell names a cell twice", (long long)m, cell);
        ref[(size_t)(3 * S.nCd + cell)] = 3 * nC + (int64_t)m;
    }
    if (3 * nC + (int64_t)S.cond_cell.size() != n) fail("3 nC + nU != n", 3 * nC, n);
    return ref;
}

void check_expansion(const SavHost &S, int64_t n, const std::vector<double> &valA, const std::vector<int32_t> &irow,
                     const std::vector<int32_t> &jcol)
{
    if (S.n_ref != n || S.n_dev != 4 * S.nCd || S.n_pad % EC3D_TILE || S.n_pad < S.n_dev || S.n_pad - S.n_dev >= EC3D_TILE ||
        (int64_t)S.cls.size() != S.n_pad || (int64_t)S.table.size() != (int64_t)S.ncls * 16 || S.zero != S.ncls - 1 ||
        !(0 <= S.a0 && S.a0 <= S.u0 && S.u0 <= S.zero) || S.nCd % S.pitch || S.plane % S.sdx || S.pitch < S.plane) {
        fail("inconsistent sizes");
        return;
    }
    for (int s = 0; s < 16; ++s)
        if (bits(S.table[(size_t)S.zero * 16 + s]) != 0) fail("the zero class holds a coefficient", s);
    const std::vector<int64_t> ref = ref_of_dev(S, n);
    std::vector<int64_t> dev((size_t)n, -1);
    for (int64_t r = 0; r < S.n_pad; ++r)
        if (ref[(size_t)r] >= 0 && ref[(size_t)r] < n) dev[(size_t)ref[(size_t)r]] = r;
    const int64_t boff[7] = {-S.pitch, -S.sdx, -1, 0, 1, S.sdx, S.pitch}, step[3] = {1, S.sdx, S.pitch};
    const int order_a[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    const int order_u[16] = {7, 8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6};
    for (int64_t r = 0; r < S.n_pad; ++r) {
        const int c = S.cls[(size_t)r];
        if (c >= S.ncls) {
            fail("class byte out of range", r, c);
            return;
        }
        if (ref[(size_t)r] < 0) {
            if (c != S.zero) fail("a row without an unknown has a class other than zero", r, c);
            continue;
        }
        const int64_t rr = ref[(size_t)r];
        const bool urow = r >= 3 * S.nCd;
        const int d = (int)(r / S.nCd);
        if (c != S.zero && (urow != (c >= S.u0))) fail("class kind does not match the row's block", r, c);
        const double *t = &S.table[(size_t)c * 16];
        if (!urow)
            for (int s = 12; s < 16; ++s)
                if (t[s] != 0.0) fail("an A row holds a slot above 11", r, s);
        int64_t p = irow[(size_t)rr] - 1;
        const int64_t p1 = irow[(size_t)rr + 1] - 1;
        const int nslot = urow ? 16 : 12;
        for (int i = 0; i < nslot; ++i) {
            const int s = urow ? order_u[i] : order_a[i];
            if (t[s] == 0.0) continue;
            int64_t dc;
            if (s < 7) dc = r + boff[s];
            else if (!urow) dc = r + (3 - d) * S.nCd + (s - 9) * step[d];
            else dc = r - (3 - (s - 7) / 3) * S.nCd + ((s - 7) % 3 - 1) * step[(s - 7) / 3];
            if (dc < 0 || dc >= S.n_pad || ref[(size_t)dc] < 0) {
                fail("a slot points at a row without an unknown", r, s);
                continue;
            }
            while (p < p1 && valA[(size_t)p] == 0.0) ++p; // explicit zeros: not held
            if (p == p1) {
                fail("the form holds an entry the input does not", rr, s);
                break;
            }
            if ((int64_t)jcol[(size_t)p] - 1 != ref[(size_t)dc] || bits(valA[(size_t)p]) != bits(t[s]))
                fail("entry differs (row, slot)", rr, s);
            ++p;
        }
        while (p < p1 && valA[(size_t)p] == 0.0) ++p;
        if (p != p1) fail("the input holds an entry the form does not", rr, p);
    }
    for (int64_t rr = 0; rr < n; ++rr)
        if (dev[(size_t)rr] < 0) fail("an unknown without a device row", rr);
}

// tile_flag and ulist of a form, global or slice, against its class bytes
void check_tiles(const SavHost &S, const char *what)
{
    const int64_t nt = S.n_pad / EC3D_TILE;
    if ((int64_t)S.tile_flag.size() != nt || S.ntiles_front != (3 * S.nCd + EC3D_TILE - 1) / EC3D_TILE) {
        fail(what, -1, -1);
        return;
    }
    std::vector<int32_t> want;
    for (int64_t t = 0; t < nt; ++t) {
        bool any = false;
        for (int64_t r = t * EC3D_TILE; r < (t + 1) * EC3D_TILE; ++r) any = any || (S.cls[(size_t)r] >= S.a0 && S.cls[(size_t)r] < S.zero);
        if ((S.tile_flag[(size_t)t] != 0) != any) fail(what, t, any);
        if (any && t >= S.ntiles_front) want.push_back((int32_t)t);
    }
    if (want != S.ulist) fail(what, (long long)want.size(), (long long)S.ulist.size());
}

void check_slice(const SavHost &G, int64_t e0, int64_t e1, int64_t k0, int64_t k1)
{
    SavHost L;
    ec3d_sav_slice(G, e0, e1, k0, k1, L);
    const int64_t pitch = G.pitch, np = e1 - e0, nCd = np * pitch;
    if (L.pitch != pitch || L.plane != G.plane || L.sdx != G.sdx || L.nCd != nCd || L.n_dev != 4 * nCd || L.n_pad % EC3D_TILE ||
        L.n_pad < L.n_dev || L.n_pad - L.n_dev >= EC3D_TILE || (int64_t)L.cls.size() != L.n_pad || L.a0 != G.a0 || L.u0 != G.u0 ||
        L.zero != G.zero || L.ncls != G.ncls || L.table != G.table || L.halo != pitch || L.nown != 4) {
        fail("slice: inconsistent sizes", e0, e1);
        return;
    }
    for (int64_t r = 0; r < L.n_pad; ++r) {
        int want = G.zero;
        if (r < L.n_dev) {
            const int64_t d = r / nCd, p = r % nCd / pitch + e0, c = r % pitch;
            if (p >= k0 && p < k1) want = G.cls[(size_t)(d * G.nCd + p * pitch + c)];
        }
        if (L.cls[(size_t)r] != want) {
            fail("slice: class byte", r, want);
            break;
        }
    }
    for (int d = 0; d < 4; ++d)
        if (L.own_lo[d] != d * nCd + (k0 - e0) * pitch || L.own_hi[d] != d * nCd + (k1 - e0) * pitch) fail("slice: owned rows", d);
    // held conducting cells: the global list's members in planes [e0, e1), which must be consecutive
    int64_t first = -1, last = -1, cnt = 0;
    for (size_t m = 0; m < G.cond_cell.size(); ++m) {
        const int64_t pl = G.cond_cell[m] / pitch;
        if (pl < e0 || pl >= e1) continue;
        if (first < 0) first = (int64_t)m;
        last = (int64_t)m;
        ++cnt;
    }
    if (cnt && last - first + 1 != cnt) fail("slice: held unknowns are not one run", first, last);
    if ((int64_t)L.cond_cell.size() != cnt || (cnt && L.u_first != first)) fail("slice: u_first / count", L.u_first, cnt);
    else
        for (int64_t i = 0; i < cnt; ++i)
            if (L.cond_cell[(size_t)i] + e0 * pitch != G.cond_cell[(size_t)(first + i)]) {
                fail("slice: cond_cell", i, L.cond_cell[(size_t)i]);
                break;
            }
    if (L.n_ref != 3 * np * G.plane + cnt) fail("slice: n_ref", L.n_ref);
    check_tiles(L, "slice: tile_flag / ulist");
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[3];
    while (std::fread(head, sizeof(int64_t), 3, f) == 3) {
        const int64_t n = head[0], nnz = head[1], nslice = head[2];
        std::vector<int32_t> irow, jcol;
        std::vector<double> valA;
        std::vector<int64_t> slices;
        if (!read_n(f, irow, (size_t)n + 1) || !read_n(f, jcol, (size_t)nnz) || !read_n(f, valA, (size_t)nnz) ||
            !read_n(f, slices, (size_t)nslice * 6)) {
            std::fclose(f);
            return 2;
        }
        SavHost S;
        const int rc = ec3d_csr_to_sav_host(n, valA.data(), irow.data(), jcol.data(), S);
        std::printf("case %d structured %d classes %d pitch %lld cut", case_no, rc == 0, rc == 0 ? S.ncls : 0,
                    rc == 0 ? (long long)S.pitch : 0LL);
        std::vector<int64_t> cut;
        if (rc == 0) {
            int64_t asked = 0;
            for (int64_t i = 0; i < nslice; ++i) {
                const int64_t *s = &slices[(size_t)i * 6];
                std::string why;
                if (s[0] != asked && ec3d_sav_cuttable(S, (int)s[0], why) == 0) cut.push_back(s[0]);
                asked = s[0];
            }
            for (int64_t r : cut) std::printf(" %lld", (long long)r);
        }
        std::printf("\n");
        if (rc == 0) {
            check_expansion(S, n, valA, irow, jcol);
            check_tiles(S, "tile_flag / ulist");
            for (int64_t i = 0; i < nslice; ++i) {
                const int64_t *s = &slices[(size_t)i * 6];
                if (std::find(cut.begin(), cut.end(), s[0]) != cut.end()) check_slice(S, s[2], s[3], s[4], s[5]);
            }
        }
        ++case_no;
    }
    std::fclose(f);
    std::printf("done %d\n", case_no);
    return failures ? 1 : 0;
}
