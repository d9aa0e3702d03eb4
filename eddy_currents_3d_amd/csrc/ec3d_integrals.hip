// ec3d_integrals.hip — integrals of the resident fields, on the device: per-domain Joule loss and Lorentz force
// (ec3d_domain_integrals), the magnetic energy of the box (ec3d_field_energy) and the flux linkage of every
// non-conducting domain (ec3d_domain_linkage).
//
// The integrals of the very fields field_N.vtk shows (k_vtk_fields, ec3d_output.hip; writeVtk_field,
// src/utilites.f90:238-289) BEFORE their rounding to float32:
//   J = s * Jaf, s = -0.07957747154594766788444d7 (= -1/mu0; valPHYS(:,2) is mu0*sigma)
//   B = curl A, central differences clamped at the box faces
//   q = Jx*Jx + Jy*Jy + Jz*Jz,   f = J x B,   a = (Ax*Jx + Ay*Jy) + Az*Jz
// per conducting domain d: joule_w = (dx*dy*dz) * sum(q) / sigma_d,  force_n = (dx*dy*dz) * sum(f).  Not a Maxwell-stress
// evaluation.  Per non-conducting domain: linkage = (dx*dy*dz) * sum(a), jsum = (dx*dy*dz) * sum(J).  Over the box:
// energy_b = (dx*dy*dz) * (0.5 * 0.07957747154594766788444d7) * sum(Bx*Bx + By*By + Bz*Bz), each axis summed on its own.
//
// Lists (the per-domain calls).  The cells' device indices sorted by (domain id, scan order), 4 B per cell, cut into chunks
// of EC3D_DOM_CHUNK entries that never straddle a domain (a domain's last chunk may be short); `chunk` holds (first entry,
// entries, domain ordinal) per chunk and `dom_chunk` the first chunk of every domain.  The order is a property of the
// geometry, not of the storage: the structured form and bands + tail sum the same values in the same order.  The conducting
// domains' lists go to the device at assembly; the non-conducting domains' stay on the host until the first
// ec3d_domain_linkage.
//
// Summation chain of a list (ec3d_stream.hpp's: the result is a pure function of X, B and the geometry).  A value of
// sums[d] is reached through, at most,
//   k_dom_partials   3 additions of a thread's own 4 entries (stride 256), 6 levels of the wave's shuffle tree, 4 wave sums
//   k_dom_final      ceil(chunks_d / 256) - 1 additions of a thread's own partials (stride 256), 6 levels, 4 wave sums
// i.e. 13 + ceil(n_d / 262144) + 9 dependent additions for a domain of n_d cells: 61 at 10 M cells, and below 2100 for any
// list whose device rows fit the library's int32 row index (4 nCd < 2^31).
//
// The streaming pass (ec3d_field_energy; a streaming launch of ec3d_stream.hpp over cells instead of rows).  Every xy
// plane is cut into ceil(sdx*sdy / EC3D_TILE) chunks of EC3D_TILE cells -- of the plane, not of the device rows, so both
// storage forms and every plane pitch cut alike --; thread t takes the cells 2t and 2t + 1 of a chunk, cell 2t first.  Cells
// past the plane's end are never loaded and add nothing.  k_energy_collapse, one workgroup, collapses the partials.
// tests/field_integrals_numpy.py restates both chains.
#include "ec3d_stream.hpp"

#include <algorithm>

#define EC3D_DOM_CHUNK 1024 /* list entries per workgroup of k_dom_partials: 4 per thread */
#define EC3D_ENERGY_NV 5     /* sums of the streaming pass: Bx^2, By^2, Bz^2, A.J outside the conductors, A.J inside */

namespace {

typedef stream_d2 d2;

struct Grid {
    int sdx, sdy, sdz;
    int64_t pitch, nCd; // device rows per xy plane and per component block
    double dx, dy, dz;
};

// the four terms of a conductor cell: q, fx, fy, fz
struct JouleForce {
    static __device__ __forceinline__ void add(double (&v)[4], const Grid &g, int64_t pm, const double *__restrict__ U,
                                               const double *__restrict__ J)
    {
        const double s = -0.07957747154594766788444e7;
        const int64_t q = pm % g.pitch, nCd = g.nCd;
        const int i = (int)(q % g.sdx) + 1, j = (int)(q / g.sdx) + 1, k = (int)(pm / g.pitch) + 1;
        const double jx = s * J[pm], jy = s * J[nCd + pm], jz = s * J[2 * nCd + pm];
        const int64_t nim = i == 1 ? pm : pm - 1, nip = i == g.sdx ? pm : pm + 1;
        const int64_t njm = j == 1 ? pm : pm - g.sdx, njp = j == g.sdy ? pm : pm + g.sdx;
        const int64_t nkm = k == 1 ? pm : pm - g.pitch, nkp = k == g.sdz ? pm : pm + g.pitch;
        const double bx = 0.5 * (U[2 * nCd + njp] - U[2 * nCd + njm]) / g.dy - 0.5 * (U[nCd + nkp] - U[nCd + nkm]) / g.dz;
        const double by = 0.5 * (U[nkp] - U[nkm]) / g.dz - 0.5 * (U[2 * nCd + nip] - U[2 * nCd + nim]) / g.dx;
        const double bz = 0.5 * (U[nCd + nip] - U[nCd + nim]) / g.dx - 0.5 * (U[njp] - U[njm]) / g.dy;
        v[0] = v[0] + (jx * jx + jy * jy + jz * jz);
        v[1] = v[1] + (jy * bz - jz * by);
        v[2] = v[2] + (jz * bx - jx * bz);
        v[3] = v[3] + (jx * by - jy * bx);
    }
};

// the four terms of a cell outside the conductors: a, Jx, Jy, Jz
struct Linkage {
    static __device__ __forceinline__ void add(double (&v)[4], const Grid &g, int64_t pm, const double *__restrict__ U,
                                               const double *__restrict__ J)
    {
        const double s = -0.07957747154594766788444e7;
        const int64_t nCd = g.nCd;
        const double jx = s * J[pm], jy = s * J[nCd + pm], jz = s * J[2 * nCd + pm];
        v[0] = v[0] + ((U[pm] * jx + U[nCd + pm] * jy) + U[2 * nCd + pm] * jz);
        v[1] = v[1] + jx;
        v[2] = v[2] + jy;
        v[3] = v[3] + jz;
    }
};

// One workgroup per chunk.  cell: device cell p = kl*pitch + q of plane kl (k_vtk_fields' pm on an undivided handle);
// U and J are the device vectors X and B, component c of cell p at c*nCd + p.
template <class Term>
__global__ __launch_bounds__(256) void k_dom_partials(Grid g, const int32_t *__restrict__ cell,
                                                      const int32_t *__restrict__ chunk, const double *__restrict__ U,
                                                      const double *__restrict__ J, double *__restrict__ partial)
{
    __shared__ double lds[4 * 4];
    const int64_t first = chunk[3 * (int64_t)blockIdx.x];
    const int cnt = chunk[3 * (int64_t)blockIdx.x + 1];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < cnt; e += 256) // entries past the domain's end: no address formed, no load
        Term::add(v, g, cell[first + e], U, J);
    stream_block_sum<4>(v, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) partial[4 * (int64_t)blockIdx.x + c] = v[c];
}

// One workgroup per domain: thread t adds the partials of the domain's chunks t, t + 256, ... in order.
__global__ __launch_bounds__(256) void k_dom_final(const int32_t *__restrict__ dom_chunk,
                                                   const double *__restrict__ partial, double *__restrict__ sums)
{
    __shared__ double lds[4 * 4];
    const int64_t c0 = dom_chunk[blockIdx.x], c1 = dom_chunk[blockIdx.x + 1];
    double v[4];
    stream_strided_sum<4>(v, partial + 4 * c0, c1 - c0, 1, 4);
    stream_block_sum<4>(v, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) sums[4 * (int64_t)blockIdx.x + c] = v[c];
}

// ---- the streaming pass -------------------------------------------------------------------------------------------------
// Two neighbouring doubles.  V: one 16-byte access -- the caller knows the address to be even and row a + 1 to lie inside
// the vector (a cell, or a row of the pitch gap whose value is dropped).  Otherwise 8-byte accesses, the second only when
// it is a cell.
template <bool V> __device__ __forceinline__ d2 load2(const double *__restrict__ p, int64_t a, bool second)
{
    if (V) return stream_load(p, a);
    d2 v;
    v.x = p[a];
    v.y = second ? p[a + 1] : 0.0;
    return v;
}

// VP: the plane pitch is even (centre and +-plane neighbours as 16-byte accesses); VY: so is sdx (+-sdx neighbours too: both
// cells of a thread then lie in one grid row).  cond: one byte per device cell, 1 inside a conductor; NULL without any.
// part: sum j of workgroup b at part[j * gridDim.x + b].
template <bool VP, bool VY>
__global__ __launch_bounds__(256) void k_field_energy(Grid g, int cpp, int nchunk, const uint8_t *__restrict__ cond,
                                                      const double *__restrict__ U, const double *__restrict__ J,
                                                      double *__restrict__ part)
{
    __shared__ double lds[4 * EC3D_ENERGY_NV];
    const double s = -0.07957747154594766788444e7;
    const int kdz = g.sdx * g.sdy;
    const int64_t nCd = g.nCd;
    double acc[EC3D_ENERGY_NV] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const int k = ch / cpp;
        const int q = (ch - k * cpp) * EC3D_TILE + 2 * (int)threadIdx.x; // cell of the plane
        if (q >= kdz) continue;                                          // past the plane's end: nothing is read
        const bool two = q + 1 < kdz;
        const int64_t pm = (int64_t)k * g.pitch + q;
        const double *Ux = U + pm, *Uy = U + nCd + pm, *Uz = U + 2 * nCd + pm;
        const d2 ax = load2<VP>(Ux, 0, two), ay = load2<VP>(Uy, 0, two), az = load2<VP>(Uz, 0, two);
        const d2 jx = load2<VP>(J + pm, 0, two), jy = load2<VP>(J + nCd + pm, 0, two), jz = load2<VP>(J + 2 * nCd + pm, 0, two);
        // +-plane: both cells share k
        const int64_t okm = k == 0 ? 0 : -g.pitch, okp = k == g.sdz - 1 ? 0 : g.pitch;
        const d2 axkm = load2<VP>(Ux, okm, two), axkp = load2<VP>(Ux, okp, two);
        const d2 aykm = load2<VP>(Uy, okm, two), aykp = load2<VP>(Uy, okp, two);
        // +-sdx
        const int j0 = q / g.sdx, i0 = q - j0 * g.sdx;
        const int i1 = i0 + 1 == g.sdx ? 0 : i0 + 1, j1 = i0 + 1 == g.sdx ? j0 + 1 : j0;
        const int64_t ojm = j0 == 0 ? 0 : -g.sdx, ojp = j0 == g.sdy - 1 ? 0 : g.sdx;
        d2 axjm, axjp, azjm, azjp;
        if (VY) {
            axjm = load2<true>(Ux, ojm, two), axjp = load2<true>(Ux, ojp, two);
            azjm = load2<true>(Uz, ojm, two), azjp = load2<true>(Uz, ojp, two);
        } else {
            axjm.x = Ux[ojm], axjp.x = Ux[ojp], azjm.x = Uz[ojm], azjp.x = Uz[ojp];
            axjm.y = axjp.y = azjm.y = azjp.y = 0.0;
            if (two) {
                const int64_t pjm = j1 == 0 ? 1 : 1 - g.sdx, pjp = j1 == g.sdy - 1 ? 1 : 1 + g.sdx;
                axjm.y = Ux[pjm], axjp.y = Ux[pjp], azjm.y = Uz[pjm], azjp.y = Uz[pjp];
            }
        }
        // +-1: the pair holds each cell's neighbour inside it; rows q - 1 and q + 2 are loaded where they are cells of the row
        d2 ayim, ayip, azim, azip;
        ayim.x = ay.x, azim.x = az.x;
        if (i0 != 0) ayim.x = Uy[-1], azim.x = Uz[-1];
        ayip.x = i0 == g.sdx - 1 ? ay.x : ay.y, azip.x = i0 == g.sdx - 1 ? az.x : az.y;
        ayim.y = i1 == 0 ? ay.y : ay.x, azim.y = i1 == 0 ? az.y : az.x;
        ayip.y = ay.y, azip.y = az.y;
        if (two && i1 != g.sdx - 1) ayip.y = Uy[2], azip.y = Uz[2];
        const bool c0 = cond && cond[pm] != 0, c1 = cond && two && cond[pm + 1] != 0;
        {
            const double bx = 0.5 * (azjp.x - azjm.x) / g.dy - 0.5 * (aykp.x - aykm.x) / g.dz;
            const double by = 0.5 * (axkp.x - axkm.x) / g.dz - 0.5 * (azip.x - azim.x) / g.dx;
            const double bz = 0.5 * (ayip.x - ayim.x) / g.dx - 0.5 * (axjp.x - axjm.x) / g.dy;
            const double a = (ax.x * (s * jx.x) + ay.x * (s * jy.x)) + az.x * (s * jz.x);
            acc[0] = acc[0] + bx * bx;
            acc[1] = acc[1] + by * by;
            acc[2] = acc[2] + bz * bz;
            acc[3] = acc[3] + (c0 ? 0.0 : a);
            acc[4] = acc[4] + (c0 ? a : 0.0);
        }
        if (two) {
            const double bx = 0.5 * (azjp.y - azjm.y) / g.dy - 0.5 * (aykp.y - aykm.y) / g.dz;
            const double by = 0.5 * (axkp.y - axkm.y) / g.dz - 0.5 * (azip.y - azim.y) / g.dx;
            const double bz = 0.5 * (ayip.y - ayim.y) / g.dx - 0.5 * (axjp.y - axjm.y) / g.dy;
            const double a = (ax.y * (s * jx.y) + ay.y * (s * jy.y)) + az.y * (s * jz.y);
            acc[0] = acc[0] + bx * bx;
            acc[1] = acc[1] + by * by;
            acc[2] = acc[2] + bz * bz;
            acc[3] = acc[3] + (c1 ? 0.0 : a);
            acc[4] = acc[4] + (c1 ? a : 0.0);
        }
    }
    stream_block_sum<EC3D_ENERGY_NV>(acc, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < EC3D_ENERGY_NV; ++c) part[(int64_t)c * gridDim.x + blockIdx.x] = acc[c];
}

// One workgroup: thread t adds the partials t, t + 256, ... of every sum in order.
__global__ __launch_bounds__(256) void k_energy_collapse(const double *__restrict__ part, int count, double *__restrict__ sums)
{
    __shared__ double lds[4 * EC3D_ENERGY_NV];
    double v[EC3D_ENERGY_NV];
    stream_strided_sum<EC3D_ENERGY_NV>(v, part, count, count);
    stream_block_sum<EC3D_ENERGY_NV>(v, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < EC3D_ENERGY_NV; ++c) sums[c] = v[c];
}

__global__ void k_cond_bytes(uint8_t *cond, const int32_t *__restrict__ cell, int64_t ncond)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < ncond) cond[cell[m]] = 1;
}

Grid grid_of(const ec3d_ctx *c, const double *delta)
{
    const int64_t kdz = (int64_t)c->sdx * c->sdy;
    return Grid{c->sdx, c->sdy, c->sdz, c->pitch ? c->pitch : kdz, c->nCd ? c->nCd : c->n_cells, delta[0], delta[1], delta[2]};
}

// The domains that hold cells of the wanted kind (conducting or not), ascending id, and their cells' device indices sorted
// by (domain id, scan order), cut into chunks.
void build_lists(const ec3d_ctx *c, int64_t nCells, const int8_t *geoPHYS, const int32_t *geoPHYS_C, int32_t nsub_glob,
                 bool conducting, std::vector<int32_t> &id, std::vector<int64_t> &cells, std::vector<int32_t> &cell,
                 std::vector<int32_t> &chunk, std::vector<int32_t> &dom_chunk)
{
    std::vector<int64_t> count((size_t)nsub_glob + 1, 0);
    for (int64_t q = 0; q < nCells; ++q)
        if ((geoPHYS_C[q] != 0) == conducting) ++count[(size_t)geoPHYS[q]];
    std::vector<int64_t> at((size_t)nsub_glob + 1, -1); // domain id -> where its next cell goes
    int64_t n = 0;
    for (int32_t d = 0; d <= nsub_glob; ++d) { // ascending id
        if (count[(size_t)d] == 0) continue;
        id.push_back(d);
        cells.push_back(count[(size_t)d]);
        at[(size_t)d] = n;
        dom_chunk.push_back((int32_t)(chunk.size() / 3));
        for (int64_t e = 0; e < count[(size_t)d]; e += EC3D_DOM_CHUNK) {
            chunk.push_back((int32_t)(n + e));
            chunk.push_back((int32_t)std::min<int64_t>(EC3D_DOM_CHUNK, count[(size_t)d] - e));
            chunk.push_back((int32_t)id.size() - 1);
        }
        n += count[(size_t)d];
    }
    if (n == 0) return;
    dom_chunk.push_back((int32_t)(chunk.size() / 3));
    cell.resize((size_t)n);
    for (int64_t q = 0; q < nCells; ++q) // scan order within each domain
        if ((geoPHYS_C[q] != 0) == conducting) cell[(size_t)at[(size_t)geoPHYS[q]]++] = (int32_t)c->dev_cell(q);
}

// the chunk launch, the per-domain launch, the call's one copy and its one synchronisation
template <class Term>
int list_sums(ec3d_ctx *c, const double *delta, int ndom, int64_t nchunk, const int32_t *cell, const int32_t *chunk,
              const int32_t *dom_chunk, double *partial, double *sums, double *host)
{
    k_dom_partials<Term><<<(unsigned)nchunk, 256, 0, c->stream>>>(grid_of(c, delta), cell, chunk, c->vec[EC3D_VEC_X],
                                                                 c->vec[EC3D_VEC_B], partial);
    k_dom_final<<<(unsigned)ndom, 256, 0, c->stream>>>(dom_chunk, partial, sums);
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipMemcpyAsync(host, sums, (size_t)32 * ndom, hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

} // namespace

int ec3d_need_undivided(ec3d_ctx *c, const char *who)
{
    if (!c || !c->have_matrix || c->sdx == 0 || c->n_cells == 0 || c->A.n < 3 * c->n_cells) { // as ec3d_vtk_fields
        ec3d_set_error(std::string(who) + ": needs the A-V system [Ax|Ay|Az|U] from ec3d_assemble");
        return 3;
    }
    if (c->in_multi || c->n_cells != (int64_t)c->sdx * c->sdy * c->sdz) {
        ec3d_set_error(std::string(who) + ": a z-slab holds only part of a domain; undivided handles (ec3d_assemble) only");
        return 5;
    }
    return 0;
}

void ec3d_free_integrals(ec3d_ctx *c)
{
    c->dom = DomIntegrals();
    c->link = DomLinkage();
    c->energy = FieldEnergy();
}

// Called by ec3d_setup_rhs with the geometry of an undivided handle.  The conducting domains' tables are built into `d` and
// moved into the handle at the end: a failure leaves the handle without them (ec3d_domain_integrals then says so).  The
// non-conducting domains' lists stay on the host: ec3d_domain_linkage uploads them when it is first called.
int ec3d_setup_integrals(ec3d_ctx *c, int64_t nCells, const int8_t *geoPHYS, const int32_t *geoPHYS_C,
                         const double *valPHYS, int32_t nsub_glob)
{
    ec3d_free_integrals(c);
    {
        DomLinkage l;
        build_lists(c, nCells, geoPHYS, geoPHYS_C, nsub_glob, false, l.id, l.cells, l.cell_host, l.chunk_host, l.dom_chunk_host);
        l.ndom = (int)l.id.size();
        l.nchunk = (int64_t)(l.chunk_host.size() / 3);
        l.built = true;
        c->link = std::move(l);
    }
    DomIntegrals d;
    std::vector<int32_t> cell, chunk, dom_chunk;
    build_lists(c, nCells, geoPHYS, geoPHYS_C, nsub_glob, true, d.id, d.cells, cell, chunk, dom_chunk);
    if (cell.empty()) return 0;
    for (int32_t id : d.id) d.C.push_back(valPHYS[1 * (int64_t)nsub_glob + id - 1]); // valPHYS(id, 2), as ec3d_setup_rhs reads it
    d.ndom = (int)d.id.size();
    d.nchunk = (int64_t)(chunk.size() / 3);
    EC3D_HIP(d.cell.alloc(cell.size()));
    EC3D_HIP(d.chunk.alloc(chunk.size()));
    EC3D_HIP(d.dom_chunk.alloc(dom_chunk.size()));
    EC3D_HIP(d.partial.alloc((size_t)4 * d.nchunk));
    EC3D_HIP(d.sums.alloc((size_t)4 * d.ndom));
    EC3D_HIP(d.host.alloc((size_t)4 * d.ndom));
    EC3D_HIP(hipMemcpyAsync(d.cell, cell.data(), cell.size() * 4, hipMemcpyHostToDevice, c->stream));
    EC3D_HIP(hipMemcpyAsync(d.chunk, chunk.data(), chunk.size() * 4, hipMemcpyHostToDevice, c->stream));
    EC3D_HIP(hipMemcpyAsync(d.dom_chunk, dom_chunk.data(), dom_chunk.size() * 4, hipMemcpyHostToDevice, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream)); // the host vectors go out of scope
    c->dom = std::move(d);
    return 0;
}

extern "C" int ec3d_domain_integrals(ec3d_handle c, const double *delta, int32_t cap, int32_t *ndomains,
                                     ec3d_domain_integral *out)
{
    int rc = ec3d_need_undivided(c, "ec3d_domain_integrals");
    if (rc) return rc;
    if (!delta || !ndomains) {
        ec3d_set_error("ec3d_domain_integrals: delta and ndomains are required");
        return 2;
    }
    const DomIntegrals &d = c->dom;
    if (c->n_cond > 0 && d.ndom == 0) {
        ec3d_set_error("ec3d_domain_integrals: the handle has no domain tables (their set-up failed at assembly)");
        return 100;
    }
    *ndomains = d.ndom;
    if (!out || d.ndom == 0) return 0;
    if (cap < d.ndom) {
        ec3d_set_error("ec3d_domain_integrals: " + std::to_string(d.ndom) + " conducting domains, room for " +
                       std::to_string(cap));
        return 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    rc = list_sums<JouleForce>(c, delta, d.ndom, d.nchunk, d.cell, d.chunk, d.dom_chunk, d.partial, d.sums, d.host);
    if (rc) return rc;
    const double vol = delta[0] * delta[1] * delta[2];
    for (int m = 0; m < d.ndom; ++m) {
        const double *s = d.host + 4 * m;
        ec3d_domain_integral &o = out[m];
        o.domain = d.id[(size_t)m];
        o.pad = 0;
        o.cells = d.cells[(size_t)m];
        o.sigma = d.C[(size_t)m] * 0.07957747154594766788444e7;
        o.joule_w = vol * s[0] / o.sigma;
        for (int a = 0; a < 3; ++a) o.force_n[a] = vol * s[1 + a];
    }
    return 0;
}

extern "C" int ec3d_domain_linkage(ec3d_handle c, const double *delta, int32_t cap, int32_t *ndomains, ec3d_domain_link *out)
{
    int rc = ec3d_need_undivided(c, "ec3d_domain_linkage");
    if (rc) return rc;
    if (!delta || !ndomains) {
        ec3d_set_error("ec3d_domain_linkage: delta and ndomains are required");
        return 2;
    }
    DomLinkage &d = c->link;
    if (!d.built) {
        ec3d_set_error("ec3d_domain_linkage: the handle has no domain lists (their set-up failed at assembly)");
        return 100;
    }
    *ndomains = d.ndom;
    if (!out || d.ndom == 0) return 0;
    if (cap < d.ndom) {
        ec3d_set_error("ec3d_domain_linkage: " + std::to_string(d.ndom) + " non-conducting domains, room for " +
                       std::to_string(cap));
        return 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    if (!d.cell) { // the first call: the lists go to the device, the host keeps the ids and counts
        DevBuf<int32_t> cell, chunk, dom_chunk;
        EC3D_HIP(cell.alloc(d.cell_host.size()));
        EC3D_HIP(chunk.alloc(d.chunk_host.size()));
        EC3D_HIP(dom_chunk.alloc(d.dom_chunk_host.size()));
        EC3D_HIP(d.partial.alloc((size_t)4 * d.nchunk));
        EC3D_HIP(d.sums.alloc((size_t)4 * d.ndom));
        EC3D_HIP(d.host.alloc((size_t)4 * d.ndom));
        EC3D_HIP(hipMemcpyAsync(cell, d.cell_host.data(), d.cell_host.size() * 4, hipMemcpyHostToDevice, c->stream));
        EC3D_HIP(hipMemcpyAsync(chunk, d.chunk_host.data(), d.chunk_host.size() * 4, hipMemcpyHostToDevice, c->stream));
        EC3D_HIP(hipMemcpyAsync(dom_chunk, d.dom_chunk_host.data(), d.dom_chunk_host.size() * 4, hipMemcpyHostToDevice,
                                c->stream));
        EC3D_HIP(hipStreamSynchronize(c->stream));
        d.chunk = std::move(chunk);
        d.dom_chunk = std::move(dom_chunk);
        d.cell = std::move(cell);
        std::vector<int32_t>().swap(d.cell_host);
        std::vector<int32_t>().swap(d.chunk_host);
        std::vector<int32_t>().swap(d.dom_chunk_host);
    }
    rc = list_sums<Linkage>(c, delta, d.ndom, d.nchunk, d.cell, d.chunk, d.dom_chunk, d.partial, d.sums, d.host);
    if (rc) return rc;
    const double vol = delta[0] * delta[1] * delta[2];
    for (int m = 0; m < d.ndom; ++m) {
        const double *s = d.host + 4 * m;
        ec3d_domain_link &o = out[m];
        o.domain = d.id[(size_t)m];
        o.pad = 0;
        o.cells = d.cells[(size_t)m];
        o.linkage = vol * s[0];
        for (int a = 0; a < 3; ++a) o.jsum[a] = vol * s[1 + a];
    }
    return 0;
}

extern "C" int ec3d_field_energy(ec3d_handle c, const double *delta, ec3d_field_energy_info *out)
{
    int rc = ec3d_need_undivided(c, "ec3d_field_energy");
    if (rc) return rc;
    if (!delta || !out) {
        ec3d_set_error("ec3d_field_energy: delta and out are required");
        return 2;
    }
    EC3D_HIP(hipSetDevice(c->device));
    const Grid g = grid_of(c, delta);
    const int64_t kdz = (int64_t)c->sdx * c->sdy;
    const int cpp = (int)((kdz + EC3D_TILE - 1) / EC3D_TILE);
    const int nchunk = cpp * c->sdz; // (below n_cells, which fits the library's int32 row index)
    FieldEnergy &e = c->energy;
    if (!e.part) { // the first call
        DevBuf<uint8_t> cond;
        if (c->n_cond > 0) {
            const size_t rows = (size_t)(g.pitch * c->sdz);
            EC3D_HIP(cond.alloc(rows));
            EC3D_HIP(hipMemsetAsync(cond, 0, rows, c->stream));
            k_cond_bytes<<<(unsigned)((c->n_cond + 255) / 256), 256, 0, c->stream>>>(cond, c->cond_cell, c->n_cond);
            EC3D_HIP(hipGetLastError());
        }
        e.wgs = ec3d_stream_wgs((int64_t)nchunk * EC3D_TILE);
        EC3D_HIP(e.sums.alloc(EC3D_ENERGY_NV));
        EC3D_HIP(e.host.alloc(EC3D_ENERGY_NV));
        EC3D_HIP(e.part.alloc((size_t)EC3D_ENERGY_NV * e.wgs));
        e.cond = std::move(cond);
    }
    const double *U = c->vec[EC3D_VEC_X], *J = c->vec[EC3D_VEC_B];
    const uint8_t *cond = c->n_cond > 0 ? e.cond.get() : nullptr;
    // 16-byte accesses: even cell addresses in every component block, over 16-byte aligned vectors
    const bool vp = g.pitch % 2 == 0 && g.nCd % 2 == 0 && ((uintptr_t)U | (uintptr_t)J) % 16 == 0;
    const bool vy = vp && c->sdx % 2 == 0;
    const unsigned G = (unsigned)e.wgs;
    if (vy) k_field_energy<true, true><<<G, 256, 0, c->stream>>>(g, cpp, nchunk, cond, U, J, e.part);
    else if (vp) k_field_energy<true, false><<<G, 256, 0, c->stream>>>(g, cpp, nchunk, cond, U, J, e.part);
    else k_field_energy<false, false><<<G, 256, 0, c->stream>>>(g, cpp, nchunk, cond, U, J, e.part);
    k_energy_collapse<<<1, 256, 0, c->stream>>>(e.part, e.wgs, e.sums);
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipMemcpyAsync(e.host, e.sums, EC3D_ENERGY_NV * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    const double *s = e.host;
    const double vol = delta[0] * delta[1] * delta[2], half = vol * (0.5 * 0.07957747154594766788444e7);
    out->cells = c->n_cells;
    for (int a = 0; a < 3; ++a) out->energy_axis[a] = half * s[a];
    out->energy_b = half * ((s[0] + s[1]) + s[2]);
    out->aj_source = vol * s[3];
    out->aj_eddy = vol * s[4];
    return 0;
}
