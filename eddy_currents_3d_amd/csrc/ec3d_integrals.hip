// ec3d_integrals.hip — per-domain Joule loss and Lorentz force from the resident fields, on the device.
//
// The integrals, over each conducting domain, of the very fields field_N.vtk shows (k_vtk_fields, ec3d_output.hip;
// writeVtk_field, src/utilites.f90:238-289) BEFORE their rounding to float32:
//   J = s * Jaf on the conductor cells, s = -0.07957747154594766788444d7 (= -1/mu0; valPHYS(:,2) is mu0*sigma)
//   B = curl A, central differences clamped at the box faces
//   q = Jx*Jx + Jy*Jy + Jz*Jz,   f = J x B
// per domain d: joule_w = (dx*dy*dz) * sum(q) / sigma_d,  force_n = (dx*dy*dz) * sum(f).  Not a Maxwell-stress evaluation.
//
// Layout.  dom.cell: the conductor cells' device indices sorted by (domain id, scan order), 4 B per cell.  The list is cut
// into chunks of EC3D_DOM_CHUNK entries that never straddle a domain (a domain's last chunk may be short); dom.chunk holds
// (first entry, entries, domain ordinal) per chunk and dom.dom_chunk the first chunk of every domain.  The order is a
// property of the geometry, not of the storage: the structured form and bands + tail sum the same values in the same order.
//
// Summation chain (no float atomics: the result is a pure function of X, B and the geometry).  A value of sums[d] is reached
// through, at most,
//   k_dom_partials   3 additions of a thread's own 4 entries (stride 256), 6 levels of the wave's shuffle tree, 4 wave sums
//   k_dom_final      ceil(chunks_d / 256) - 1 additions of a thread's own partials (stride 256), 6 levels, 4 wave sums
// i.e. 13 + ceil(n_d / 262144) + 9 dependent additions for a domain of n_d cells: 61 at 10 M cells, and below 2100 for any
// list whose device rows fit the library's int32 row index (4 nCd < 2^31).
#include "ec3d_internal.hpp"

#include <algorithm>

#define EC3D_DOM_CHUNK 1024 /* list entries per workgroup of k_dom_partials: 4 per thread */

namespace {

// the four sums of a 256-thread workgroup: 64-lane shuffle tree, then the waves' values through the LDS (block_sum of
// ec3d_mg.hip, four values at once).  Valid in thread 0.
__device__ __forceinline__ void block_sum4(double v[4], double (*lds)[4])
{
    for (int c = 0; c < 4; ++c)
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_down(v[c], o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0)
        for (int c = 0; c < 4; ++c) lds[wid][c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
            for (int q = 0; q < (int)(blockDim.x >> 6); ++q) s += lds[q][c];
            v[c] = s;
        }
}

// One workgroup per chunk.  cell: device cell p = kl*pitch + q of plane kl (k_vtk_fields' pm on an undivided handle);
// U and J are the device vectors X and B, component c of cell p at c*nCd + p.
__global__ __launch_bounds__(256) void k_dom_partials(int sdx, int sdy, int sdz, int64_t pitch, int64_t nCd, double dx,
                                                      double dy, double dz, const int32_t *__restrict__ cell,
                                                      const int32_t *__restrict__ chunk, const double *__restrict__ U,
                                                      const double *__restrict__ J, double *__restrict__ partial)
{
    __shared__ double lds[4][4];
    const int64_t first = chunk[3 * (int64_t)blockIdx.x];
    const int cnt = chunk[3 * (int64_t)blockIdx.x + 1];
    const double s = -0.07957747154594766788444e7;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < cnt; e += 256) { // entries past the domain's end: no address formed, no load
        const int64_t pm = cell[first + e];
        const int64_t q = pm % pitch;
        const int i = (int)(q % sdx) + 1, j = (int)(q / sdx) + 1, k = (int)(pm / pitch) + 1;
        const double jx = s * J[pm], jy = s * J[nCd + pm], jz = s * J[2 * nCd + pm];
        const int64_t nim = i == 1 ? pm : pm - 1, nip = i == sdx ? pm : pm + 1;
        const int64_t njm = j == 1 ? pm : pm - sdx, njp = j == sdy ? pm : pm + sdx;
        const int64_t nkm = k == 1 ? pm : pm - pitch, nkp = k == sdz ? pm : pm + pitch;
        const double bx = 0.5 * (U[2 * nCd + njp] - U[2 * nCd + njm]) / dy - 0.5 * (U[nCd + nkp] - U[nCd + nkm]) / dz;
        const double by = 0.5 * (U[nkp] - U[nkm]) / dz - 0.5 * (U[2 * nCd + nip] - U[2 * nCd + nim]) / dx;
        const double bz = 0.5 * (U[nCd + nip] - U[nCd + nim]) / dx - 0.5 * (U[njp] - U[njm]) / dy;
        v[0] = v[0] + (jx * jx + jy * jy + jz * jz);
        v[1] = v[1] + (jy * bz - jz * by);
        v[2] = v[2] + (jz * bx - jx * bz);
        v[3] = v[3] + (jx * by - jy * bx);
    }
    block_sum4(v, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) partial[4 * (int64_t)blockIdx.x + c] = v[c];
}

// One workgroup per domain: thread t adds the partials of the domain's chunks t, t + 256, ... in order.
__global__ __launch_bounds__(256) void k_dom_final(const int32_t *__restrict__ dom_chunk,
                                                   const double *__restrict__ partial, double *__restrict__ sums)
{
    __shared__ double lds[4][4];
    const int64_t c0 = dom_chunk[blockIdx.x], c1 = dom_chunk[blockIdx.x + 1];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t ch = c0 + threadIdx.x; ch < c1; ch += 256)
        for (int c = 0; c < 4; ++c) v[c] = v[c] + partial[4 * ch + c];
    block_sum4(v, lds);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) sums[4 * (int64_t)blockIdx.x + c] = v[c];
}

} // namespace

void ec3d_free_integrals(ec3d_ctx *c) { c->dom = DomIntegrals(); }

// Called by ec3d_setup_rhs with the geometry of an undivided handle.  Everything is built into `d` and moved into the
// handle at the end: a failure leaves the handle without the tables (ec3d_domain_integrals then says so).
int ec3d_setup_integrals(ec3d_ctx *c, int64_t nCells, const int8_t *geoPHYS, const int32_t *geoPHYS_C,
                         const double *valPHYS, int32_t nsub_glob)
{
    ec3d_free_integrals(c);
    std::vector<int64_t> count((size_t)nsub_glob + 1, 0);
    for (int64_t q = 0; q < nCells; ++q)
        if (geoPHYS_C[q] != 0) ++count[(size_t)geoPHYS[q]];
    DomIntegrals d;
    std::vector<int64_t> at((size_t)nsub_glob + 1, -1); // domain id -> where its next cell goes
    std::vector<int32_t> chunk, dom_chunk;
    int64_t n = 0;
    for (int32_t id = 0; id <= nsub_glob; ++id) { // ascending id
        if (count[(size_t)id] == 0) continue;
        d.id.push_back(id);
        d.cells.push_back(count[(size_t)id]);
        d.C.push_back(valPHYS[1 * (int64_t)nsub_glob + id - 1]); // valPHYS(id, 2), as ec3d_setup_rhs reads it
        at[(size_t)id] = n;
        dom_chunk.push_back((int32_t)(chunk.size() / 3));
        for (int64_t e = 0; e < count[(size_t)id]; e += EC3D_DOM_CHUNK) {
            chunk.push_back((int32_t)(n + e));
            chunk.push_back((int32_t)std::min<int64_t>(EC3D_DOM_CHUNK, count[(size_t)id] - e));
            chunk.push_back((int32_t)d.id.size() - 1);
        }
        n += count[(size_t)id];
    }
    if (n == 0) return 0;
    dom_chunk.push_back((int32_t)(chunk.size() / 3));
    std::vector<int32_t> cell((size_t)n);
    for (int64_t q = 0; q < nCells; ++q) // scan order within each domain
        if (geoPHYS_C[q] != 0) cell[(size_t)at[(size_t)geoPHYS[q]]++] = (int32_t)c->dev_cell(q);
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
    if (!c || !c->have_matrix || c->sdx == 0 || c->n_cells == 0 || c->A.n < 3 * c->n_cells) { // as ec3d_vtk_fields
        ec3d_set_error("ec3d_domain_integrals: needs the A-V system [Ax|Ay|Az|U] from ec3d_assemble");
        return 3;
    }
    if (c->in_multi || c->n_cells != (int64_t)c->sdx * c->sdy * c->sdz) {
        ec3d_set_error("ec3d_domain_integrals: a z-slab holds only part of a domain; undivided handles (ec3d_assemble) only");
        return 5;
    }
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
    const int64_t kdz = (int64_t)c->sdx * c->sdy;
    const int64_t pitch = c->pitch ? c->pitch : kdz, nCd = c->nCd ? c->nCd : c->n_cells;
    k_dom_partials<<<(unsigned)d.nchunk, 256, 0, c->stream>>>(c->sdx, c->sdy, c->sdz, pitch, nCd, delta[0], delta[1],
                                                              delta[2], d.cell, d.chunk, c->vec[EC3D_VEC_X],
                                                              c->vec[EC3D_VEC_B], d.partial);
    k_dom_final<<<(unsigned)d.ndom, 256, 0, c->stream>>>(d.dom_chunk, d.partial, d.sums);
    EC3D_HIP(hipGetLastError());
    EC3D_HIP(hipMemcpyAsync(d.host, d.sums, (size_t)32 * d.ndom, hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
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
