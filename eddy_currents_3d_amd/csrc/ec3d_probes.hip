// ec3d_probes.hip — the resident fields at chosen cells, sampled on the device: ec3d_set_probes, ec3d_probe_sample,
// ec3d_probe_record, ec3d_probe_read, ec3d_probe_reset, ec3d_get_probes.
//
// A probe is a cell of the box.  Its 13 values are what field_N.vtk shows at that cell (k_vtk_fields, ec3d_output.hip;
// writeVtk_field, src/utilites.f90:222-289) BEFORE the rounding to float32, and the cell's scalar potential:
//    0 ..  2  a       A
//    3 ..  5  eddy    s * Jaf in a conductor cell, else 0.0;  s = -0.07957747154594766788444d7
//    6 ..  8  source  Jaf outside the conductors, else 0.0
//    9 .. 11  b       curl A, central differences clamped at the box faces
//   12        u       the cell's U, 0.0 outside the conductors
// The same literal, the same clamping and the same expression order as k_vtk_fields, no contraction: (float) of the
// first twelve is bit for bit what ec3d_vtk_fields returns at the cell.
//
// ec3d_set_probes resolves every cell on the host, once: to its device cell kl*pitch + q, and -- a conductor cell -- to
// the device row of its U unknown (ec3d_get_row_map's), -1 otherwise.  The kernel therefore is the same for the
// structured form, any plane pitch, and bands + tail, and needs no conductor mask.
//
// Layout.  A record is 13 * nprobes doubles, by component, then by probe: value c of probe p at c*nprobes + p, so
// neighbouring threads store neighbouring doubles; a box listed in scan order (probe_box) loads neighbouring cells
// too.  The record buffer holds `capacity` of them one after the other; ec3d_probe_record writes record number
// `recorded` on the handle's stream and waits for nothing, ec3d_probe_read brings a run of records back with one copy.
// The kernel does not reduce: no LDS, no atomics, one thread per probe in a grid-stride loop.
#include "ec3d_internal.hpp"

#include <algorithm>

#define EC3D_PROBE_MAX_WGS 1024 /* workgroups of a launch at most: ceil(nprobes / 256) below that, the stride loop above */

namespace {

struct ProbeGrid {
    int sdx, sdy, sdz;
    int64_t pitch, nCd; // device rows per xy plane and per component block
    double dx, dy, dz;
};

// cell: device cell p = kl*pitch + q (k_vtk_fields' pm on an undivided handle); urow: device row of the cell's U, -1
// outside the conductors; U and J are the device vectors X and B, component c of cell p at c*nCd + p.
__global__ __launch_bounds__(256) void k_probe_sample(ProbeGrid g, int64_t n, const int32_t *__restrict__ cell,
                                                      const int32_t *__restrict__ urow, const double *__restrict__ U,
                                                      const double *__restrict__ J, double *__restrict__ out)
{
    const double s = -0.07957747154594766788444e7;
    const int64_t nCd = g.nCd, sdx = g.sdx, pitch = g.pitch;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int64_t pm = cell[p], ur = urow[p];
        const int64_t q = pm % pitch;
        const int i = (int)(q % sdx) + 1, j = (int)(q / sdx) + 1, k = (int)(pm / pitch) + 1;
        const bool cond = ur >= 0;
        out[0 * n + p] = U[pm];
        out[1 * n + p] = U[nCd + pm];
        out[2 * n + p] = U[2 * nCd + pm];
        for (int c = 0; c < 3; ++c) {
            const double jaf = J[c * nCd + pm];
            out[(3 + c) * n + p] = cond ? s * jaf : 0.0;
            out[(6 + c) * n + p] = cond ? 0.0 : jaf;
        }
        const int64_t nim = i == 1 ? pm : pm - 1, nip = i == g.sdx ? pm : pm + 1;
        const int64_t njm = j == 1 ? pm : pm - sdx, njp = j == g.sdy ? pm : pm + sdx;
        const int64_t nkm = k == 1 ? pm : pm - pitch, nkp = k == g.sdz ? pm : pm + pitch;
        const double bx = 0.5 * (U[2 * nCd + njp] - U[2 * nCd + njm]) / g.dy - 0.5 * (U[nCd + nkp] - U[nCd + nkm]) / g.dz;
        const double by = 0.5 * (U[nkp] - U[nkm]) / g.dz - 0.5 * (U[2 * nCd + nip] - U[2 * nCd + nim]) / g.dx;
        const double bz = 0.5 * (U[nCd + nip] - U[nCd + nim]) / g.dx - 0.5 * (U[njp] - U[njm]) / g.dy;
        out[9 * n + p] = bx;
        out[10 * n + p] = by;
        out[11 * n + p] = bz;
        out[12 * n + p] = cond ? U[ur] : 0.0;
    }
}

// what every call but ec3d_get_probes needs: an undivided A-V handle (3, 5), then a probe set (2)
int need_probes(ec3d_ctx *c, const char *who)
{
    int rc = ec3d_need_undivided(c, who);
    if (rc) return rc;
    if (c->probes.n == 0) {
        ec3d_set_error(std::string(who) + ": no probes are set (ec3d_set_probes)");
        return 2;
    }
    return 0;
}

int launch(ec3d_ctx *c, const double *delta, double *out)
{
    const Probes &d = c->probes;
    const int64_t kdz = (int64_t)c->sdx * c->sdy;
    const ProbeGrid g{c->sdx, c->sdy, c->sdz, c->pitch ? c->pitch : kdz, c->nCd ? c->nCd : c->n_cells,
                      delta[0], delta[1], delta[2]};
    const unsigned wgs = (unsigned)std::min<int64_t>((d.n + 255) / 256, EC3D_PROBE_MAX_WGS);
    k_probe_sample<<<wgs, 256, 0, c->stream>>>(g, d.n, d.cell, d.urow, c->vec[EC3D_VEC_X], c->vec[EC3D_VEC_B], out);
    EC3D_HIP(hipGetLastError());
    return 0;
}

} // namespace

void ec3d_free_probes(ec3d_ctx *c) { c->probes = Probes(); }

extern "C" int ec3d_set_probes(ec3d_handle c, int64_t nprobes, const int64_t *cells, int64_t capacity)
{
    int rc = ec3d_need_undivided(c, "ec3d_set_probes");
    if (rc) return rc;
    if (nprobes < 0 || capacity < 0 || (nprobes > 0 && !cells)) {
        ec3d_set_error("ec3d_set_probes: nprobes and capacity must not be negative, and cells is required");
        return 2;
    }
    for (int64_t p = 0; p < nprobes; ++p)
        if (cells[p] < 0 || cells[p] >= c->n_cells) {
            ec3d_set_error("ec3d_set_probes: cells[" + std::to_string(p) + "] = " + std::to_string(cells[p]) +
                           " is outside the box of " + std::to_string(c->n_cells) + " cells");
            return 2;
        }
    if (nprobes == 0) {
        ec3d_free_probes(c);
        return 0;
    }
    EC3D_HIP(hipSetDevice(c->device));
    // the conductor cells' device cells, ascending (scan order): entry m belongs to U unknown m
    std::vector<int32_t> ccell((size_t)c->n_cond);
    if (c->n_cond) EC3D_HIP(hipMemcpy(ccell.data(), c->cond_cell, ccell.size() * 4, hipMemcpyDeviceToHost));
    const int64_t ubase = c->A.sav ? 3 * c->A.sav_nC : 3 * c->n_cells;
    std::vector<int32_t> cell((size_t)nprobes), urow((size_t)nprobes);
    for (int64_t p = 0; p < nprobes; ++p) {
        const int32_t dev = (int32_t)c->dev_cell(cells[p]);
        const auto at = std::lower_bound(ccell.begin(), ccell.end(), dev);
        cell[(size_t)p] = dev;
        if (at == ccell.end() || *at != dev) urow[(size_t)p] = -1;
        else urow[(size_t)p] = (int32_t)(ubase + (c->A.sav ? (int64_t)dev : (int64_t)(at - ccell.begin())));
    }
    Probes d; // moved into the handle when complete: a failure leaves the previous set in place
    d.n = nprobes;
    d.capacity = capacity;
    EC3D_HIP(d.cell.alloc((size_t)nprobes));
    EC3D_HIP(d.urow.alloc((size_t)nprobes));
    EC3D_HIP(d.sample.alloc((size_t)EC3D_PROBE_NCOMP * nprobes));
    if (capacity) EC3D_HIP(d.record.alloc((size_t)EC3D_PROBE_NCOMP * nprobes * capacity));
    d.T.reserve((size_t)capacity);
    EC3D_HIP(hipMemcpyAsync(d.cell, cell.data(), cell.size() * 4, hipMemcpyHostToDevice, c->stream));
    EC3D_HIP(hipMemcpyAsync(d.urow, urow.data(), urow.size() * 4, hipMemcpyHostToDevice, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream)); // the host vectors go out of scope
    c->probes = std::move(d);
    return 0;
}

extern "C" int ec3d_probe_sample(ec3d_handle c, const double *delta, double *out)
{
    int rc = need_probes(c, "ec3d_probe_sample");
    if (rc) return rc;
    if (!delta || !out) {
        ec3d_set_error("ec3d_probe_sample: delta and out are required");
        return 2;
    }
    const Probes &d = c->probes;
    EC3D_HIP(hipSetDevice(c->device));
    if ((rc = launch(c, delta, d.sample))) return rc;
    EC3D_HIP(hipMemcpyAsync(out, d.sample, (size_t)EC3D_PROBE_NCOMP * d.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ec3d_probe_record(ec3d_handle c, const double *delta, double T)
{
    int rc = need_probes(c, "ec3d_probe_record");
    if (rc) return rc;
    if (!delta) {
        ec3d_set_error("ec3d_probe_record: delta is required");
        return 2;
    }
    Probes &d = c->probes;
    if (d.recorded >= d.capacity) {
        ec3d_set_error("ec3d_probe_record: the buffer holds " + std::to_string(d.capacity) +
                       " records and is full (ec3d_probe_read, then ec3d_probe_reset)");
        return EC3D_PROBE_E_FULL;
    }
    EC3D_HIP(hipSetDevice(c->device));
    if ((rc = launch(c, delta, d.record + EC3D_PROBE_NCOMP * d.n * d.recorded))) return rc;
    d.T.push_back(T);
    ++d.recorded;
    return 0;
}

extern "C" int ec3d_probe_read(ec3d_handle c, int64_t first, int64_t count, double *T_out, double *out)
{
    int rc = need_probes(c, "ec3d_probe_read");
    if (rc) return rc;
    const Probes &d = c->probes;
    if (!T_out || !out) {
        ec3d_set_error("ec3d_probe_read: T_out and out are required");
        return 2;
    }
    if (first < 0 || count < 0 || first > d.recorded || count > d.recorded - first) {
        ec3d_set_error("ec3d_probe_read: records [" + std::to_string(first) + ", " + std::to_string(first) + " + " +
                       std::to_string(count) + ") of " + std::to_string(d.recorded) + " recorded");
        return 2;
    }
    if (count == 0) return 0;
    EC3D_HIP(hipSetDevice(c->device));
    const int64_t rec = EC3D_PROBE_NCOMP * d.n;
    EC3D_HIP(hipMemcpyAsync(out, d.record + rec * first, (size_t)(rec * count) * sizeof(double), hipMemcpyDeviceToHost,
                            c->stream));
    EC3D_HIP(hipStreamSynchronize(c->stream));
    std::copy(d.T.begin() + first, d.T.begin() + first + count, T_out);
    return 0;
}

extern "C" int ec3d_probe_reset(ec3d_handle c)
{
    int rc = need_probes(c, "ec3d_probe_reset");
    if (rc) return rc;
    // records still being written are overwritten in stream order by the next ec3d_probe_record: nothing to wait for
    c->probes.recorded = 0;
    c->probes.T.clear();
    return 0;
}

extern "C" int ec3d_get_probes(ec3d_handle c, ec3d_probe_info *info)
{
    if (!c || !info) {
        ec3d_set_error("ec3d_get_probes: the handle and info are required");
        return 2;
    }
    const Probes &d = c->probes;
    info->nprobes = d.n;
    info->capacity = d.capacity;
    info->recorded = d.recorded;
    info->device_bytes = d.n ? 8 * d.n + (int64_t)sizeof(double) * EC3D_PROBE_NCOMP * d.n * (1 + d.capacity) : 0;
    return 0;
}
