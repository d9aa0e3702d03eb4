// ec3d_internal.hpp — shared declarations of libec3d_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ec3d_hip.h"
#include "ec3d_own.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>

#define EC3D_THREADS 256
#define EC3D_TILE 512 /* rows per tile: every thread owns 2 consecutive rows (one 16-B access) */
#define EC3D_SAV_MAXDOM 22 /* conducting domains the structured form holds: 55 + 9 D classes fit a byte */
#define EC3D_MAXB 16  /* DIA bands */
#define EC3D_CHUNK 64 /* sliced-ELL slice height = one wavefront */
#define EC3D_OUT_SLOTS 3 /* pinned host buffers of the overlapped field output (ec3d_vtk_fields_begin) */
#ifndef EC3D_PX
#define EC3D_PX 128   /* 2-D tile (patch) of the z-marching kernels: cells along x (one wave = one patch row) ... */
#endif
#define EC3D_PY (EC3D_TILE / EC3D_PX) /* ... and along y */

// ---------------------------------------------------------------------------------------------
// Device format.  Rows [0, n_pad).  Row r of A is
//     sum_b band[b][r] * x[r + off[b]]   (bands in ascending offset order)
//   + sum_j tval[...] * x[tcol[...]]     (tail entries of row r, in stored order)
// which is the reference's ascending-column summation order (src/solvers.f90:59 after full_sort,
// src/EC3D.f90:715) whenever every tail column of a row exceeds its band columns; rows that
// violate that are stored entirely in the tail (their band coefficients are zero).
struct MatView {
    const double *band[EC3D_MAXB];
    int64_t off[EC3D_MAXB];
    int nb;
    int has_tail;
    const int32_t *tail_id;   // [n_pad]  -1 or index of the row's tail slot
    const uint8_t *tile_flag; // [ntiles] 1 when any row of the tile has a tail
    const int64_t *chunk_ptr; // [nchunk+1] entry offsets of the 64-row slices
    const int32_t *tcol;      // 0-based column
    const double *tval;
    // dictionary form of the bands (ncls > 0): band[b][r] == table[cls[r] * nb + b]
    const uint8_t *cls; // [n_pad]
    const uint8_t *cls_same; // per 2-D tile: its classes equal those of the tile below (DevMatrix::cls_same); or null
    const double *table;
    int ncls;
    int pm1; // bands 2 and 4 of a 7-band operator are the offsets -1 and +1
    // Structured A-V form (sav != 0): unknowns [Ax | Ay | Az | U] with U EMBEDDED in the grid (one U
    // slot per cell, 4*nC rows), so the A<->U couplings are fixed-offset stencil slots too and there is
    // no tail.  A class = 7 band coefficients + 9 coupling coefficients (table stride 16):
    //   row of block d < 3, classes [sav_a0, sav_u0): + sum_{m=-2..2} t[7+m+2] * x[r + (3-d)*nC + m*step_d]
    //   row of block 3,     classes [sav_u0, sav_zero): sum_{d,j} t[7+3d+j] * x[r - (3-d)*nC + (j-1)*step_d]
    //                       added BEFORE the bands (the A columns are the lower ones)
    int sav;
    int sav_a0, sav_u0, sav_zero;
    int64_t sav_nC, sav_step[3];
};

// where a kernel finds the partial sums it has to finish: value i of slot s is
// base[s * slot_mul + i * stride], i < count.  Single GPU: the producer's per-workgroup partials
// (count = nblk, stride = 1, slot_mul = nblk).  Multi rank: the all-gathered per-rank sums
// (count = nranks, stride = P_NSLOT, slot_mul = 1).  In-library multi-GPU (ec3d_multi.hip): no gathered
// copy at all -- ptrs[i] is rank i's own lsum[P_NSLOT], read in place through the peer mapping
// (value i of slot s = ptrs[i][s]).
struct RedSrc {
    const double *base;
    int count, stride, slot_mul;
    const double *const *ptrs;
};

// blockIdx -> tile map (XCD aware when S > 0): see ec3d_tile_of() in ec3d_kernels.hip
struct Sweep {
    int64_t ntiles; // LOGICAL tiles of the front sweep (see win_* below); the U-block list comes behind them
    int64_t n; // rows owned; rows in [n, ntiles*EC3D_TILE) are padding
    int nblk;
    int S;
    int nt;      // nontemporal policy for once-touched streams (large problems)
    int vec_depth; // vector kernels: tiles whose operands are requested together (1, 2, 4)
    int pstride; // doubles between two slots of the partial-sum buffer
    // z-marching map of the SpMV kernels (zm_tpp > 0): a workgroup owns one 512-row position of the
    // xy-plane ("column") and walks zm_pps consecutive planes, so x[r-kdz], x[r] stay in registers
    int zm_tpp;  // tiles per plane = kdz / 512
    int zm_pps;  // planes per z segment
    // 2-D tiles of the z-marching single-component kernels (patch_npx > 0): a tile is a patch of EC3D_PX x EC3D_PY
    // cells of the xy plane instead of 512 consecutive cells; tile q of a plane is patch (q % patch_npx, q / patch_npx),
    // thread t owns cells 2 (t % (EC3D_PX/2)) and the next one of the patch's row t / (EC3D_PX/2).  See patch_pair in
    // ec3d_kernels.hip.
    int patch_npx;  // patches per grid row = sdx / EC3D_PX
    int64_t patch_sdx;
    // Runtime-shaped 2-D tiles of the z-marching STRUCTURED A-V kernels (rp_px > 0; sav_patch_step in
    // ec3d_kernels.hip): a tile is a patch of rp_px x rp_py cells (rp_px even, a divisor of the grid's sdx,
    // rp_px * rp_py <= 512) of one xy plane of one block; zm_tpp = rp_npx * ceil(rp_sdy / rp_py) patches per plane,
    // patch q of a plane is (q % rp_npx, q / rp_npx); thread t owns cells 2t, 2t + 1 of the patch in row-major order
    // (threads with 2t >= rp_px * rp_py, and rows beyond rp_sdy in the last patch row, idle).  A plane of a block
    // starts every rp_pitch device rows (the structured form's plane pitch), so tile T = P * zm_tpp + q lies in
    // plane P of the four stacked blocks.  rp_flag[T]: some row of the A-block patch T is coupled to U.
    int rp_px, rp_py, rp_npx, rp_sdy;
    int64_t rp_sdx, rp_pitch;
    const uint8_t *rp_flag;
    // rows that count in the dot products when this handle holds an A-V slab on an extended grid whose planes
    // are NOT tile aligned (nown > 0; bands + tail, or the structured form on a small grid): [Ax | Ay | Az | U]
    // each contribute one owned index range.  Tile-aligned structured slabs use the window below instead.
    int nown;
    int64_t own_lo[4], own_hi[4];
    // Window (structured A-V slab with tile-aligned planes, win_nt > 0): a block of the device layout holds
    // win_blk tiles (all held planes), of which the win_nt tiles from win_t0 on are OWNED; the halo planes'
    // rows are read (neighbours' values) but never swept: no kernel computes or stores there and every swept
    // row counts in the dot products.  Logical tile L of the front sweep is physical tile
    // (L / win_nt) * win_blk + win_t0 + L % win_nt; the same in planes (tiles / zm_tpp) for the z-march.
    int64_t win_nt, win_blk, win_t0;
    // split launches of the SpMV kernels in a z-slab, so the halo exchange overlaps the interior:
    // zm_pl0 > 0: z-march over planes [zm_pl0, zm_pl0 + zm_npl) only (interior launch);
    // bnd_last >= 0: the launch covers planes 0 and bnd_last only (boundary launch, plain tile order)
    int zm_pl0, zm_npl;
    // zm_plstep > 1: the launch covers the logical planes zm_pl0, zm_pl0 + zm_plstep, ... (zm_npl of them), one plane per
    // workgroup step sequence (zm_pps = 1): the boundary launch of the 2-D-tile kernels in a z-slab -- planes 0 and np-1
    int zm_plstep;
    int bnd_last;  // -1: not a boundary launch
    // z-slab of the single-component operator running the three-launch iteration (K2 inside K3, K5 inside the next K1):
    // S and P are FORMED on the halo planes by the kernels that need them there, and stored into the vectors' ghost rows
    // for the next kernel's stencil (K4 in SpMV form reads S one plane away; the next K5-in-K1 reads the old P there).
    // bit 0: this slab has a lower z-neighbour (store the plane below plane 0), bit 1: an upper one (above the last plane)
    int halo_store;
    int part_off;  // first partial-sum index this launch writes within a slot
    // structured A-V form: tiles [0, ntiles) are swept as usual (the three A blocks); of the tiles
    // behind them (the grid-shaped U block) only those holding an unknown are visited, from a list --
    // everything else there is identically zero in every vector and stays so
    const int32_t *ulist;
    int ulist_n;
    // INTERLEAVED z-march of the structured A-V form (il_planes > 0; single-rank handle, tile-aligned planes; walk_zm_il in
    // ec3d_kernels.hip): a workgroup owns one column and a range of xy planes k of ONE block's extent, and at every plane
    // visits the tiles of A_x, A_y, A_z there and -- when it holds an unknown -- the U tile, before it moves to plane
    // k + 1.  The coupling operands of a row (U next to an A row's cell, A_x / A_y / A_z next to a U row's cell,
    // src/EC3D.f90:656-711, :766-959) are then lines the same workgroup (or its XCD neighbour) fetched within the last
    // step or two: they come out of the L2 instead of HBM.  il_planes = planes per block, il_umask = one bit per
    // (column, plane): word col * il_nw + plane / 32; the trailing U list is empty (ulist_n = 0).
    int il_planes = 0, il_nw = 0;
    const uint32_t *il_umask = nullptr;
    // the march's work list: workgroup b takes planes [il_seg[4 b + 1], il_seg[4 b + 2]) of column il_seg[4 b] (an empty range:
    // nothing).  Cut by WEIGHT (a plane with a U tile costs more than one without), per column, the columns of XCD label x =
    // b % 8 being its cpx adjacent ones, so that every workgroup of the launch ends at about the same time.
    const int32_t *il_seg = nullptr;
    // Paired patch columns (2-D tiles; ec3d_patch_pairs_ok in ec3d_sweep_lists.hpp): the launch kinds (EC3D_PAIR_* bits)
    // that run nblk / 2 workgroups of 512 threads, each hosting two y-adjacent workgroups of the nblk this sweep counts.
    // nblk, the partials, the visit order and the tile lists keep speaking of those nblk "virtual" workgroups.
    int pair = 0;
    // K5-in-K1 forms AP_old inside the patch instead of loading it (undivided dictionary cube on 2-D tiles; choose_sweep's
    // policy, EC3D_K51_AP; ec3d_form_apc in ec3d_form.hpp)
    int k51_ap = 0;
};

// first of the two consecutive rows thread t of a workgroup owns in `tile`
template <class SW>
__host__ __device__ inline int64_t ec3d_row_of(const SW &sw, int64_t tile, int t)
{
    if (sw.patch_npx <= 0) return tile * EC3D_TILE + 2 * (int64_t)t;
    const int64_t plane = tile / sw.zm_tpp, q = tile % sw.zm_tpp;
    const int64_t py = q / sw.patch_npx, px = q % sw.patch_npx;
    return plane * (int64_t)sw.zm_tpp * EC3D_TILE + (py * EC3D_PY + t / (EC3D_PX / 2)) * sw.patch_sdx + px * EC3D_PX +
           2 * (int64_t)(t % (EC3D_PX / 2));
}

// logical -> physical tile of the front sweep (identity without a window)
template <class SW>
__host__ __device__ inline int64_t ec3d_phys_tile(const SW &sw, int64_t t)
{
    if (sw.win_nt <= 0) return t;
    return (t / sw.win_nt) * sw.win_blk + sw.win_t0 + t % sw.win_nt;
}

// blockIdx -> tile map of a sweep (host and device: ec3d_get_visit_order enumerates with the same function).
// Returns the PHYSICAL tile, or -1 when workgroup b has no i-th tile in the front sweep.
// MODE: -1 = decide from the sweep's fields (host enumeration, vector kernels); 1 = the z-marching map is known to
// apply; 0 = it is known not to.  (The z-marching SpMV kernels walk the same sequence incrementally,
// EC3D_ZSWEEP in ec3d_kernels.hip: plane after plane of one column, restarting at every block of a windowed slab.)
template <int MODE = -1, class SW = Sweep>
__host__ __device__ inline int64_t ec3d_tile_of(const SW &sw, int b, int64_t i)
{
    if (MODE != 1 && sw.bnd_last >= 0) {
        // boundary launch of a z-slab: the first and the last owned plane, plain tile order
        const int64_t t = i * (int64_t)sw.nblk + b;
        if (t >= 2 * (int64_t)sw.zm_tpp) return -1;
        return (t < sw.zm_tpp ? 0 : (int64_t)sw.bnd_last * sw.zm_tpp) + t % sw.zm_tpp;
    }
    if (MODE == 1 || (MODE == -1 && sw.zm_tpp > 0)) {
        // XCD label c owns zm_tpp/8 adjacent columns, so the +-sdx lines a column needs were fetched
        // by a neighbour on the same XCD one step earlier (L2 hit); logical plane k = pl0 + seg*pps + i
        const int cpx = (sw.zm_tpp + 7) >> 3, c = b & 7, s = b >> 3;
        const int64_t col = c * cpx + s % cpx, seg = s / cpx;
        const int64_t pl = seg * sw.zm_pps + i;
        if (col >= sw.zm_tpp || i >= sw.zm_pps || (sw.zm_npl > 0 && pl >= sw.zm_npl)) return -1;
        const int64_t t = (sw.zm_pl0 + (sw.zm_plstep > 1 ? pl * sw.zm_plstep : pl)) * sw.zm_tpp + col;
        return t < sw.ntiles ? ec3d_phys_tile(sw, t) : -1;
    }
    int64_t t;
    if (sw.S > 0) {
        int64_t c = b & 7, s = b >> 3;
        t = (i * 8 + c) * sw.S + s;
    } else {
        t = i * (int64_t)sw.nblk + b;
    }
    return t < sw.ntiles ? ec3d_phys_tile(sw, t) : -1;
}

// A kernel of a z-slab as two launches, so that the halo exchange overlaps the interior: `bnd` visits the tiles next to a
// cut, `inte` all others, each tile in exactly one of them.  Every pair is derived in ec3d_split_sweeps.hpp (host only; the
// record lives here because ec3d_ctx holds three).  !ok: the kernel runs unsplit.
struct SplitSweep {
    Sweep bnd{}, inte{};
    bool ok = false;
    // partial sums per slot the two launches leave: one's, from its part_off = 0, followed by the other's
    int parts() const { return bnd.nblk + inte.nblk; }
};
#define EC3D_XD_MAX 4 // deepest deferral of the X update (iterations whose P and S are kept)
struct SolverState {
    double rr0[2]; // R·R0 entering iteration it is rr0[it & 1]
    double alpha, omega;
    double bnorm, tol;
    double rnorm;  // ||R|| of the last iteration that got as far as its K5 (what the itmax exit prints, solvers.f90:27)
    int stop_iter; // INT_MAX while running; iteration at which an exit was taken
    int stop_kind; // 1: ‖S‖ exit (solvers.f90:34-38), 2: ‖R‖ exit (:43), 0: none / ‖b‖ = 0
    int restarts;  // times the restart R0 = R, P = R (solvers.f90:47-49) fired in this solve (ec3d_get_restart_count)
    int pad_;
    // X updates not applied yet (k4d_x_r_update): alpha, omega of the pending iterations, oldest first
    // (two groups' worth: with the groups applied by a kernel of their own beside the iteration -- ec3d_xasync -- the
    // entry of iteration it is it % (2 D), and group g + 1 fills its half while group g's kernel still reads the other)
    double pend_alpha[2 * EC3D_XD_MAX], pend_omega[2 * EC3D_XD_MAX];
    int npend;     // how many
    int pend_half; // the newest one is the ||S|| exit's X = X + alpha*P (no omega*S term)
};

// host-side image of the format (CSR conversion / export)
struct HostMatrix {
    int64_t n = 0, n_pad = 0, nnz = 0;
    int nb = 0;
    int64_t off[EC3D_MAXB] = {0};
    std::vector<double> bands;      // nb * n_pad
    std::vector<int32_t> tail_id;   // n_pad
    std::vector<uint8_t> tile_flag; // n_pad / EC3D_TILE
    int64_t ntail = 0;
    std::vector<int64_t> chunk_ptr;
    std::vector<int32_t> tcol;
    std::vector<double> tval;
    // dictionary form (ncls > 0): `bands` may then be empty
    std::vector<uint8_t> cls;
    std::vector<double> table;
    int ncls = 0;
};

// host-side image of the structured A-V form recognised in a CSR matrix (ec3d_sav_csr.cpp)
struct SavHost {
    int64_t n_ref = 0, n_dev = 0, n_pad = 0, nnz = 0;
    int64_t sdx = 0, plane = 0, pitch = 0, nCd = 0;
    int a0 = 0, u0 = 0, zero = 0, ncls = 0;
    std::vector<uint8_t> cls, tile_flag;
    std::vector<double> table; // ncls * 16
    std::vector<int32_t> ulist, cond_cell;
    int64_t ntiles_front = 0;
    // a z-slab cut out of a recognised system (ec3d_sav_slice): rows of the halo planes are inert and only the
    // owned planes of each block count in the dot products (as ec3d_assemble_slab sets it up natively)
    int nown = 0;
    int64_t own_lo[4] = {0, 0, 0, 0}, own_hi[4] = {0, 0, 0, 0};
    int64_t halo = 0;
    int64_t u_first = 0; // index, among the whole system's U unknowns, of the slab's first held one
};

struct DevMatrix {
    int64_t n = 0, n_pad = 0, nnz = 0;
    int nb = 0;
    int64_t off[EC3D_MAXB] = {0};
    DevBuf<double> bands;
    DevBuf<int32_t> tail_id;
    DevBuf<uint8_t> tile_flag;
    int64_t ntail = 0, nchunk = 0, tail_entries = 0;
    DevBuf<int64_t> chunk_ptr;
    DevBuf<int32_t> tcol;
    DevBuf<double> tval;
    DevBuf<uint8_t> cls; // dictionary form (ncls > 0): bands is empty
    // dictionary form on a grid that divides into EC3D_PX x EC3D_PY patches: one byte per patch tile, 1 = every class
    // byte of the tile equals the one kdz rows below (ec3d_class_runs in ec3d_sweep_lists.hpp; made from `cls` once per
    // matrix by ec3d_build_class_runs, never a source of its own).  Empty: the kernels load the class bytes every step.
    DevBuf<uint8_t> cls_same;
    int64_t cls_same_n = 0; // flags (planes * tiles per plane; the buffer holds a plane of zeros more)
    DevBuf<double> table;
    int ncls = 0;
    // structured A-V form (see MatView)
    int sav = 0, sav_a0 = 0, sav_u0 = 0, sav_zero = 0;
    bool sav_box = false; // classes 0 .. 26 are box positions tx + 3 ty + 9 tz (ec3d_assemble; not a form read from CSR)
    DevBuf<int32_t> ulist; // tiles of the U block that hold at least one unknown
    int ulist_n = 0;
    std::vector<int32_t> ulist_host; // host copy for the visit-order export
    // the same for runtime-shaped 2-D tiles (Sweep::rp_*), made by choose_sweep for the shape it picked
    int rp_px = 0, rp_py = 0;
    DevBuf<uint8_t> rp_flag;               // per patch tile of the three A blocks: coupled
    std::vector<int32_t> rp_ulist_host;    // patch tiles of the U block that hold an unknown, ascending
    int64_t ntiles_front = 0; // tiles swept unconditionally
    int64_t sav_nC = 0, sav_step[3] = {0, 0, 0};
    int64_t bytes = 0;
    MatView view() const;
};

struct ec3d_mg; // multigrid hierarchy (ec3d_mg.hip)
// beta and the restart decision of the outer iteration (ec3d_outer.hip), left on the device by k_mg_scalar
struct MgScalars {
    double beta;
    int restart;
    int pad_;
};

// Tables of ec3d_domain_integrals (ec3d_integrals.hip), made with the RHS tables of an undivided A-V handle: the
// conducting domains in ascending id order and the conductor cell list sorted by (domain id, scan order), cut into
// chunks that never straddle a domain.
struct DomIntegrals {
    int ndom = 0;
    int64_t nchunk = 0;
    std::vector<int32_t> id;    // [ndom] geoPHYS id
    std::vector<int64_t> cells; // [ndom] conductor cells of the domain
    std::vector<double> C;      // [ndom] valPHYS(id, 2) = mu0 * sigma
    DevBuf<int32_t> cell;       // [n_cond] 0-based DEVICE cell index (dev_cell)
    DevBuf<int32_t> chunk;      // [nchunk][3] first entry, entries, domain ordinal
    DevBuf<int32_t> dom_chunk;  // [ndom + 1] first chunk of every domain
    DevBuf<double> partial;     // [nchunk][4] sums of q, fx, fy, fz per chunk
    DevBuf<double> sums;        // [ndom][4]
    PinnedBuf<double> host;     // [ndom][4] where the call's one copy lands
};

// Tables of ec3d_domain_linkage: the same for the domains that hold cells outside the conductors (the coils, the plain
// bodies and the air).  Built on the host at assembly; the device buffers are made by the first call, which frees the
// host lists.
struct DomLinkage {
    bool built = false;
    int ndom = 0;
    int64_t nchunk = 0;
    std::vector<int32_t> id;    // [ndom] geoPHYS id
    std::vector<int64_t> cells; // [ndom] non-conducting cells of the domain
    std::vector<int32_t> cell_host, chunk_host, dom_chunk_host; // until the first call
    DevBuf<int32_t> cell, chunk, dom_chunk;
    DevBuf<double> partial;     // [nchunk][4] sums of A.J, Jx, Jy, Jz per chunk
    DevBuf<double> sums;        // [ndom][4]
    PinnedBuf<double> host;
};

// What ec3d_field_energy keeps, made by its first call: one byte per device cell (1 inside a conductor; none without
// conductors), the workgroups' partials and the five sums.
struct FieldEnergy {
    int wgs = 0;
    DevBuf<uint8_t> cond;
    DevBuf<double> part, sums;
    PinnedBuf<double> host;
};

// The probe set of ec3d_set_probes (ec3d_probes.hip): the cells resolved to device cells and U rows, the buffer of the
// immediate sample and the record that stays on the device.  Belongs to the matrix (ec3d_free_matrix).
struct Probes {
    int64_t n = 0, capacity = 0, recorded = 0;
    DevBuf<int32_t> cell;   // [n] 0-based DEVICE cell index (dev_cell)
    DevBuf<int32_t> urow;   // [n] device row of the cell's U unknown (ec3d_get_row_map's), -1 outside the conductors
    DevBuf<double> sample;  // [13][n] what ec3d_probe_sample copies out
    DevBuf<double> record;  // [capacity][13][n]
    std::vector<double> T;  // [recorded] the caller's time of every record
};

// The host's cursor of a run of iterations.  The device state is addressed by the iteration number (rr0[it & 1], AP in
// apbuf[it & 1], P and S in their rings), so the host keeps in step with it here and nowhere else: ec3d_run_reset starts
// a run, ec3d_run_open says which iterations a call launches, ec3d_after_s / ec3d_after_p advance it behind a launch
// (ec3d_solve.hip); a default-constructed cursor IS the state of a run that has just begun.
struct IterCursor {
    int p_off = 0;         // P(it) lives in pbuf[(it + p_off) % pdepth] (0: iterations are numbered from the last ec3d_run_reset)
    int it_next = 1;       // the iteration the next launch has to be: ec3d_iterate / ec3d_multi_iterate must continue where the last call ended
    int xd_base = 1;       // the iteration the groups of D are counted from (1 in a solve; ec3d_iterate: its first_iter)
    int xd_last = INT_MAX; // the last iteration the present call is going to launch: it applies whatever is pending
    int pcur = 1;          // which P buffer holds the CURRENT P (what ec3d_download and ec3d_device_vector hand out)
    int apcur = 1, scur = 1; // the same for AP and S (a run begins with P = R in vec[P] = pbuf[1])
    int ap_valid_for = 0;  // K5-in-K1: the iteration whose AP = A P the last K51 launch already produced (0: none)
    int ss_parts = 0;      // z-slab: workgroup partials of S.S that K2 left for K3's collapse launch to fold (0: none pending)
    int xg_n = 0;          // groups of X updates launched since the last ec3d_run_reset
    int xg_done_upto = 0;  // the last iteration whose X update an enqueued k_x_group covers
    void forget_ap() { ap_valid_for = 0; } // the next stage 1 launches K1 on its own (ec3d_time_kernel)
};

// ec3d_set_guess_history (ec3d_guess.hip): the pairs (Q_i, A Q_i) a solve is started from.  Library-owned vectors of n_pad
// doubles -- no ghosts: no stencil reads them -- outside the work vectors' block, allocated by the first solve after the depth
// was set; pair i (oldest first) lives in slot (head + i) % depth.  The depth belongs to the handle, the pairs to the matrix.
struct GuessHistory {
    int depth = 0;       // m: 0 = off
    int k = 0, head = 0; // pairs stored, slot of the oldest
    std::vector<DevBuf<double>> q, aq;
    DevBuf<double> xs;   // X as the solve found it
    DevBuf<double> part; // per-workgroup partials, (EC3D_GUESS_MAX_DEPTH + 1) slots of wgs
    DevBuf<double> scal; // the solve's scalars (GS_* in ec3d_guess.hip) ...
    PinnedBuf<double> host; // ... and where the one copy per solve lands
    int64_t len = 0;     // doubles per vector (0: nothing allocated)
    int wgs = 0;         // workgroups of the streaming launches
    ec3d_guess_info last{}; // what ec3d_get_guess_history reports
};

// ec3d_set_null_projection (ec3d_null.hip): the orthonormal left null vectors Q of the structured A-V matrix, one per
// conducting component kept.  Library-owned vectors of n_pad doubles, no ghosts (the transposed kernel tests its
// source rows instead of reading zeros), vector i at q + i * len.  The setting belongs to the handle, Q to the matrix.
struct NullProjection {
    int on = 0;
    double null_tol = 1e-10;
    bool built = false;
    int kept = 0;
    int64_t len = 0;
    DevBuf<double> q;
    DevBuf<double> part, coef; // per-workgroup partials (kept slots of wgs), the collapsed sums
    DevBuf<double> kpart;      // the adjoint iteration's partials (ec3d_outer_begin)
    DevBuf<MgScalars> kscal;
    int wgs = 0;
    ec3d_null_info last{};
    // ec3d_set_null_precond: N of the adjoint solves.  The setting stays with the handle; the hierarchy lives inside one
    // set-up only, what it looked like is kept for ec3d_get_null_precond
    int precond = EC3D_NULL_PRECOND_NONE, pre = 0, post = 0, coarse = 0;
    int32_t levels = 0, dims[3 * EC3D_NULL_PRECOND_MAX_LEVELS] = {0};
    double hierarchy_ms = 0.0;
};

// ec3d_harmonic_* (ec3d_harmonic.hip): the time-harmonic operator K + j omega M on the class bytes
// of the structured A-V form.  re and m are made by every ec3d_assemble (k_build_table_harmonic beside
// k_build_table_sav: the transient table without its dt terms, and the unit imaginary table); everything else by
// ec3d_harmonic_setup and ec3d_harmonic_batch_setup only.  Belongs to the matrix (ec3d_free_matrix).
enum { HV_X = 0, HV_B, HV_R, HV_R0, HV_P, HV_AP, HV_S, HV_AS, HV_N };
struct HarmonicState; // the solve's scalars and exit words on the device (ec3d_harmonic.hip)

// The left null vectors of a HarmonicSystems (DESIGN sections 18a, 18c): one orthonormal set per DISTINCT omega, found by
// adjoint solves that run in lock step in the work vectors, partials and states of the systems 0 .. sets - 1.  The
// setting (on, tol) belongs to the handle, everything else to the systems AND their omegas.
struct HarmonicNull {
    int on = 0;
    double tol = 1e-10;
    bool built = false;
    int sets = 0, ncomp = 0;                     // ncomp: the conducting components, the room of a set
    int set_of[EC3D_HARMONIC_MAX_BATCH] = {0};   // system -> set
    int first[EC3D_HARMONIC_MAX_BATCH] = {0};    // set -> its lowest system
    int kept[EC3D_HARMONIC_MAX_BATCH] = {0};     // per set
    DevBuf<double> q;          // vector i of set d: the n_pad pairs at q + (d * ncomp + i) * 2 * n_pad
    DevBuf<double> y, tab;     // the batch only: per set the unknown of its adjoint solve and the table of its omega
    DevBuf<double> part, coef; // per SYSTEM [2 * ncomp * wgs] partials of its coefficients' parts, [2 * ncomp] coefficients
    int64_t bytes = 0;
    double removed[EC3D_HARMONIC_MAX_BATCH] = {0.0};     // per system, of its last projection
    ec3d_null_info last[EC3D_HARMONIC_MAX_BATCH] = {};   // per set
    int32_t restarts[EC3D_HARMONIC_MAX_BATCH][EC3D_NULL_MAX_REPORT] = {{0}}; // of the adjoint solves, per set (tests)
};

// n systems (omega_s, b^_s, x^_s) solved in lock step: system s has its HV_N vectors of n_pad (re, im) pairs (device
// numbering, no ghosts) at vec + s * HV_N * 2 * n_pad, its table of [ncls * 16] (re, omega_s * m) pairs at
// tab + s * 2 * ncls * 16, its per-workgroup partial sums at part + s * HP_NSLOT * wgs, and state[s].
struct HarmonicSystems {
    int n = 0;
    double omega[EC3D_HARMONIC_MAX_BATCH] = {0.0};
    DevBuf<double> vec, tab, part;
    DevBuf<double> stage; // [2 * n_pad] a real and an imaginary part in device numbering (host copies)
    DevBuf<HarmonicState> state;
    int wgs = 0;
    int64_t bytes = 0;
    ec3d_harmonic_info last[EC3D_HARMONIC_MAX_BATCH] = {};
    HarmonicNull null;
};

// one: the system of ec3d_harmonic_setup (n = 1 once it ran), which keeps its vectors across omegas.  batch: the
// systems of ec3d_harmonic_batch_setup, storage of their own that every set-up makes anew;
// ec3d_harmonic_setup leaves it alone.
struct Harmonic {
    DevBuf<double> re, m; // [ncls * 16] each
    HarmonicSystems one, batch;
};

struct ec3d_ctx {
    int device = 0;
    hipStream_t stream = nullptr;         // the stream every launch goes to
    Stream own_stream_obj;                // created by ec3d_create; `stream` may point elsewhere (and is never destroyed here)
    DevMatrix A;
    bool have_matrix = false;
    int64_t ghost = 0;     // zero halo (doubles) on both sides of every vector
    // The work vectors.  vec_own holds them when they are the handle's; it is EMPTY while the handle works on vectors the
    // caller gave it (ec3d_adopt_vectors).  vec_base / vec[] are what everything else uses: a view, never freed.
    DevBuf<double> vec_own;
    double *vec_base = nullptr;
    double *vec[8] = {nullptr};
    bool own_vectors() const { return vec_base == vec_own.get(); } // (also true while there are none)
    Sweep sweep{};   // vector kernels: K4's grid (and the geometry every other sweep is derived from)
    Sweep sweep_k2{}, sweep_k5{}; // K2 (2 reads + 1 write) and K5 (3 + 1) like other workgroup counts than K4 (5 + 2)
    Sweep sweep_s{}; // SpMV kernels (K1, K3, residual, spmv)
    // z-slab: the kernels that run as boundary + interior launch (SplitSweep; ec3d_split_sweeps.hpp derives all three).
    // While a split is refused, split_s and split_f hold the unsplit sweep_s twice.
    SplitSweep split_s; // K1 and K3 (ec3d_can_overlap): the planes next to a cut / those between
    // on 2-D tiles: planes {0, np-1} / 1 .. np-2 as two launches of the 2-D-tile kernels (K4 in SpMV form and K5-in-K1 of
    // the three-launch iteration: the producers of the exchanged R and AP)
    SplitSweep split_f;
    // K2 and K5, made by ec3d_dist_set_boundary_rows (tile lists: vb_list, vi_list) or ec3d_dist_set_boundary_planes
    // (windows) after the matrix is set, and dropped (ok = false, the sweeps left as they were) whenever the geometry changes
    SplitSweep split_v;
    bool fuse23_ok = false; // 2-D tiles: K2 may run inside K3 (single rank only, see ec3d_fused23)
    bool fuse51_ok = false; // 2-D tiles: K5 may run inside the next iteration's K1 (ec3d_fused51)
    bool k4s_ok = false;    // dictionary cube on 2-D tiles: K4 may run as an SpMV kernel that computes A S again (ec3d_k4s)
    // z-slab of a multi-rank job (set by the job's driver once EVERY rank can do it: the exchanges differ, so the plan is a
    // property of the job): the three-launch iteration on this slab (AP and R are exchanged instead of P and S, see
    // Sweep::halo_store); the X update deferred over slab_xd iterations (0: not on this slab)
    bool slab_fused = false;
    int slab_xd = 0;
    IterCursor run; // where the iterations of this handle stand (host side)
    // K5-in-K1 reads the previous iteration's P and AP while it writes the new ones (neighbouring workgroups read the
    // old values of cells this one owns), so both vectors alternate between two buffers: P(it) lives in
    // pbuf[it & 1], AP(it) in apbuf[it & 1]; index 1 is vec[EC3D_VEC_P] / vec[EC3D_VEC_AP], index 0 the spare pair
    // With the X update deferred over D iterations (k4d_x_r_update; only together with both fusions) P(it) lives in
    // pbuf[it % D] and S(it) in sbuf[it % D] (index 1 = vec[EC3D_VEC_P] / vec[EC3D_VEC_S]); AP keeps its two buffers.
    DevBuf<double> pp_base;
    int64_t pp_len = 0;    // doubles allocated at pp_base
    double *pbuf[2 * EC3D_XD_MAX] = {nullptr}, *sbuf[2 * EC3D_XD_MAX] = {nullptr}, *apbuf[2] = {nullptr, nullptr};
    int pdepth = 2;        // buffers P cycles through (2, or D; 2 D with the X groups on a stream of their own)
    int sdepth = 1;        // buffers S cycles through (D; 2 D with the X groups on a stream of their own)
    int ring_cap = 0;      // ring buffers allocated for each of P and S (ec3d_spare_pair): D, or 2 D
    // The groups of D pending X updates applied by a kernel of their own (k_x_group) on a second, low-priority stream,
    // beside the following iterations, instead of by every D-th K4: nothing in the loop reads X, so the work fills what
    // the iteration leaves idle -- on a z-slab the waits for halo planes and reduced sums (ec3d_xasync)
    bool xasync_cap = false;  // the rings hold two groups (2 D buffers each)
    bool xasync_forced = false; // EC3D_XASYNC=2: also on a handle that is no slab (tests)
    bool slab_xasync = false; // a z-slab: the job's driver said so (every rank the same ring depth)
    // ... or as launches of their own on the iteration's OWN stream, behind the K4 of each group's last iteration (rings of one
    // group suffice): the undivided handle's three-launch iteration, where K4 in SpMV form with ten more operand streams in
    // the applying launch ran 18 % over what its bytes allow and a light K4 + one streaming launch per group do not
    bool xinline = false;
    Stream xstream;
    Event ev_xready, ev_xdone[2];
    // first failed runtime call of a launcher that cannot return a status (ec3d_launch_x_group_of sits inside the void stage
    // launchers): noted there, turned into an error code by whoever checks the stage's launches (EC3D_ASYNC_CHECK)
    hipError_t async_err = hipSuccess;
    const char *async_what = nullptr;
    int xdefer = 1;        // D: iterations between two X updates on this handle (1: every iteration, the classic K4)
    DevBuf<int32_t> vb_list, vi_list; // split_v from tile lists (ec3d_dist_set_boundary_rows): the lists on the device
    DevBuf<int32_t> us_list; // structured form: the U tiles in the order the z-marching SpMV kernels take them (choose_sweep)
    DevBuf<int32_t> ii_list, ib_list; // structured z-slab, K1 / K3 split: the interior launch's U tiles, the boundary launch's tiles
    std::vector<int32_t> us_host; // host copy (visit-order export)
    DevBuf<uint32_t> il_umask;         // interleaved z-march of the structured form (Sweep::il_*): one bit per (column, plane)
    std::vector<uint32_t> il_umask_host;
    DevBuf<int32_t> il_seg;            // ... and its work list (four int32 per workgroup)
    std::vector<int32_t> il_seg_host;
    int nown = 0;    // ownership ranges of an A-V slab (see Sweep)
    int64_t own_lo[4] = {0}, own_hi[4] = {0};
    bool dist = false;
    // multi-rank (z-slab) mode: reductions come from the all-gathered per-rank sums
    int nranks = 1;
    // BORROWED: the caller's device buffers, never freed here and dropped with the matrix (ec3d_free_matrix)
    double *lsum = nullptr, *gsum = nullptr; // (P_NSLOT, nranks*P_NSLOT)
    const double *const *lsum_ptrs = nullptr; // device array of nranks pointers: every rank's lsum (ec3d_multi.hip)
    int64_t halo = 0;                        // doubles per halo plane (kdz), 0 when not a slab
    bool use_dict = true;
    bool use_sav = true;   // structured A-V form for ec3d_assemble when the problem allows it (EC3D_SAV)
    int64_t n_ref = 0;     // unknowns in the reference's numbering (what host vectors hold); = A.n unless sav
    // sav: every xy plane starts on a tile boundary (pitch >= plane cells, multiple of EC3D_TILE) so the
    // z-marching SpMV map always applies; plane == pitch == 0 otherwise.  Device cell of reference cell q:
    // (q / plane) * pitch + q % plane; a component block holds nCd = sdz * pitch device rows.
    int64_t plane = 0, pitch = 0, nCd = 0;
    int64_t dev_cell(int64_t q) const { return pitch == plane ? q : (q / plane) * pitch + q % plane; }
    int64_t ref_cell(int64_t p) const { return pitch == plane ? p : (p / pitch) * plane + p % pitch; }
    int64_t planes() const { return pitch ? nCd / pitch : 0; } // xy planes per component block
    DevBuf<double> io_tmp; // sav: staging for the U part of host<->device vector copies
    int nblk_request = 0;
    int nt_request = -1; // -1 auto, 0/1 forced (EC3D_NT)
    int zm_request = 1;  // z-marching SpMV map when the grid allows it (EC3D_ZMARCH)
    int shuffle_request = 1; // +-1 neighbours by lane shuffle (EC3D_SHUFFLE)
    DevBuf<double> partials; // 8 * nblk doubles
    DevBuf<SolverState> state;
    PinnedBuf<SolverState> state_pinned; // 2 slots
    DevBuf<double> hist;
    int64_t hist_cap = 0;
    Event ev[2];
    Event t0, t1;
    // assembly by-products (1-based ids, reference order)
    std::vector<int32_t> cel_bnd[6];
    // grid of the last native assembly (0 when the matrix came from CSR)
    int32_t sdx = 0, sdy = 0, sdz = 0;
    int64_t n_cells = 0; // cells this handle holds per component (a z-slab: its extended planes only)
    int32_t slab_e0 = 0, slab_k0 = 0, slab_k1 = 0; // global planes: first held, owned range [k0, k1)
    // per-step RHS build / post-update on the device (src/EC3D.f90:370-404, :412-433)
    int64_t n_cond = 0;            // conducting cells (U unknowns), scan order
    int n_cond_domains = 0;
    int64_t nu_siz_max = 0;        // max over conducting domains of the domain's cell count (PHYS_C%siznod)
    int u_rhs = 0;                 // EC3D_U_RHS_*: which U rows the RHS step gives their A-part (ec3d_set_u_rhs)
    DevBuf<int32_t> cond_cell;     // [n_cond] 0-based DEVICE cell index (dev_cell)
    DevBuf<double> cond_a;         // [n_cond] 2*C/dt of the cell's domain (PHYS_C%valdom)
    DevBuf<int32_t> bnd_list;      // the six cel_bnd* lists, 0-based unknown ids, concatenated
    int64_t bnd_off[7] = {0};
    DevBuf<double> rhs_tmp;        // [3*n_cond] scratch for the moving-source reset
    DevBuf<int32_t> src_idx;       // per-step source scatter staging
    DevBuf<double> src_val;
    int64_t src_cap = 0;
    DomIntegrals dom;              // per-domain integrals (ec3d_integrals.hip); freed with cond_cell
    DomLinkage link;               // ... of the non-conducting domains (ec3d_domain_linkage)
    FieldEnergy energy;            // ec3d_field_energy's buffers
    Probes probes;                 // ec3d_set_probes' cells and records (ec3d_probes.hip)
    // plain band streams whose placement was probed (place_bands): kept across a change of matrix of the same size, so
    // the probe runs once per handle and size, and what it found (candidate times in us, the one kept)
    DevBuf<double> placed_bands;
    size_t placed_bytes = 0;
    bool bands_placed = false; // A.bands is an allocation the probe chose (or was taken back from placed_bands)
    std::vector<float> place_us;
    int place_kept = -1;
    // the work vectors' placement (place_vectors): doubles per vector the probe last ran for (0: never), the candidates'
    // iteration times, which one was kept, what the search cost
    int64_t vplace_len = 0;
    DevBuf<double> parked_vec, parked_pp; // the chosen allocation between two matrices (ec3d_free_matrix)
    int64_t parked_pp_len = 0;
    std::vector<float> vplace_us;
    int vplace_kept = -1;
    float vplace_ms = 0.f;
    std::vector<uint64_t> src_seen; // host: one bit per A unknown, all zero between calls (repeat check of ec3d_rhs_step)
    // field output (ec3d_output.hip): device scratch for the four float32 vectors, the conductor mask, and -- for
    // output overlapped with the next time step -- a side stream with two pinned host buffers
    DevBuf<float> out_dev;
    int64_t out_cells = 0;
    DevBuf<int32_t> out_mask;
    PinnedBuf<float> out_pinned[EC3D_OUT_SLOTS];
    Stream out_stream;
    Event out_ev_fields, out_ev_free, out_ev_copied[EC3D_OUT_SLOTS];
    int out_next = 0;
    bool out_busy = false;
    unsigned out_started = 0;  // bit i: slot i has had an ec3d_vtk_fields_begin (its event is worth waiting for)
    // the matrix came from ec3d_assemble_poisson on the whole grid (what the multigrid hierarchy rediscretises), with
    // this BND and spacing; in_multi: the handle is a slab of ec3d_multi (no preconditioner there)
    bool poisson_full = false;
    double poisson_bnd[6] = {0, 0, 0, 0, 0, 0}, poisson_delta[3] = {0, 0, 0};
    bool in_multi = false;
    // the matrix came from ec3d_set_matrix_csr; precond_grid: the box the caller said it is a 7-point operator on
    // (ec3d_set_precond_grid; zeros: none).  Both belong to the matrix: ec3d_free_matrix clears them
    bool from_csr = false;
    int32_t precond_grid[3] = {0, 0, 0};
    ec3d_mg *mg = nullptr; // ec3d_set_preconditioner(EC3D_PRECOND_MG): solves run the preconditioned iteration
    int precond_precision = 0; // EC3D_PRECOND_FP64 / _FP32: what the next ec3d_set_preconditioner builds (ec3d_set_precond_precision)
    int precond_coarsening = 0; // EC3D_COARSEN_REDISCRETIZE / _AGGREGATE: likewise (ec3d_set_precond_coarsening)
    GuessHistory guess;
    NullProjection nullp;
    Harmonic harm;
    ec3d_ctx() = default;
    ~ec3d_ctx(); // ec3d_context.hip: the hierarchy goes (ec3d_mg_free), then every owner above, last declared first
};

// partial-sum slots inside ctx->partials (each nblk doubles)
enum { P_BB = 0, P_RR_INIT = 1, P_D1 = 2, P_SS = 3, P_D2 = 4, P_D3 = 5, P_RR = 6, P_RR0N = 7, P_NSLOT = 8 };

void ec3d_set_error(const std::string &msg);
// a REAL(8) as the reference's `print*` writes it (src/solvers.f90:27, flang's list-directed output); buf >= 40
void ec3d_format_list_directed(double v, char *buf);
// the same value as gfortran's list-directed output writes it (one blank + G25.17E3); buf >= 40
void ec3d_format_list_directed_gfortran(double v, char *buf);
// the itmax exit's line: norm2(R) on stdout, as the reference prints it (src/solvers.f90:27, `print*`).  List-directed
// output is compiler specific: flang's form by default (the toolchain of this image, which built oracle/_ref),
// EC3D_PRINT_STYLE=gfortran for the form of the reference's own Makefile (src/Makefile:1-28)
void ec3d_print_rnorm(double rnorm);
// itmax exit: the reference prints norm2(R) (src/solvers.f90:25-28).  When this points somewhere, the solve entry
// points store the value there instead of printing it (the drop-in prints it once its result is accepted).
extern thread_local double *ec3d_itmax_print_hold;
#define EC3D_HIP(call)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            ec3d_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                 \
            return 100;                                                                        \
        }                                                                                      \
    } while (0)
// a runtime call inside a launcher without a status of its own: the first failure is kept in the context ...
#define EC3D_NOTE(c_, call)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess && (c_)->async_err == hipSuccess) {                               \
            (c_)->async_err = e_;                                                              \
            (c_)->async_what = #call;                                                          \
        }                                                                                      \
    } while (0)
// ... and reported where the stage's launches are checked
#define EC3D_ASYNC_CHECK(c_)                                                                   \
    do {                                                                                       \
        if ((c_)->async_err != hipSuccess) {                                                   \
            ec3d_set_error(std::string((c_)->async_what) + ": " + hipGetErrorString((c_)->async_err)); \
            (c_)->async_err = hipSuccess;                                                      \
            return 100;                                                                        \
        }                                                                                      \
    } while (0)

// ec3d_format.cpp
int ec3d_csr_to_host_matrix(int64_t n, const double *valA, const int32_t *irow, const int32_t *jcol,
                            HostMatrix &M);
// native assembly's grid for ec3d_host_matrix_to_csr: an A row keeps the entry of every neighbour inside the box, even
// where its coefficient is 0.0 (a boundary value of 0: the reference stores that zero, src/EC3D.f90:528-646)
struct CsrGrid {
    int64_t sdx, sdy, sdz, cells; // global grid; cells held per component
    int64_t e0, k0, k1;           // first plane held; owned planes [k0, k1)
};
void ec3d_host_matrix_to_csr(const HostMatrix &M, std::vector<int32_t> &irow, std::vector<int32_t> &jcol,
                             std::vector<double> &valA, const CsrGrid *grid = nullptr);

// ec3d_sav_csr.cpp: 0, or -1 when the matrix does not have the structure
int ec3d_csr_to_sav_host(int64_t n, const double *valA, const int32_t *irow, const int32_t *jcol, SavHost &S);
// Can a recognised system be cut into `nranks` z-slabs?  0, or 2 (fewer than two planes per rank) / 7 (something
// couples across the z faces of a component: not the reference's system on a box) with the reason in `why`.
// seven bands at (-kdz, -sdx, -1, 0, 1, sdx, kdz), no tail, n a whole number of planes of kdz rows (kdz a whole
// number of sdx lines): a single-component 7-point operator on a grid, which can be cut along z plane by plane
bool ec3d_host_matrix_is_cube(const HostMatrix &M, int64_t &sdx, int64_t &kdz);
int ec3d_sav_cuttable(const SavHost &G, int nranks, std::string &why);
// planes [e0, e1) of a recognised system as a slab that owns [k0, k1) (same pitch, classes and table)
void ec3d_sav_slice(const SavHost &G, int64_t e0, int64_t e1, int64_t k0, int64_t k1, SavHost &L);

// ec3d_context.hip
int ec3d_upload_sav(ec3d_ctx *c, const SavHost &S);
// halo > 0: the matrix is a z-slab of a single-component operator whose planes hold `halo` rows (the ghost zones of
// the vectors then carry the neighbours' planes, ec3d_assemble_poisson_slab does the same natively)
int ec3d_upload_matrix(ec3d_ctx *c, const HostMatrix &M, int64_t halo = 0);
int ec3d_download_matrix(ec3d_ctx *c, HostMatrix &M);
void ec3d_free_matrix(ec3d_ctx *c);
int ec3d_prepare_vectors(ec3d_ctx *c);
// A matrix being built into the handle (behind ec3d_free_matrix): unless done(0) is reached -- on every early return --
// ec3d_free_matrix runs again and the handle is left without a matrix and with none of the failed one's memory.  What a
// placement search chose on this handle earlier is no part of the failed matrix and stays parked as after any
// ec3d_free_matrix: band streams taken back from placed_bands, the placed vectors and rings.  The assembly entry points
// call done(0) in front of ec3d_setup_rhs, so a failure there leaves the matrix in place, as it always did.
struct MatrixBuild {
    ec3d_ctx *c;
    bool kept = false;
    explicit MatrixBuild(ec3d_ctx *c_) : c(c_) {}
    MatrixBuild(const MatrixBuild &) = delete;
    MatrixBuild &operator=(const MatrixBuild &) = delete;
    ~MatrixBuild() { if (!kept) ec3d_free_matrix(c); }
    int done(int rc) { kept = rc == 0; return rc; }
};
// device memory for the plain band streams: the allocation a placement probe chose earlier, when the size fits
int ec3d_alloc_bands(ec3d_ctx *c, DevBuf<double> &bands, size_t bytes);
int ec3d_spare_pair(ec3d_ctx *c);
// host vector (reference numbering, n_ref entries) <-> device vector (device numbering)
int ec3d_vec_h2d(ec3d_ctx *c, double *dev, const double *host);
int ec3d_vec_d2h(ec3d_ctx *c, double *host, const double *dev);

// ec3d_context.hip
int ec3d_need_matrix(ec3d_ctx *c, const char *who); // 0, or 3 + error text when the handle has no matrix
// ec3d_solve.hip: where a consumer kernel finds its sums, and the launches of one iteration
// who produced the partial sums a consumer needs: an SpMV-type stage (slots BB, RR_INIT, D1, D2, D3), K2 (SS)
// or K4 (RR, RR0N)
enum { EC3D_BY_K4 = 0, EC3D_BY_SPMV = 1, EC3D_BY_K2 = 2 };
RedSrc ec3d_src_of(const ec3d_ctx *c, int producer);
RedSrc ec3d_part_of(const ec3d_ctx *c, int producer, bool split = false);
// k = 1..5, 0 = all five; part: 0 the whole launch, 1 / 2 the boundary / interior launch of stage 4 or 5 on a slab that runs
// the three-launch iteration (split_f.bnd / split_f.inte)
void ec3d_launch_stage(ec3d_ctx *c, const MatView &A, int it, int k, int part = 0);
inline bool ec3d_fused23(const ec3d_ctx *c) { return c->fuse23_ok && ((!c->dist && c->halo == 0) || c->slab_fused); }
inline bool ec3d_fused51(const ec3d_ctx *c)
{
    return c->fuse51_ok && ((!c->dist && c->halo == 0) || c->slab_fused) && c->pp_base != nullptr;
}
// K4 in SpMV form (k4s_x_r_spmv): only inside the three-launch iteration
inline bool ec3d_k4s(const ec3d_ctx *c) { return c->k4s_ok && ec3d_fused23(c) && ec3d_fused51(c); }
// deferred X update: single rank, own vectors (the rings exist), and the iteration either fully fused or not at all
inline int ec3d_xdefer(const ec3d_ctx *c)
{
    if (c->xdefer <= 1 || c->pp_base == nullptr) return 1;
    if (c->dist || c->halo != 0) { // a z-slab: only when the job's driver said so (the exchanged P / S then live in the rings)
        if (c->slab_xd <= 1) return 1;
        return (ec3d_fused23(c) == ec3d_fused51(c)) ? std::min(c->xdefer, c->slab_xd) : 1;
    }
    return (ec3d_fused23(c) == ec3d_fused51(c)) ? c->xdefer : 1;
}
// the pending X updates applied group by group on a stream of their own (only with the X update deferred)
inline bool ec3d_xasync(const ec3d_ctx *c)
{
    if (ec3d_xdefer(c) <= 1) return false;
    if (c->xinline && !c->dist && c->halo == 0) return true;
    if (!c->xasync_cap) return false;
    return (c->dist || c->halo != 0) ? c->slab_xasync : c->xasync_forced;
}
// the buffer of its ring (of AP's pair) that holds P / S / AP of iteration `it`; any `it`, negative ones too
inline int ec3d_ring_slot(int it, int depth) { return (it % depth + depth) % depth; }
inline int ec3d_p_slot(const ec3d_ctx *c, int it) { return ec3d_ring_slot(it + c->run.p_off, c->pdepth); }
inline int ec3d_s_slot(const ec3d_ctx *c, int it) { return ec3d_ring_slot(it, c->sdepth); }
inline int ec3d_ap_slot(int it) { return it & 1; }
// where vector `vec` (EC3D_VEC_P / _AP / _S; anything else: the plain work vector) of iteration `it` lives: the slot worked
// out from `me`'s cursor and plan, the pointer taken from `owner`'s tables (another slab of the job, ec3d_multi.hip)
double *ec3d_vec_at(const ec3d_ctx *me, const ec3d_ctx *owner, int vec, int it);
inline double *ec3d_vec_at(const ec3d_ctx *c, int vec, int it) { return ec3d_vec_at(c, c, vec, it); }
int ec3d_flush_x(ec3d_ctx *c, int stop_iter); // the pending X updates after an exit at stop_iter (enqueued)
bool ec3d_dist_can_split_planes(const ec3d_ctx *c);
void ec3d_launch_x_group_of(ec3d_ctx *c, int first, int count, bool join);
// a new run of iterations on this handle: the cursor as a fresh handle has it (every caller, every field)
void ec3d_run_reset(ec3d_ctx *c);
// this call launches iterations first .. last.  who: the iterate entry point that has to continue the handle's iterations
// (0, or 6 + error text when first is not the next one); nullptr: no such check
int ec3d_run_open(ec3d_ctx *c, int first, int64_t last, const char *who = nullptr);
void ec3d_after_s(ec3d_ctx *c, int it); // behind K2 / K2-in-K3 of iteration it
void ec3d_after_p(ec3d_ctx *c, int it); // behind K5 / K5-in-K1 of iteration it
void ec3d_launch_iteration(ec3d_ctx *c, const MatView &A, int it);
int ec3d_launch_begin(ec3d_ctx *c, const MatView &A, double tol, bool null_project = false);
int ec3d_single_rank_only(ec3d_ctx *c, const char *who);
// a handle of its own: not a slab, a rank or a handle of ec3d_multi (the caller words its own refusal)
inline bool ec3d_own_handle(const ec3d_ctx *c) { return !(c->in_multi || c->halo > 0 || c->nranks > 1 || c->dist); }
// K2 / K5 of a single-component z-slab as boundary-plane + interior launch (window sweeps, no tile lists); ec3d_dist.hip
int ec3d_dist_set_boundary_planes(ec3d_ctx *c, int32_t *enabled);
int ec3d_dist_launches(const ec3d_ctx *c, int stage, int it); // ec3d_dist.hip (call BEFORE the stage is launched)

// ec3d_kernels.hip — launchers (all asynchronous on `s`)
void ec3d_launch_spmv(const MatView &A, const Sweep &sw, const double *x, double *y, hipStream_t s);
void ec3d_launch_residual(const MatView &A, const Sweep &sw, const double *x, const double *b, double *r,
                          double *r0, double *p, double *part, hipStream_t s);
void ec3d_launch_finalize(const RedSrc &src, double *lsum, unsigned mask, hipStream_t s);
void ec3d_launch_finalize2(const RedSrc &a, unsigned mask_a, const RedSrc &b, unsigned mask_b, double *lsum, hipStream_t s);
void ec3d_launch_setup(SolverState *st, const RedSrc &src, double tol, hipStream_t s);
void ec3d_launch_k1(const MatView &A, const Sweep &sw, const SolverState *st, int it, const double *p,
                    const double *r0, double *ap, double *part, hipStream_t s);
void ec3d_launch_k2(const Sweep &sw, const RedSrc &src, SolverState *st, int it, const double *r, const double *ap,
                    double *sv, double *part, hipStream_t s);
void ec3d_launch_k3(const MatView &A, const Sweep &sw, SolverState *st, int it, const double *sv, double *as,
                    double *part, hipStream_t s);
void ec3d_launch_k23(const MatView &A, const Sweep &sw, const RedSrc &src, SolverState *st, int it, const double *r,
                     const double *ap, double *sv, double *as, double *part, hipStream_t s);
void ec3d_launch_k51(const MatView &A, const Sweep &sw, const RedSrc &src, SolverState *st, int it, const double *r,
                     const double *p_old, const double *ap_old, double *p_new, double *ap_new, double *r0, double *part,
                     double *hist, int64_t hist_cap, hipStream_t s);
void ec3d_launch_k4d(const Sweep &sw, const RedSrc &src_ss, const RedSrc &src, SolverState *st, int it, int ne, int xm,
                     const double *const *p, const double *const *sv, const double *as, const double *r0, double *x,
                     double *r, double *part, double *hist, int64_t hist_cap, hipStream_t s);
void ec3d_launch_k4s(const MatView &A, const Sweep &sw, const RedSrc &src_ss, const RedSrc &src, SolverState *st, int it,
                     int ne, int xm, const double *const *p, const double *const *sv, const double *r0, double *x, double *r,
                     double *part, double *hist, int64_t hist_cap, hipStream_t s);
void ec3d_launch_x_flush(const Sweep &sw, const SolverState *st, const double *const *p, const double *const *sv,
                         double *x, hipStream_t s);
void ec3d_launch_x_group(const Sweep &sw, const SolverState *st, const double *const *p, const double *const *sv, int first,
                         int count, int d2, double *x, int nblk, hipStream_t s);
void ec3d_launch_k4(const Sweep &sw, const RedSrc &src_ss, const RedSrc &src, SolverState *st, int it,
                    const double *p, const double *sv, const double *as, const double *r0, double *x, double *r,
                    double *part, double *hist, int64_t hist_cap, hipStream_t s);
void ec3d_launch_k5(const Sweep &sw, const RedSrc &src, SolverState *st, int it, const double *r, const double *ap,
                    const double *p_old, double *p, double *r0, double *hist, int64_t hist_cap, hipStream_t s);

// ec3d_assemble.hip
// planes [e0, e1) of the global grid are held (e0 = 0, e1 = sdz: everything); rows of planes outside
// [k0, k1) are inert (zero coefficients): they only carry the neighbours' values
int ec3d_assemble_device(ec3d_ctx *c, int32_t sdx, int32_t sdy, int32_t sdz, int32_t e0, int32_t e1, int32_t k0,
                         int32_t k1, const int8_t *geoPHYS, const int32_t *geoPHYS_C, const double *valPHYS,
                         int32_t nsub_glob, const double *BND, const double *delta, double dt);
// same plane arguments as ec3d_assemble_device; returns -1 when the structured form does not apply
int ec3d_assemble_sav_device(ec3d_ctx *c, int32_t sdx, int32_t sdy, int32_t sdz, int32_t e0, int32_t e1, int32_t k0,
                             int32_t k1, const int8_t *geoPHYS, const int32_t *geoPHYS_C, const double *valPHYS,
                             int32_t nsub_glob, const double *BND, const double *delta, double dt);
int ec3d_assemble_poisson_device(ec3d_ctx *c, int32_t sdx, int32_t sdy, int32_t sdz, int32_t k0, int32_t k1,
                                 const double *BND, const double *delta);
// the same assembly (dictionary form) into a matrix of its own: a coarse level of the multigrid hierarchy
// (re)make A.cls_same from A.cls where the grid divides into 2-D tiles; leaves it empty elsewhere (ec3d_assemble.hip)
int ec3d_build_class_runs(ec3d_ctx *c, DevMatrix &A);
int ec3d_assemble_poisson_level(ec3d_ctx *c, DevMatrix &A, int32_t sdx, int32_t sdy, int32_t sdz, const double *BND,
                                const double *delta);
// ec3d_mg.hip
void ec3d_mg_free(ec3d_ctx *c);
int ec3d_mg_chunk(const ec3d_ctx *c);             // iterations per poll of the preconditioned loop
void ec3d_mg_launch_iteration(ec3d_ctx *c, int it); // one preconditioned iteration (after ec3d_launch_begin)
// ec3d_format.cpp / ec3d_context.hip: dictionary compression of the bands
int ec3d_build_dictionary_host(HostMatrix &M);
// ec3d_guess.hip: the history of earlier solutions around a solve (solve_core, when guess.depth > 0)
void ec3d_guess_free(ec3d_ctx *c);  // the pairs and their memory go (a new matrix, a new depth); the depth stays
int ec3d_guess_clear(ec3d_ctx *c);  // no pair stored, the vectors zero again
int ec3d_guess_project(ec3d_ctx *c, const MatView &A);            // in front of ec3d_launch_begin
int ec3d_guess_note_setup(ec3d_ctx *c);                           // behind it
int ec3d_guess_update(ec3d_ctx *c, const MatView &A, bool store); // behind the solve and ec3d_flush_x; one read-back
// ec3d_mg.hip: N ~ (A^T)^-1 of ec3d_set_null_precond -- a block hierarchy of its own (kind: EC3D_NULL_PRECOND_BLOCK_MG
// or _A; 0 sweeps: the defaults), which the caller deletes; levels and 3 dims per level of the hierarchy.  The adjoint
// solves that use it: ec3d_outer.hpp
int ec3d_null_mg_build(ec3d_ctx *c, int kind, int pre, int post, int coarse, ec3d_mg **out);
void ec3d_null_mg_delete(ec3d_mg *m);
void ec3d_null_mg_dims(const ec3d_mg *m, int32_t *levels, int32_t *dims);
// ec3d_transpose.hip: y = A^T x on rows [0, A.n) of the structured form (x, y: device vectors, no ghosts needed)
void ec3d_launch_spmv_t(const MatView &A, int64_t n, const double *x, double *y, hipStream_t s);
// ec3d_null.hip: the left null vectors around a solve (solve_core, when nullp.on)
void ec3d_null_free(ec3d_ctx *c);                 // Q and its memory go (a new matrix); the setting stays
int ec3d_null_eligible(const ec3d_ctx *c, const char *who, bool set_text); // 0, EC3D_NULL_E_MATRIX or 4
// per connected component of the conducting cells (6-neighbourhood, scan order of the first cell): the U row of its
// middle cell, in device numbering and 0-based in the reference's -- the seeds of the real and the harmonic set-up
struct NullSeed {
    int64_t row, seed_ref;
};
int ec3d_null_seeds(ec3d_ctx *c, std::vector<NullSeed> &seeds);
int ec3d_null_prepare(ec3d_ctx *c);               // in front of the solve: builds Q when there is none
int ec3d_null_project(ec3d_ctx *c);               // behind the residual launch of ec3d_launch_begin, before its set-up
int ec3d_null_note(ec3d_ctx *c, double bnorm);    // behind the solve: `removed` of ec3d_get_null_projection
// ec3d_harmonic.hip
void ec3d_harmonic_free(ec3d_ctx *c); // the tables, the single system and the batch go (a new matrix); the settings stay
// ec3d_output.hip
void ec3d_free_output(ec3d_ctx *c);
// ec3d_rhs.hip
void ec3d_free_rhs(ec3d_ctx *c);
int ec3d_setup_rhs(ec3d_ctx *c, int64_t nCells, const int8_t *geoPHYS, const int32_t *geoPHYS_C,
                   const double *valPHYS, int32_t nsub_glob, double dt);
// ec3d_integrals.hip
void ec3d_free_integrals(ec3d_ctx *c);
int ec3d_setup_integrals(ec3d_ctx *c, int64_t nCells, const int8_t *geoPHYS, const int32_t *geoPHYS_C,
                         const double *valPHYS, int32_t nsub_glob);
// what the calls on the resident fields of an undivided A-V handle refuse first, in this order: 3 (no A-V system from
// ec3d_assemble), 5 (a z-slab or a slab of ec3d_multi), with the error text; 0 otherwise
int ec3d_need_undivided(ec3d_ctx *c, const char *who);
// ec3d_probes.hip
void ec3d_free_probes(ec3d_ctx *c);
