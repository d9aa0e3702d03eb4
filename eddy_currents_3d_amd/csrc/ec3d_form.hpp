// ec3d_form.hpp — which instance of an SpMV-type kernel a launch runs (host only: no kernels in here).
//
// Every SpMV-type kernel of ec3d_kernels.hip is a template on <FMT, NT, ZM, TAIL, PATCH[, HS]>.  ec3d_spmv_form derives
// those from the matrix and the sweep choose_sweep planned, ec3d_form_lds the dynamic LDS that instance needs; the
// dispatcher in ec3d_kernels.hip turns the result into template arguments.  DESIGN.md section 12 has the table of
// instances per kernel family.
#pragma once
#include "ec3d_internal.hpp"
#include "ec3d_sweep_lists.hpp"

// Matrix formats the row kernel is specialised for (template parameter FMT):
//   FMT_GENERIC  any number of bands, one fp64 stream per band
//   FMT_DIA7     7 bands, unrolled (72 B/row: 56 coefficients + x + y)
//   FMT_DICT7    7 bands whose coefficient 7-tuples take <= 256 distinct values ("stencil classes"):
//                one class byte per row + a table staged in LDS (17 B/row: 1 + x + y).  The values
//                multiplied are the same doubles, so results are bit-identical to FMT_DIA7.
//   FMT_SAV      the structured A-V form (MatView::sav): class byte per row, U on the grid, no tail
enum { FMT_GENERIC = 0, FMT_DIA7 = 7, FMT_DICT7 = 107, FMT_SAV = 207 };
#define EC3D_SAV_STRIDE 16 /* doubles per class of the structured form's table */
#define EC3D_NSTAGE 4 /* 16-byte slots per thread: 4 x 4 KiB per workgroup */
#define EC3D_NSTAGE_RT 2 /* the same on runtime-shaped 2-D tiles (sav_patch_step) */

struct SpmvForm {
    int fmt;    // FMT_*
    bool nt;    // nontemporal accesses to once-touched streams
    bool zm;    // z-marching map
    bool tail;  // band + sliced-ELL tail
    bool patch; // 2-D tiles (dictionary cube: EC3D_PX x EC3D_PY; structured form: runtime shaped)
    bool il;    // interleaved z-march of the structured form
    bool hs;    // z-slab of the three-launch iteration: the formed vector is also stored on the halo planes
                // (only k23_s_spmv_dots and k51_p_spmv_dot have such instances)
    bool pair;  // paired patch columns (Sweep::pair holds the launch's kind): set by the launcher, see ec3d_form_pair
    bool apc;   // k51_p_spmv_dot: AP_old of the patch's own cells formed from P_old, not loaded (Sweep::k51_ap): set by the
                // launcher, see ec3d_form_apc
};

inline SpmvForm ec3d_spmv_form(const MatView &A, const Sweep &sw)
{
    SpmvForm f{};
    f.fmt = A.sav ? FMT_SAV : A.nb == 7 && A.ncls > 0 ? FMT_DICT7 : A.nb == 7 ? FMT_DIA7 : FMT_GENERIC;
    // streaming policy: vectors of >= 32 MiB each (n_pad >= 4 Mi rows) cannot live in the caches (bits above 0: keep hints)
    f.nt = (sw.nt & 1) != 0;
    f.zm = sw.zm_tpp > 0 && sw.bnd_last < 0 && f.fmt != FMT_GENERIC;
    f.tail = f.fmt != FMT_SAV && A.has_tail;
    f.patch = f.zm && !f.tail && ((f.fmt == FMT_DICT7 && sw.patch_npx > 0) || (f.fmt == FMT_SAV && sw.rp_px > 0)); // choose_sweep
    f.il = f.zm && !f.patch && f.fmt == FMT_SAV && sw.il_planes > 0;
    f.hs = f.fmt == FMT_DICT7 && sw.halo_store != 0;
    return f;
}

// Does a launch of kind `kind` (one EC3D_PAIR_* bit) of this form run paired patch columns?  Dictionary cube on 2-D tiles,
// no z-slab instance, and the sweep's plan (choose_sweep, ec3d_patch_pairs_ok) says so for the kind.
inline bool ec3d_form_pair(const SpmvForm &f, const Sweep &sw, int kind)
{
    return f.patch && f.fmt == FMT_DICT7 && !f.hs && (sw.pair & kind) != 0;
}

// Does K5-in-K1 of this form compute AP_old inside the patch (patch_pair_apc in ec3d_kernels.hip)?  The same instances as
// pairing: dictionary cube on 2-D tiles, no z-slab instance; and choose_sweep's policy for the handle (Sweep::k51_ap).
inline bool ec3d_form_apc(const SpmvForm &f, const Sweep &sw)
{
    return f.patch && f.fmt == FMT_DICT7 && !f.hs && sw.k51_ap != 0;
}

// The form a launch of a kernel family runs: ec3d_spmv_form narrowed by what the family has instances for (fam_hs: z-slab
// instances; pair_kind: the EC3D_PAIR_* bit of its launches, 0 = never paired; fam_apc: instances that form AP_old on the
// patch).  launch_form (ec3d_kernels.hip) dispatches on exactly this, and what a handle reports of its launches
// (ec3d_get_k51_ap_form) is read off the same function.
inline SpmvForm ec3d_family_form(const MatView &A, const Sweep &sw, bool fam_hs, int pair_kind, bool fam_apc)
{
    SpmvForm f = ec3d_spmv_form(A, sw);
    f.hs = f.hs && fam_hs;
    f.pair = ec3d_form_pair(f, sw, pair_kind);
    f.apc = fam_apc && ec3d_form_apc(f, sw);
    return f;
}
// k51_p_spmv_dot's launch (Fused51Family: z-slab instances, pairs as EC3D_PAIR_K51, has the APC instances)
inline SpmvForm ec3d_k51_form(const MatView &A, const Sweep &sw) { return ec3d_family_form(A, sw, true, EC3D_PAIR_K51, true); }

// Dynamic LDS bytes of the launch; EC3D_TBL_DECL (ec3d_kernels.hip) lays the same LDS out on the device.
// The class table (55 + 9 D classes of the structured form with D conducting domains: 64 classes =
// 8 KiB for one domain, 253 = 31.6 KiB at D = 22, which with the staging slots caps the CU at 3 workgroups -- a cost
// not measured) and, for the z-marching structured kernels, the
// staging slots behind it (16 KiB): 24.6 KiB per workgroup, six of them fit a CU's 160 KiB
inline size_t ec3d_form_lds(const MatView &A, const SpmvForm &f)
{
    const size_t sav_tbl = (size_t)A.ncls * EC3D_SAV_STRIDE * 8;
    // structured form, interleaved z-march: the table alone (walk_zm_il stages nothing)
    if (f.il) return sav_tbl;
    // structured form on runtime-shaped 2-D tiles: table, two exchange buffers, two staging slots (sav_patch_step)
    if (f.patch && f.fmt == FMT_SAV) return sav_tbl + (size_t)(2 + EC3D_NSTAGE_RT) * EC3D_TILE * 8;
    // 2-D tiles of the single-component kernels: table (an even number of doubles), two centre-plane buffers (patch_pair)
    // (paired patch columns: the two buffers hold eight patch rows)
    // (AP_old formed on the patch, patch_pair_apc: two more buffers, of raw P_old, and all four with the two rim rows beside the
    // patch rows)
    if (f.patch)
        return (size_t)((f.fmt == FMT_DICT7 ? A.ncls * 7 + 1 : 0) & ~1) * 8 +
               (f.apc ? (size_t)4 * ((f.pair ? 2 : 1) * EC3D_PY + 2) * EC3D_PX * 8 : (size_t)(f.pair ? 4 : 2) * EC3D_TILE * 8);
    if (f.fmt == FMT_DICT7) return (size_t)A.ncls * 7 * 8;
    if (f.fmt == FMT_SAV) return sav_tbl + (f.zm ? (size_t)EC3D_NSTAGE * EC3D_TILE * 8 : 0);
    return 0;
}
