/*
 * ec3d_hip.h — C ABI of libec3d_hip.so, the MI355X (gfx950) solver for the A–V eddy-current
 * system of JNSresearcher/eddy_currents_3d.
 *
 * Scope: the BiCGSTAB-with-restart solve the reference time loop runs every step
 * (src/EC3D.f90:408 -> src/solvers.f90:3-63) and the one-time assembly of its matrix
 * (src/EC3D.f90:465-1049).  Everything is fp64; no CPU fallback exists: every entry point
 * fails (status != 0 / abort in the F77 symbol) when no HIP device is usable.
 *
 * Plain C types only; all arrays are caller-owned host memory unless a name says "device".
 * Fortran-side binding: see INTEGRATION.md (one `interface ... bind(C)` block) — arrays are
 * column-major with i fastest, which is the same linear order as nn = i + (j-1)*sdx + (k-1)*sdx*sdy
 * (src/EC3D.f90:506-510).
 */
#ifndef EC3D_HIP_H
#define EC3D_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * 1. Drop-in for the reference solver symbol
 *    replaces: SUBROUTINE sprsBCGstabWR (valA, irow, jcol, n, b, x, tolerance, itmax, iter)
 *              src/solvers.f90:3 (external procedure, F77 ABI: lower case + '_', all by reference)
 *    called from src/EC3D.f90:408.  Same observable behaviour: x in/out (warm start), iter out,
 *    ‖b‖ = 0 -> iter = 0 and x untouched (:23), itmax exit after itmax+1 iterations with ‖R‖
 *    printed (:25-28), restart rule (:47-49).  irow/jcol are 1-based (:58-59).
 *    The device copy of the matrix is cached across calls (the reference assembles once,
 *    src/EC3D.f90:115); ec3d_invalidate() drops the cache for callers that rebuild in place.
 *    HIP failures abort with a message (the reference interface has no status channel).
 * ---------------------------------------------------------------------------------------- */
void sprsbcgstabwr_(double *valA, int32_t *irow, int32_t *jcol, int32_t *n, double *b, double *x,
                    double *tolerance, int32_t *itmax, int32_t *iter);
void ec3d_invalidate(void);

/* ------------------------------------------------------------------------------------------
 * 2. Native handle API (what a Fortran host binds through iso_c_binding)
 *    Every function returns 0 on success, non-zero on failure; ec3d_last_error() has the text.
 * ---------------------------------------------------------------------------------------- */
typedef struct ec3d_ctx *ec3d_handle;

int ec3d_create(ec3d_handle *h, int device);
int ec3d_destroy(ec3d_handle h);
const char *ec3d_last_error(void);

/* Matrix from the reference's CSR triple (src/EC3D.f90:36-38 irow/jcol/valA, 1-based).
 * Converted once on the host to a device format: the structured A-V form (1 class byte per row, U
 * embedded in the grid) when the matrix is recognised, entry by entry, as the one gen_sparse_matrix
 * builds (see ec3d_probe_csr); otherwise 7 bands (class-coded or plain) + a sliced-ELL tail that keeps
 * every row's stored order.  Results do not depend on the format.
 * Bands: the offsets that >= 40 % of a row sample carry, at most 16 (the most frequent; equal counts in favour of
 * the smaller offset).  Seven bands at (-kdz, -sdx, -1, 0, 1, sdx, kdz) with kdz a whole number of 512-row tiles get
 * the z-marching and 2-D-tile kernels on the evidence of the offsets alone: the values are not looked at and need
 * not be a grid operator's.  A nonzero coefficient in a wrap slot (+-1 at the end of an x-row, +-sdx at the end of a
 * plane) multiplies the LINEAR neighbour x[r +- 1], x[r +- sdx] in every kernel form, as the CSR row says
 * (tests/test_gpu_generated_csr.py). */
int ec3d_set_matrix_csr(ec3d_handle h, int32_t n, const double *valA, const int32_t *irow,
                        const int32_t *jcol);

/* Assembly on the device, replaces gen_sparse_matrix (src/EC3D.f90:465-1049).
 *   geoPHYS   int8  [sdx*sdy*sdz]   src/m_vxc2data.f90:43   domain id per cell
 *   geoPHYS_C int32 [sdx*sdy*sdz]   src/m_vxc2data.f90:44   0 or U column id 3*nCells+m
 *   valPHYS   f64   (nsub_glob,5)   src/m_vxc2data.f90:52   column-major
 *   BND       f64   (3,2)           src/EC3D.f90:77         column-major
 *   delta     f64   [3], dt                                  src/EC3D.f90:60-61
 * Unknown layout [Ax | Ay | Az | U], n = 3*nCells + Ncells0 (src/EC3D.f90:101-106): that is the
 * numbering of every host vector; on the device U is embedded in the grid and xy planes may be
 * padded (ec3d_get_row_map), which only callers of ec3d_device_vector ever see.
 * Returns 3 where the reference would index out of range (conductor on the box boundary or
 * thinner than 3 cells), 1/2 for its two STOPs (:717-720, :924-936). */
int ec3d_assemble(ec3d_handle h, int32_t sdx, int32_t sdy, int32_t sdz, const int8_t *geoPHYS,
                  const int32_t *geoPHYS_C, const double *valPHYS, int32_t nsub_glob,
                  const double *BND, const double *delta, double dt);

/* The non-conducting Ax block alone (src/EC3D.f90:528-654): the synthetic-cube operator of
 * BASELINE.json configs 2 and 4; n = sdx*sdy*sdz. */
int ec3d_assemble_poisson(ec3d_handle h, int32_t sdx, int32_t sdy, int32_t sdz, const double *BND,
                          const double *delta);

/* One solve, host vectors (H2D of b and x, D2H of x).  resid_hist (may be NULL) receives
 * 2 doubles per iteration: ‖S‖₂ (src/solvers.f90:34) and ‖R‖₂ (:43), hist_cap = iterations. */
int ec3d_solve(ec3d_handle h, const double *b, double *x, double tolerance, int32_t itmax,
               int32_t *iter, double *resid_hist, int32_t hist_cap);

/* Same with b and x already resident in HBM: the library-owned device vectors are filled
 * with ec3d_upload / read with ec3d_download (or written by the caller's own kernels through
 * ec3d_device_vector).  No host<->device vector traffic inside the call. */
enum { EC3D_VEC_X = 0, EC3D_VEC_B = 1, EC3D_VEC_R = 2, EC3D_VEC_R0 = 3, EC3D_VEC_P = 4,
       EC3D_VEC_AP = 5, EC3D_VEC_S = 6, EC3D_VEC_AS = 7, EC3D_NVEC = 8 };
int ec3d_upload(ec3d_handle h, int which, const double *host);
int ec3d_download(ec3d_handle h, int which, double *host);
int ec3d_device_vector(ec3d_handle h, int which, double **device_ptr, int64_t *n);
int ec3d_solve_resident(ec3d_handle h, double tolerance, int32_t itmax, int32_t *iter,
                        double *resid_hist, int32_t hist_cap);

/* Per-time-step field work around the solve, on the resident vectors (B = Jaf, X = Uaf), so only the
 * coil cells' source values cross PCIe each step.  Needs a matrix from ec3d_assemble, or from
 * ec3d_assemble_slab: ids are then local to the held planes (d*nC_held + cell + 1) and the caller
 * refreshes the X halo planes first (eddy_currents_3d_amd/dist.py, SlabSolver.rhs_step).
 * ec3d_rhs_step  replaces src/EC3D.f90:275-404: with moving != 0 first keeps only the inertial part
 *   of Jaf (:277-296); then Jaf(src_index(q)) = src_value(q), q in order (1-based unknown ids; the
 *   host evaluates the source functions and the coil motion, :245-340); then Jaf = a*Uaf + Jaf on the
 *   conductor cells, the U-row right-hand sides (:385-392) and the zero-fills at cel_bnd* (:396-402).
 * ec3d_post_update  replaces :412-433 after the solve.
 * Any number of conducting domains on a handle of ec3d_assemble (each cell uses its own domain's 2C/dt); several of
 * them on a slab (ec3d_assemble_slab, ec3d_multi_*) return 5. */
int ec3d_rhs_step(ec3d_handle h, int32_t moving, int32_t nsrc, const int32_t *src_index,
                  const double *src_value);
int ec3d_post_update(ec3d_handle h);

/* Which U rows ec3d_rhs_step gives their right-hand side s = (the row's A part) . Uaf.  The reference loops over the
 * conducting domains m and sets Jaf(3*nCells + n) = s for n = 1..siznod(m) (src/EC3D.f90:374-392), so with several
 * domains only the U rows n <= max_m siznod(m) get theirs and every later U row keeps 0: EC3D_U_RHS_REFERENCE, the
 * default.  EC3D_U_RHS_ALL gives every U row its s, the physically consistent right-hand side and a DEPARTURE from
 * the reference.  With one conducting domain the two are the same.  The rule belongs to the handle and outlives new
 * matrices.  An unknown rule returns 2 and leaves the handle unchanged. */
enum { EC3D_U_RHS_REFERENCE = 0, EC3D_U_RHS_ALL = 1 };
int ec3d_set_u_rhs(ec3d_handle h, int32_t rule);

/* The four float32 point vectors of the reference's field_N.vtk (writeVtk_field, src/utilites.f90:222-289)
 * from the resident Uaf (X) and Jaf (B): Field_A, Vector_field_eddy (NULL allowed when there is no
 * conductor), Vector_field_SOURCE, Vector_field_B = curl A (central differences clamped at the box
 * faces, :276-289).  Each output: 3*nCells floats, xyz interleaved, cell order nn.  Host byte order.
 * On a handle from ec3d_assemble_slab: the owned planes only (3*sdx*sdy*(k1-k0) floats per output, in
 * order), the curl reading the halo planes at the slab's edges -- refresh the X halo first; a slab without
 * conducting cells leaves field_eddy untouched (pass zeros). */
int ec3d_vtk_fields(ec3d_handle h, const double *delta, float *field_A, float *field_eddy,
                    float *field_source, float *field_B);

/* The same, overlapped with the next time step (the reference's loop writes field_N.vtk every output step and does
 * nothing else meanwhile, src/EC3D.f90:436-444).  _begin enqueues the field kernel on the handle's stream -- it sees
 * the X and B of this step -- and the copy of the four vectors into one of three pinned host buffers (taken in turn) on a side stream,
 * and returns without waiting: the caller goes on with ec3d_rhs_step / ec3d_solve_resident of the next step.
 * big_endian != 0: the floats arrive in the byte order of the reference's BINARY legacy-VTK file (swapped on the
 * device), ready to be written as they are.  _wait blocks until that slot's copy has landed and returns pointers into
 * the pinned buffer (field_eddy = NULL without conductors), valid until the third ec3d_vtk_fields_begin after this
 * one (EC3D_VTK_SLOTS buffers); *ncells = cells per vector (3 floats each). */
#define EC3D_VTK_SLOTS 3
int ec3d_vtk_fields_begin(ec3d_handle h, const double *delta, int32_t big_endian, int32_t *slot);
int ec3d_vtk_fields_wait(ec3d_handle h, int32_t slot, const float **field_A, const float **field_eddy,
                         const float **field_source, const float **field_B, int64_t *ncells);

/* Joule loss and Lorentz force per conducting domain, from the resident Uaf (X) and Jaf (B), summed on the device.
 * They are the integrals of the very fields field_N.vtk shows, before their rounding to float32 -- not a
 * Maxwell-stress evaluation.  Per conductor cell (geoPHYS_C != 0), in double precision and without contraction:
 *   J = s * Jaf, s = -0.07957747154594766788444e7 (Vector_field_eddy, A/m^2: valPHYS(:,2) is mu0 * sigma)
 *   B = curl A, central differences clamped at the box faces (Vector_field_B)
 *   q = Jx*Jx + Jy*Jy + Jz*Jz,   f = J x B
 * and per domain d (the cells' geoPHYS id), with C_d = valPHYS(d, 2):
 *   cells    conductor cells of the domain
 *   sigma    C_d * 0.07957747154594766788444e7                S/m
 *   joule_w  (dx*dy*dz) * sum(q) / sigma                      W
 *   force_n  (dx*dy*dz) * sum(fx, fy, fz)                     N
 * Domains come in ascending id order.  *ndomains receives their number; out == NULL: the count only; no conductor:
 * 0 domains, status 0.  The sums have a fixed order (no atomics): the same X, B and geometry give the same bits,
 * whichever device form holds them.  X and B are read as they stand -- they mean the above after ec3d_post_update of
 * a step; nothing is checked about that -- and no work vector is written.  One 32-byte-per-domain copy and one
 * synchronisation of the handle's stream per call.
 * Status 3: no A-V system from ec3d_assemble (a Poisson or CSR matrix); 5: a z-slab (ec3d_assemble_slab) or a slab
 * of ec3d_multi; 2: delta or ndomains NULL, or out != NULL with cap < *ndomains (the count is still written). */
typedef struct {
    int32_t domain;
    int32_t pad;
    int64_t cells;
    double sigma;
    double joule_w;
    double force_n[3];
} ec3d_domain_integral;
int ec3d_domain_integrals(ec3d_handle h, const double *delta, int32_t cap, int32_t *ndomains,
                          ec3d_domain_integral *out);

/* Magnetic energy of the box and the integral of A.J, from the resident Uaf (X) and Jaf (B), in one streaming pass over
 * every cell on the device.  Per cell, in double precision and without contraction, the B and s of
 * ec3d_domain_integrals:
 *   B = curl A (Vector_field_B),   J = s * Jaf in EVERY cell,   a = (Ax*Jx + Ay*Jy) + Az*Jz
 * and over the box, with 1/mu0 = 0.07957747154594766788444e7 (the literal behind s):
 *   cells        cells of the box
 *   energy_axis  (dx*dy*dz) * (0.5 / mu0) * sum(Bx*Bx), sum(By*By), sum(Bz*Bz)      J
 *   energy_b     (dx*dy*dz) * (0.5 / mu0) * ((sum Bx*Bx + sum By*By) + sum Bz*Bz)   J   (L = 2 W / I^2)
 *   aj_source    (dx*dy*dz) * sum(a) over the cells outside the conductors          J
 *   aj_eddy      (dx*dy*dz) * sum(a) over the conductor cells (geoPHYS_C != 0)       J
 * The sums have a fixed order (no atomics): the same X, B and geometry give the same bits, whichever
 * device form and plane pitch hold them.  X and B are read as they stand -- they mean the above after
 * ec3d_post_update of a step -- and no work vector is written.  The first call allocates one byte per cell (none
 * without conductors) and 40 KB; every call is two launches, one 40-byte copy and one synchronisation of the handle's
 * stream.  Status 3, 5 as ec3d_domain_integrals; 2: delta or out NULL. */
typedef struct {
    int64_t cells;
    double energy_b;
    double energy_axis[3];
    double aj_source;
    double aj_eddy;
} ec3d_field_energy_info;
int ec3d_field_energy(ec3d_handle h, const double *delta, ec3d_field_energy_info *out);

/* Flux linkage of every domain that holds cells outside the conductors, from the resident Uaf (X) and Jaf (B), summed on
 * the device.  Per such cell (geoPHYS_C == 0), J and a as in ec3d_field_energy; per domain d (the cells' geoPHYS id):
 *   cells    cells of the domain
 *   linkage  (dx*dy*dz) * sum(a)              J    (the reference stores +mu0 * J in source cells, so s * Jaf is minus the
 *                                                   source current density: psi * I of a coil is -linkage)
 *   jsum     (dx*dy*dz) * sum(Jx, Jy, Jz)     A m  (divides the current out of a straight conductor segment)
 * The library is given ids, not roles: it cannot tell the environment (air) from a coil that carries no current at the
 * moment, so EVERY non-conducting domain is listed, the air among them with its own cell list -- where Jaf is 0 the
 * sums are exactly 0.  Conducting domains are not listed (ec3d_domain_integrals covers them).  Domains come in
 * ascending id order; *ndomains receives their number; out == NULL: the count only.  The cell lists are built on the
 * host by ec3d_assemble (4 B per non-conducting cell) and moved to the device by the first call with out != NULL; a
 * handle that never calls holds nothing on the device.  Fixed summation order as in ec3d_domain_integrals; X and B are
 * read as they stand and no work vector is written; one 32-byte-per-domain copy and one synchronisation per call.
 * Status 3, 5 as ec3d_domain_integrals; 2: delta or ndomains NULL, or out != NULL with cap < *ndomains (the count is
 * still written). */
typedef struct {
    int32_t domain;
    int32_t pad;
    int64_t cells;
    double linkage;
    double jsum[3];
} ec3d_domain_link;
int ec3d_domain_linkage(ec3d_handle h, const double *delta, int32_t cap, int32_t *ndomains, ec3d_domain_link *out);

/* The resident fields at chosen cells (probes): points, lines, planes or any sub-box, sampled from the resident Uaf (X)
 * and Jaf (B) by one small launch, returned at once (ec3d_probe_sample) or appended to a record that stays on the device
 * and is read once at the end of a run (ec3d_probe_record, ec3d_probe_read).  The EC3D_PROBE_NCOMP = 13 values of the
 * probe at cell (i, j, k), in double precision and without contraction, the s and the B of ec3d_domain_integrals:
 *    0 ..  2  a       A                                               (Field_A)
 *    3 ..  5  eddy    s * Jaf in a conductor cell (geoPHYS_C != 0), else 0.0   (Vector_field_eddy)
 *    6 ..  8  source  Jaf outside the conductors, else 0.0           (Vector_field_SOURCE)
 *    9 .. 11  b       curl A, central differences clamped at the box faces     (Vector_field_B)
 *   12        u       the cell's U, 0.0 outside the conductors
 * (float) of the first twelve is bit for bit what ec3d_vtk_fields returns at that cell.  X and B are read as they stand
 * -- they mean the above after ec3d_post_update of a step -- and no work vector is written.  Nothing is summed: the
 * same X, B and geometry give the same bits, whichever device form and plane pitch hold them.
 *
 * ec3d_set_probes    cells: nprobes 0-based cell numbers i + j*sdx + k*sdx*sdy, in the caller's order, duplicates
 *                    allowed.  capacity: records the device buffer holds (13 * nprobes doubles each); 0: no buffer,
 *                    ec3d_probe_sample only.  nprobes = 0 clears the set and frees everything.  The set replaces the
 *                    previous one and its records; it belongs to the assembled matrix: a new assembly or matrix clears
 *                    it.  Device memory: 8 B per probe and 104 B per probe and record (one more for the sample).
 * ec3d_probe_sample  one launch, one copy, one synchronisation of the handle's stream: out receives 13 * nprobes
 *                    doubles by component, then by probe: out[c * nprobes + p].
 * ec3d_probe_record  enqueues the same launch on the handle's stream into record number `recorded`, keeps T beside
 *                    it on the host and returns without waiting.  A full buffer (recorded == capacity; always with
 *                    capacity 0): nothing is written, status EC3D_PROBE_E_FULL.
 * ec3d_probe_read    records [first, first + count) with one copy and one synchronisation:
 *                    out[(s * 13 + c) * nprobes + p] and T_out[s], s counted from `first`.
 * ec3d_probe_reset   recorded = 0; the set and the buffer stay.
 * ec3d_get_probes    nprobes, capacity, recorded and the device bytes held (all 0 without a set); any handle.
 * Status 3, 5 as ec3d_domain_integrals; 2: a NULL argument, a negative count, no probes set, first + count > recorded,
 * or a cell outside the box -- ec3d_last_error() then names the first offending entry and the previous set stays. */
#define EC3D_PROBE_NCOMP 13
#define EC3D_PROBE_E_FULL 24
typedef struct {
    int64_t nprobes;
    int64_t capacity;
    int64_t recorded;
    int64_t device_bytes;
} ec3d_probe_info;
int ec3d_set_probes(ec3d_handle h, int64_t nprobes, const int64_t *cells, int64_t capacity);
int ec3d_probe_sample(ec3d_handle h, const double *delta, double *out);
int ec3d_probe_record(ec3d_handle h, const double *delta, double T);
int ec3d_probe_read(ec3d_handle h, int64_t first, int64_t count, double *T_out, double *out);
int ec3d_probe_reset(ec3d_handle h);
int ec3d_get_probes(ec3d_handle h, ec3d_probe_info *info);

/* ||B - A*X|| / ||B|| of the RESIDENT vectors, computed on the device by the solve's own setup kernel
 * (src/solvers.f90:14-21); bnorm (may be NULL) receives ||B||.  The check of a returned x that does not rely
 * on the iteration's recurrence for R.  Overwrites the work vectors R, R0, P (rebuilt by the next solve). */
int ec3d_true_residual(ec3d_handle h, double *rel, double *bnorm);

/* y = A*x through the device format (src/solvers.f90:54-61), host vectors.  Parity probe. */
int ec3d_spmv(ec3d_handle h, const double *x, double *y);
/* y = A^T*x on the structured A-V form of ec3d_assemble (undivided handle), host vectors.  Row j adds
 * table[class(i)][slot] * x[i] over the rows i that hold an entry in column j, in ascending i (the reference's
 * numbering), from +0.0, every product and sum rounded on its own, zero coefficients left out.  Any other matrix
 * form, a z-slab or a slab of ec3d_multi: EC3D_NULL_E_MATRIX / 4, nothing computed.  Uses P and AP as scratch. */
int ec3d_spmv_t(ec3d_handle h, const double *x, double *y);

/* Read the device matrix back as the reference's 1-based CSR (two-pass: jcol == NULL -> sizes).  A matrix from
 * ec3d_assemble comes back with the zeros the reference stores (boundary value 0); one from ec3d_set_matrix_csr
 * without the zeros it stored. */
int ec3d_export_csr(ec3d_handle h, int32_t *n, int64_t *nnz, int32_t *irow, int32_t *jcol,
                    double *valA);

/* Index lists the reference builds during assembly (src/EC3D.f90:758-760, :938-940), 1-based:
 * which = 0..5 -> cel_bndX, Y, Z, Ux, Uy, Uz.  list == NULL -> count only. */
int ec3d_get_cel_bnd(ec3d_handle h, int which, int32_t *count, int32_t *list);

/* Band storage: 1 (default) = dictionary form whenever the band coefficient tuples of the matrix
 * take <= 256 distinct values (always true for the reference's operator: 27 boundary types + one
 * per conducting domain) — 1 byte per row instead of 56; 0 = plain DIA streams.  Same doubles are
 * multiplied in the same order either way.  Call before ec3d_set_matrix_csr / ec3d_assemble*. */
int ec3d_set_format(ec3d_handle h, int dictionary);
/* 1 (default): ec3d_assemble, ec3d_assemble_slab and ec3d_set_matrix_csr store the A-V system in its
 * structured form when they can (dictionary format on, <= 256 coefficient classes, U ids in scan order):
 * U is embedded in the grid (device vectors hold 4 blocks of planes*pitch rows, pitch >= sdx*sdy), every
 * A<->U coupling is a fixed-offset stencil slot with a class-coded coefficient, and there is no sliced-ELL
 * tail.  ec3d_assemble takes up to 22 conducting domains (55 + 9 D classes) as long as geoPHYS_C's
 * domain-major U numbering (src/vxc2data.f90:624-636) equals scan order, i.e. every domain's cells follow the
 * previous domain's in scan order: the reference's U ROWS are in scan order (src/EC3D.f90:521), and only then is
 * its system a symmetric permutation of the structured one.  ec3d_assemble_slab and ec3d_set_matrix_csr take one
 * conducting domain.  Otherwise bands + tail, which holds the reference's rows and columns as they are.  Host
 * vectors keep the reference's numbering (3*nCells + Ncells0); the library permutes on upload/download.
 * 0: bands + tail. */
int ec3d_set_structured(ec3d_handle h, int on);
/* device row of every unknown of the reference's numbering (n entries); identity unless structured.  Structured:
 * A rows go to their (pitched) cell, the U unknown 3*nCells + m (0-based m) to the U block row of the m-th conducting
 * cell in scan order, which is the cell whose geoPHYS_C is 3*nCells + m + 1; the map increases within each block. */
int ec3d_get_row_map(ec3d_handle h, int32_t *ref_to_dev);

/* Preconditioner of ec3d_solve / ec3d_solve_resident.  EC3D_PRECOND_NONE (default): the reference's
 * iteration, unchanged.  EC3D_PRECOND_MG: right-preconditioned BiCGSTAB with restart whose preconditioner M is
 * one geometric multigrid V-cycle (red-black Gauss-Seidel, `pre` + `post` sweeps per level, mean restriction,
 * piecewise-constant prolongation, `coarse_sweeps` symmetric sweeps on the coarsest level in one workgroup):
 *   p^ = M p; v = A p^; alpha = rho/(r0.v); s = r - alpha v; [exit on ||s||/||b||]
 *   s^ = M s; t = A s^; omega = (t.s)/(t.t); x += alpha p^ + omega s^; r = s - omega t; [exit on ||r||/||b||]
 * Iteration count, itmax exit, ||b|| = 0 return and restart rule are src/solvers.f90:24-50's; resid_hist keeps
 * ||S||, ||R|| of the recurrence (R = b - A x).  Only for a matrix from ec3d_assemble_poisson on a handle of its
 * own: every coarser level reruns that assembly at half the cells and twice the spacing on each axis that is
 * even and >= 8 (same BND), until no axis halves or a level has <= 4096 rows.  Zeros select the defaults
 * (pre = post = 2, coarse_sweeps = 16).  The hierarchy is built at once and freed by ec3d_destroy, by a new
 * matrix or by EC3D_PRECOND_NONE.  Refused, with the handle left as it was: EC3D_PRECOND_E_MATRIX (A-V, CSR
 * without ec3d_set_precond_grid, a slab, a handle of ec3d_multi), EC3D_PRECOND_E_COARSE (the coarsest level has
 * > 4096 rows). */
/* EC3D_PRECOND_BLOCK_MG: the same outer iteration on the structured A-V form (ec3d_assemble with the structured
 * form on, an undivided single-GPU handle), v = A p^ and t = A s^ by the full operator.  M is block diagonal over
 * [Ax | Ay | Az | U]; the A-U couplings are left out of M.  The three A blocks have the same band coefficients in every
 * cell (checked; else EC3D_PRECOND_E_MATRIX), so one hierarchy serves them: level 0 is the handle's matrix, every
 * coarser level the Galerkin product of piecewise-constant aggregation (2 cells along every axis whose extent is > 1,
 * ceil-halving; scaled by 1 / (2 * nominal children)), built on the device until a level has <= 4096 cells; one
 * V-cycle per block as for EC3D_PRECOND_MG, with the mean over the aggregate's actual cells.  The U block gets
 * pre + post red-black Gauss-Seidel sweeps from zero on its unknowns, its right-hand side first projected onto the
 * U block's range (each conducting component's weighted mean taken out).  Rows without a diagonal give 0.  Same defaults
 * (2 / 2 / 16).  Refused with EC3D_PRECOND_E_MATRIX, the handle unchanged: Poisson, bands + tail (CSR, or
 * ec3d_set_structured(h, 0)), a slab, a handle of ec3d_multi, more than 4 conducting domains (the smoothers' class
 * table holds 64 classes, the structured form has 27 + 9 D A-row classes).  ec3d_get_preconditioner reports the A blocks'
 * levels; ec3d_precond_apply applies M on host vectors in the reference's numbering. */
enum { EC3D_PRECOND_NONE = 0, EC3D_PRECOND_MG = 1, EC3D_PRECOND_BLOCK_MG = 2 };
enum { EC3D_PRECOND_E_MATRIX = 20, EC3D_PRECOND_E_COARSE = 21 };
int ec3d_set_preconditioner(ec3d_handle h, int kind, int32_t pre, int32_t post, int32_t coarse_sweeps);
/* kind, number of levels, and (dims != NULL) sdx, sdy, sdz of every level, finest first (3*levels entries) */
int ec3d_get_preconditioner(ec3d_handle h, int *kind, int32_t *levels, int32_t *dims /* 3*levels */);
/* z = M r, one V-cycle on host vectors (H2D, apply, D2H).  Parity probe, like ec3d_spmv.  On an fp32 hierarchy r and z
 * are doubles all the same: r is narrowed by the cycle, z widened exactly. */
int ec3d_precond_apply(ec3d_handle h, const double *r, double *z);
/* Precision of the V-cycle of EC3D_PRECOND_MG.  EC3D_PRECOND_FP64 (default): as above.  EC3D_PRECOND_FP32: M in single
 * precision.  Every level's coefficients are its own fp64 rediscretisation narrowed once (round to nearest) at
 * set-up; the right-hand side of an application is narrowed once; every level vector, product, difference and
 * division of the cycle, the coarse solve included, is fp32 in the fp64 kernels' operation order; p^ and s^ are
 * stored in fp32 and widened (exactly) where the outer iteration reads them.  The outer iteration -- A p^, the dot
 * products, the scalars, s, x, r, p, the exits, the restart rule -- stays fp64, and forms v = A p^ and x += alpha p^
 * from the same p^, so R = b - A x holds as before and the solve reaches the same true residual; only the
 * iteration count may differ.  The hierarchy then holds fp32 vectors only.  The setting belongs to the handle and
 * outlives new matrices and EC3D_PRECOND_NONE; it takes effect at the next ec3d_set_preconditioner and does not
 * rebuild a hierarchy already set.  With EC3D_PRECOND_FP32 set, EC3D_PRECOND_BLOCK_MG is refused
 * (EC3D_PRECOND_E_MATRIX, the handle unchanged).  An unknown value returns 2 and leaves the handle unchanged.
 * ec3d_get_precond_precision: *setting = the handle's setting, *in_use = the precision of the hierarchy now set
 * (EC3D_PRECOND_FP64 when there is none); either may be NULL. */
enum { EC3D_PRECOND_FP64 = 0, EC3D_PRECOND_FP32 = 1 };
int ec3d_set_precond_precision(ec3d_handle h, int32_t precision);
int ec3d_get_precond_precision(ec3d_handle h, int32_t *setting, int32_t *in_use);
/* Coarsening rule of EC3D_PRECOND_MG.  EC3D_COARSEN_REDISCRETIZE (default): as above -- an axis halves only while it is
 * even and >= 8, and a box whose coarsest level stays above 4096 rows is refused (EC3D_PRECOND_E_COARSE).
 * EC3D_COARSEN_AGGREGATE (opt-in): every box gets a hierarchy.  Every axis whose extent is > 1 is ceil-halved
 * (aggregates of 2 cells, the last one 1 cell on an odd axis) until a level has <= 4096 rows.  Level l + 1 is a
 * rediscretisation (1 class byte per row, as above) while no Galerkin level has appeared and every axis of level l is
 * even and >= 8; from the first level that fails this, level l + 1 and every coarser one is the Galerkin product of
 * piecewise-constant aggregation in the arithmetic of EC3D_PRECOND_BLOCK_MG (scaled by 1 / (2 * nominal children)),
 * built on the device in fp64 and kept as seven band streams (56 B per row, 28 B narrowed once under
 * EC3D_PRECOND_FP32).  The restriction is the mean over the aggregate's actual cells.  Where the default rule halves
 * every axis at every level (64^3, 48x40x36) both rules build the same hierarchy and M is the same bits; 100^3 or
 * 500^3 keep their large levels in the 1-byte form, and only a box whose finest level has an odd or short axis
 * (255^3) pays the band form on level 1, at one eighth of the rows.  EC3D_PRECOND_E_COARSE cannot occur; the
 * EC3D_PRECOND_E_MATRIX refusals are unchanged.  The setting belongs to the handle and outlives new matrices and
 * EC3D_PRECOND_NONE; it takes effect at the next ec3d_set_preconditioner and does not rebuild a hierarchy already
 * set.  EC3D_PRECOND_BLOCK_MG has always aggregated and ignores it.  An unknown value returns 2 and leaves the handle
 * unchanged.
 * ec3d_get_precond_coarsening: *setting = the handle's setting; *in_use = the rule of the hierarchy now set
 * (EC3D_COARSEN_REDISCRETIZE when there is none, EC3D_COARSEN_AGGREGATE for EC3D_PRECOND_BLOCK_MG); level_kinds: one
 * entry per level of the hierarchy now set (ec3d_get_preconditioner's count): 0 = the handle's matrix,
 * 1 = rediscretised, 2 = Galerkin.  Any of the three may be NULL. */
enum { EC3D_COARSEN_REDISCRETIZE = 0, EC3D_COARSEN_AGGREGATE = 1 };
int ec3d_set_precond_coarsening(ec3d_handle h, int32_t rule);
int ec3d_get_precond_coarsening(ec3d_handle h, int32_t *setting, int32_t *in_use, int32_t *level_kinds);
/* EC3D_PRECOND_MG for a matrix the caller brings.  ec3d_set_precond_grid says that the matrix ec3d_set_matrix_csr put
 * on the handle is a 7-point operator on an sdx x sdy x sdz box, rows numbered as the reference numbers cells,
 * r = i + j * sdx + k * sdx * sdy; its coefficients may vary from cell to cell and it need not be symmetric.  The
 * statement belongs to the matrix, not to the handle: a new matrix (ec3d_set_matrix_csr, any assembly) clears it.
 * It returns 2 with a message and changes nothing when the handle holds no matrix from ec3d_set_matrix_csr, is a slab
 * or a handle of ec3d_multi, an extent is < 2, or sdx * sdy * sdz != n; only sdx = sdy = sdz = 0 is accepted beside
 * a box, and takes the statement back (no grid, as after a new matrix).  Nothing is checked or built by the call, and
 * a hierarchy already set stays.
 * With a grid set, ec3d_set_preconditioner(h, EC3D_PRECOND_MG, ...) builds a hierarchy from the matrix alone instead of
 * refusing.  First the matrix is checked on the device, in its stored form; EC3D_PRECOND_E_MATRIX, the handle as it
 * was and a message naming the first offending row (1-based) unless: no row has a tail entry; every band offset is one
 * of 0, +-1, +-sdx, +-sdx*sdy (fewer than seven bands is fine: a missing band is zeros); the slots whose neighbour
 * lies beyond an x or y face (-1 at i = 0, +1 at i = sdx - 1, -sdx at j = 0, +sdx at j = sdy - 1) are zero; every
 * row's diagonal is nonzero and finite.  A matrix recognised as the structured A-V form is refused likewise, and so
 * is EC3D_PRECOND_BLOCK_MG on any CSR handle, grid or not.  Level 0 is the handle's own dictionary form -- no copy,
 * 1 class byte per row -- when that has exactly the seven offsets and at most 32 classes; otherwise (variable
 * coefficients with more classes, fewer than seven bands, ec3d_set_format(h, 0)) the seven band streams are gathered
 * once into a copy the hierarchy owns: 56 B per row on top of the handle's matrix, released with the hierarchy, and
 * kept under EC3D_PRECOND_FP32 too (the outer iteration's A p^ reads it) beside the 28 B per row narrowed from it.
 * Level dims are EC3D_COARSEN_AGGREGATE's ceil-halving until a level has <= 4096 rows, and every coarse level is a
 * Galerkin product (there is no BND and no spacing to rediscretise with): ec3d_get_precond_coarsening reports
 * in_use = EC3D_COARSEN_AGGREGATE and level kinds 0, 2, 2, ...  The handle's own coarsening setting is ignored on this
 * path and left as it is; EC3D_PRECOND_E_COARSE cannot occur; ec3d_set_precond_precision applies as above.  Without
 * the call everything is as before: EC3D_PRECOND_MG on a CSR handle is refused with EC3D_PRECOND_E_MATRIX.
 * ec3d_get_precond_grid: dims[0..2] = the grid now set, zeros when none. */
int ec3d_set_precond_grid(ec3d_handle h, int32_t sdx, int32_t sdy, int32_t sdz);
int ec3d_get_precond_grid(ec3d_handle h, int32_t *dims /* 3; zeros when none */);
/* A solve started from the projection onto earlier solutions (opt-in; no reference counterpart: the reference starts
 * from the previous x and nothing else).  With depth m in 1 .. EC3D_GUESS_MAX_DEPTH the handle keeps k <= m pairs
 * (Q_i, A Q_i), oldest first, the A Q_i orthonormal.  In front of every ec3d_solve / ec3d_solve_resident:
 * R = B - A X, c_i = (A Q_i).R, X = X + c_1 Q_1 + ... + c_k Q_k, in that order, every term a rounded product and a
 * rounded sum (Fischer's projection in GCR form: A need not be symmetric); with ||B|| = 0 every c_i is 0, X keeps its
 * bits, iter = 0 and nothing is stored.  Then the solve runs as without a history -- iteration, exits, restart rule and
 * kernels unchanged -- from the new X.  Behind it, whichever exit it took: Q_new = X - X_start (the X the call found),
 * A Q_new by the handle's own SpMV, two passes of classical Gram-Schmidt of A Q_new against the stored A Q_i (Q_new gets
 * the same combination of the Q_i), both scaled by 1 / ||A Q_new||, the oldest pair dropped when k = m.  The new pair is
 * discarded when ||A Q_new|| behind the passes is <= EC3D_GUESS_MIN_NEW times its value before them (noise of the
 * inexact solve, or a null direction of A), and the whole history is cleared when any of these numbers is not finite:
 * a solve that went NaN leaves no trace.  The pairs belong to the matrix: ec3d_set_matrix_csr, every ec3d_assemble*,
 * ec3d_place_vectors and a call that changes the depth clear them; ec3d_upload, ec3d_rhs_step, ec3d_post_update and
 * ec3d_set_preconditioner do not (a preconditioned solve uses them unchanged).  The depth belongs to the handle and
 * outlives new matrices.  Memory: 2 m + 1 library-owned vectors of n_pad doubles (the pairs and X_start), allocated by
 * the first solve after the depth was set, never part of the work vectors (ec3d_adopt_vectors handles work); one host
 * read-back of the deciding scalars per solve.  depth = 0 (default): a solve launches and allocates nothing more and
 * returns the same bits as before.  A depth outside 0 .. EC3D_GUESS_MAX_DEPTH returns 2, a z-slab or a slab of
 * ec3d_multi 4 (the sums would need every rank's), the handle unchanged either way.
 * ec3d_get_guess_history, of the last solve: used = pairs the projection ran on; kept = 1 the new pair was stored,
 * 0 discarded (or ||B|| = 0), -1 the history was cleared; stored = pairs held now; coef[i] = c_i (i < used);
 * res_before / res_after = ||B - A X|| / ||B|| in front of and behind the projection, the latter from the solve's own
 * set-up. */
#define EC3D_GUESS_MAX_DEPTH 8
#define EC3D_GUESS_MIN_NEW 1e-6
int ec3d_set_guess_history(ec3d_handle h, int32_t depth);
typedef struct {
    int32_t depth, stored, used, kept;
    double res_before, res_after;
    double coef[EC3D_GUESS_MAX_DEPTH];
} ec3d_guess_info;
int ec3d_get_guess_history(ec3d_handle h, ec3d_guess_info *info);
/* Left null vectors of the A-V system taken out of every solve's initial residual (opt-in; no reference counterpart;
 * DESIGN.md section 16).  A constant U on one connected conducting component is a right null vector of A, so A has a
 * left null vector w per component, every residual keeps w.r = w.b, and no iterate gets below |w.b| / ||w||: the
 * floor the reference's tolerances sit just above.  With the setting on, the first solve on a matrix finds the
 * connected components of the conducting cells (6-neighbourhood, scan order of their first cell) and for each the
 * U row m of its middle cell, solves A^T y = -A^T e_m from y = 0 by the reference's BiCGSTAB with restart (operator
 * ec3d_spmv_t's kernel) to null_tol, at most 20 n^(1/3) + 2000 iterations, and sets w = y + e_m.  The w are
 * orthonormalised by classical Gram-Schmidt in component order (fixed-order sums); one that keeps less than
 * EC3D_NULL_MIN_KEEP of its norm is dropped and counted.  Every solve then replaces R = B - A X by R - Q (Q^T R)
 * before R0, P and R.R are taken: since (I - Q Q^T) A = A this is the solve of A x = (I - Q Q^T) b.  B itself, ||b||,
 * the exits, the restart rule and the iteration's kernels are untouched; the tolerance then reachable is about the
 * adjoint residual times what was removed.  A w that did not reach null_tol is never used: the solve returns
 * EC3D_NULL_E_SETUP with the component named in the error text.  Q belongs to the matrix (a new matrix clears it, the
 * next solve rebuilds it); the setting belongs to the handle.  Applies to the structured form of ec3d_assemble on an
 * undivided handle; on a Poisson, CSR or bands + tail matrix ec3d_set_null_projection(h, 1, ..) returns
 * EC3D_NULL_E_MATRIX, on a z-slab or a slab of ec3d_multi 4, and the setting stays off; a solve that finds such a
 * matrix under a setting made earlier returns the same status.  on = 0 (default): a solve launches and allocates
 * nothing more and returns the same bits as before.  null_tol <= 0: the default 1e-10.
 * ec3d_get_null_projection: built = Q exists for the present matrix; found / kept / dropped components; of the first
 * EC3D_NULL_MAX_REPORT components the seed row (0-based, the reference's numbering), the adjoint solve's iterations,
 * ||A^T w|| / ||w|| and whether it was kept; removed = ||Q^T R|| / ||b|| of the last solve; setup_ms = wall time of the
 * set-up.  ec3d_left_null_vector: kept vector `index` of Q (n doubles, the reference's numbering); builds Q when the
 * setting is on and it does not exist yet. */
#define EC3D_NULL_MAX_REPORT 32
#define EC3D_NULL_MIN_KEEP 1e-6
#define EC3D_NULL_E_MATRIX 22
#define EC3D_NULL_E_SETUP 23
int ec3d_set_null_projection(ec3d_handle h, int32_t on, double null_tol);
typedef struct {
    int32_t on, built;
    int32_t found, kept, dropped, reported;
    double null_tol;
    double removed;
    double setup_ms;
    int64_t seed_row[EC3D_NULL_MAX_REPORT];
    int32_t iterations[EC3D_NULL_MAX_REPORT];
    int32_t was_kept[EC3D_NULL_MAX_REPORT];
    double residual[EC3D_NULL_MAX_REPORT];
} ec3d_null_info;
int ec3d_get_null_projection(ec3d_handle h, ec3d_null_info *info);
int ec3d_left_null_vector(ec3d_handle h, int32_t index, double *w_host);
/* A preconditioner N ~ (A^T)^-1 for the adjoint solves of that set-up (opt-in): the block
 * multigrid of EC3D_PRECOND_BLOCK_MG, transposed.  N is block diagonal over [Ax | Ay | Az | U].  A blocks: the
 * hierarchy and V-cycle of EC3D_PRECOND_BLOCK_MG on the transposed block (EC3D_NULL_PRECOND_BLOCK_MG: level 0 is the
 * transposed block, gathered once into seven band streams; coarse levels its Galerkin products) or on the block of A as
 * it stands (EC3D_NULL_PRECOND_BLOCK_MG_A).  U block, both kinds: the plain mean of every conducting component leaves
 * the right-hand side, pre + post red-black sweeps from zero run on U^T, and the plain mean leaves the result.  The
 * adjoint iteration is then the right-preconditioned BiCGSTAB of ec3d_set_preconditioner around ec3d_spmv_t's kernel:
 * the residual tested is the true one, so null_tol, the cap, EC3D_NULL_E_SETUP and ec3d_null_info mean what they meant.
 * The hierarchy is built inside the set-up and released before it returns; the handle's own preconditioner is not
 * touched.  pre / post / coarse_sweeps = 0: the defaults of ec3d_set_preconditioner.  The setting stays with the
 * handle across matrices; changing it clears vectors already built.  Status: as ec3d_set_null_projection
 * (EC3D_NULL_E_MATRIX, 4); an unknown kind or a negative count 2; with a matrix on the handle, what the block
 * hierarchy refuses (A blocks that differ, more than 4 conducting domains) EC3D_PRECOND_E_MATRIX, the setting as it
 * was.  EC3D_NULL_PRECOND_NONE (default): the set-up launches what it launched before and returns the same bits.
 * ec3d_get_null_precond: the kind set; levels and dims (3 per level, at most EC3D_NULL_PRECOND_MAX_LEVELS levels) of
 * the hierarchy the last set-up built (0 levels when none was built) and the wall time spent building it.
 * ec3d_null_precond_apply: z = N r on host vectors in the reference's numbering; builds N for the call and releases
 * it (status 3 when the kind is EC3D_NULL_PRECOND_NONE). */
#define EC3D_NULL_PRECOND_NONE 0
#define EC3D_NULL_PRECOND_BLOCK_MG 1
#define EC3D_NULL_PRECOND_BLOCK_MG_A 2
#define EC3D_NULL_PRECOND_MAX_LEVELS 16
int ec3d_set_null_precond(ec3d_handle h, int32_t kind, int32_t pre, int32_t post, int32_t coarse_sweeps);
int ec3d_get_null_precond(ec3d_handle h, int32_t *kind, int32_t *levels, int32_t *dims, double *hierarchy_ms);
int ec3d_null_precond_apply(ec3d_handle h, const double *r, double *z);

/* ------------------------------------------------------------------------------------------
 * 2b. Multi-rank building blocks (z-slab decomposition, one process per GPU).
 *     No reference counterpart: the reference is serial.  The host
 *     (eddy_currents_3d_amd/dist.py) owns the communicator; between stages it exchanges the halo
 *     planes of P and S with the z-neighbours and all-gathers the 8 per-rank partial sums.
 * ---------------------------------------------------------------------------------------- */
/* launch on a caller-owned HIP stream (e.g. torch's current stream); NULL = the library's own */
int ec3d_set_stream(ec3d_handle h, void *hip_stream);
/* planes [k0, k1) (0-based) of the ec3d_assemble_poisson operator: n = (k1-k0)*sdx*sdy rows; the
 * z-neighbour planes are read from the vectors' ghost zones: v[-kdz..0) and v[n..n+kdz) */
int ec3d_assemble_poisson_slab(ec3d_handle h, int32_t sdx, int32_t sdy, int32_t sdz, int32_t k0, int32_t k1,
                               const double *BND, const double *delta);
/* One z-slab of the full A-V system (ec3d_assemble) on an EXTENDED grid: the handle holds planes
 * [e0, e1) of the global grid = the owned planes [k0, k1) plus two halo planes on every interior side
 * (the one-sided A-U stencils reach two cells, src/EC3D.f90:697-706).  geoPHYS_ext / geoPHYS_C_ext
 * cover the extended planes; geoPHYS_C_ext numbers the conducting cells of the extended slab in
 * scan order (3*nCells_ext + m).  Local unknowns [Ax_ext | Ay_ext | Az_ext | U_ext]; rows of halo
 * planes are inert and excluded from every dot product; their vector entries are filled by the
 * host's halo exchange (contiguous ranges, eddy_currents_3d_amd/dist.py). */
int ec3d_assemble_slab(ec3d_handle h, int32_t sdx, int32_t sdy, int32_t sdz, int32_t e0, int32_t e1, int32_t k0,
                       int32_t k1, const int8_t *geoPHYS_ext, const int32_t *geoPHYS_C_ext, const double *valPHYS,
                       int32_t nsub_glob, const double *BND, const double *delta, double dt);
/* every work vector is [ghost | n_pad | ghost] doubles; halo = doubles per z-plane (0 if not a slab) */
int ec3d_vector_layout(ec3d_handle h, int64_t *ghost, int64_t *n, int64_t *n_pad, int64_t *halo);
/* use caller-owned, zero-filled device memory (EC3D_NVEC * (2*ghost + n_pad) doubles) for the vectors */
int ec3d_adopt_vectors(ec3d_handle h, double *device_base);
/* reductions then come from gsum_device[nranks][8] (the all-gather of every rank's lsum_device[8]); from then
 * on the handle is driven stage by stage (ec3d_dist_step) and ec3d_solve / ec3d_iterate / ec3d_time_* refuse
 * it.  ec3d_dist_configure(h, 1, NULL, NULL) leaves that mode again; so does a new matrix. */
int ec3d_dist_configure(ec3d_handle h, int32_t nranks, double *lsum_device, double *gsum_device);
enum { EC3D_STAGE_RESID = 0, /* R = B - A X, R0 = P = R; lsum <- B.B, R.R      src/solvers.f90:14-21 */
       EC3D_STAGE_SETUP = 1, /* Bnorm, rr0 from gsum                                            :21-23 */
       EC3D_STAGE_K1 = 2,    /* AP = A P; lsum <- AP.R0        (P halo must be current)          :30-32 */
       EC3D_STAGE_K2 = 3,    /* alpha, S = R - alpha AP; partials of S.S (collapsed by K3's stage) :32-34 */
       EC3D_STAGE_K3 = 4,    /* AS = A S; lsum <- S.S (K2's), AS.S, AS.AS (S halo current; no gather
                                needed between K2 and K3: the S exit is taken by K4)              :39-40 */
       EC3D_STAGE_K4 = 5,    /* S exit (X += alpha P) or omega, X, R; lsum <- R.R, R.R0          :34-44 */
       EC3D_STAGE_K5 = 6,    /* R exit, beta, P, restart                                         :43-49 */
       /* K1 and K3 in two launches, so the halo exchange of P / S overlaps the first one:
        * *_INT = owned planes 1 .. np-2 (need no halo), *_BND = planes 0 and np-1 (after the exchange;
        * also collapses both launches' partials into lsum).  Only when ec3d_can_overlap(). */
       EC3D_STAGE_K1_INT = 7, EC3D_STAGE_K1_BND = 8, EC3D_STAGE_K3_INT = 9, EC3D_STAGE_K3_BND = 10,
       /* The other way to hide the exchange, for any slab and storage format: the PRODUCERS of the
        * exchanged vectors run in two launches -- *_BND first (the tiles holding the rows the neighbours
        * receive, ec3d_dist_set_boundary_rows), then the exchange starts, then *_INT (everything else)
        * while the planes travel.  K2 produces S (both launches' S.S partials are collapsed by K3's stage),
        * K5 produces P. */
       EC3D_STAGE_K2_BND = 11, EC3D_STAGE_K2_INT = 12, EC3D_STAGE_K5_BND = 13, EC3D_STAGE_K5_INT = 14,
       /* A slab that runs the THREE-launch iteration (in-library / RCCL drivers only: it needs the library's own spare
        * buffers; stage 3 is then K2-in-K3, stage 4 K4 in SpMV form, stage 5 K5-in-K1): the producers of the exchanged
        * vectors -- K4 makes R, K5-in-K1 makes the next AP -- in two launches, planes 0 and np-1 first (*_BND), then the
        * exchange starts, then planes 1 .. np-2 (*_INT, which also collapses both launches' partial sums). */
       EC3D_STAGE_K4F_BND = 15, EC3D_STAGE_K4F_INT = 16, EC3D_STAGE_K5F_BND = 17, EC3D_STAGE_K5F_INT = 18 };
int ec3d_dist_step(ec3d_handle h, int32_t stage, int32_t it, double tolerance);
/* Device-row ranges [lo, hi) this rank sends AND receives in a halo exchange (the first/last owned planes
 * of every block; the halo rows of an extended slab, which the interior launch must not overwrite once
 * the exchange has started); *enabled = 1 when the K2/K5 boundary/interior stages can be used (0: no range given, or every
 * tile touches a boundary). */
int ec3d_dist_set_boundary_rows(ec3d_handle h, int32_t nranges, const int64_t *lo, const int64_t *hi,
                                int32_t *enabled);
/* 1 when the slab held can run K1/K3 split into interior + boundary launches (single-component slab
 * on a grid whose xy-plane is a whole number of 512-row tiles, at least 10 planes) */
int ec3d_can_overlap(ec3d_handle h);
/* Without draining: enqueue, on the handle's stream, a copy of the stop flag into PINNED host memory
 * (2147483647 while running, else the iteration at which an exit was taken); the caller records an event
 * behind it and reads the value once the event has completed -- lets a multi-rank driver keep a chunk of
 * iterations in flight while it looks at the previous one (as ec3d_solve does on a single device). */
int ec3d_read_state_async(ec3d_handle h, int32_t *stop_iter_pinned);
/* drain the stream and read the device-resident state; stop_iter = -1 while still running */
int ec3d_read_state(ec3d_handle h, int32_t *stop_iter, int32_t *stop_kind, double *bnorm);
/* how often the restart rule R0 = R, P = R (src/solvers.f90:47-49) fired during the last solve on this handle
 * (drains the stream): lets a test assert that a parity case really went through the restart branch */
int ec3d_get_restart_count(ec3d_handle h, int32_t *count);

/* ------------------------------------------------------------------------------------------
 * 2c. Multi-GPU behind one handle: one process, N devices, invisible to the caller (SURVEY §8b
 *     "Threading": the caller of src/EC3D.f90:408 is single-threaded and must not have to know).
 *     The library cuts the grid into z-slabs (rank g owns planes [g*sdz/N, (g+1)*sdz/N), lower ranks
 *     take the remainder), keeps one host thread per slab, pulls the halo planes of P and S from the
 *     z-neighbours' memory over xGMI (peer access) while the interior planes compute, and lets every
 *     kernel read the N ranks' partial sums in place, added in rank order -- the schedule of §2b and of
 *     eddy_currents_3d_amd/dist.py, results bit-identical to it.  sprsbcgstabwr_ uses this path when the
 *     environment says EC3D_NGPU=N (N > 1) and the matrix is recognised as the reference's A-V system.
 *     devices == NULL: devices 0 .. nranks-1 (status 103 "needs N devices" when the machine has fewer);
 *     an explicit list may name a device several times (several slabs on one GPU: tests, rehearsals).
 * ---------------------------------------------------------------------------------------- */
typedef struct ec3d_multi *ec3d_multi_handle;
int ec3d_multi_create(ec3d_multi_handle *mh, int32_t nranks, const int32_t *devices);
/* ONE PROCESS PER GPU (the launch form of torch.distributed.run / mpirun): the same handle and the same calls, but this
 * process holds ONE slab -- rank `rank` of `nranks` -- on `device`, and RCCL carries what crosses the ranks: the halo
 * planes as ncclSend / ncclRecv pairs in one group on a side stream (beside the interior launch), the eight partial
 * sums of every rank by ncclAllGather on the compute stream, added in rank order by the consumer kernels.  The whole
 * iteration loop is enqueued from C++.  id_halo, id_sum: two RCCL unique ids (128 bytes each), made by
 * ec3d_rccl_unique_id on ONE rank and handed to all of them by the launcher's own means (the Python host uses the
 * torch.distributed store; an MPI host would broadcast them); the call returns when every rank has made it.  Host
 * vectors (ec3d_multi_upload / _download / _solve, the time loop's source lists) are GLOBAL on every rank, each rank
 * takes and fills its own planes.  RCCL is loaded at run time (librccl.so.1; status 109 when it is missing).
 * as_world > 0 (with nranks = 1): a REHEARSAL of rank as_rank of as_world on one GPU -- that rank's slab, plan, launches
 * and RCCL calls, every neighbour mapped to this process itself; for timing, not for results. */
int ec3d_rccl_unique_id(void *id128);
int ec3d_multi_create_rank(ec3d_multi_handle *mh, int32_t rank, int32_t nranks, int32_t device, const void *id_halo,
                           const void *id_sum, int32_t as_rank, int32_t as_world);
int ec3d_multi_destroy(ec3d_multi_handle mh);
int ec3d_multi_ranks(ec3d_multi_handle mh);
/* the slab of one rank (an ordinary handle in multi-rank mode: introspection only) and its planes */
int ec3d_multi_slab(ec3d_multi_handle mh, int32_t rank, ec3d_handle *h, int32_t *k0, int32_t *k1);
/* as ec3d_set_format / ec3d_set_structured for every slab; -1 leaves a setting as it is */
int ec3d_multi_set_format(ec3d_multi_handle mh, int dictionary, int structured);
/* same arguments as ec3d_assemble_poisson / ec3d_assemble / ec3d_set_matrix_csr: GLOBAL tables in */
int ec3d_multi_assemble_poisson(ec3d_multi_handle mh, int32_t sdx, int32_t sdy, int32_t sdz, const double *BND,
                                const double *delta);
int ec3d_multi_assemble(ec3d_multi_handle mh, int32_t sdx, int32_t sdy, int32_t sdz, const int8_t *geoPHYS,
                        const int32_t *geoPHYS_C, const double *valPHYS, int32_t nsub_glob, const double *BND,
                        const double *delta, double dt);
/* CSR triple of the whole system (src/EC3D.f90:36-38): must be recognisable as the reference's A-V system
 * on a grid (ec3d_probe_csr) or as a single-component 7-point operator on one (seven bands at -kdz, -sdx, -1, 0,
 * 1, sdx, kdz and nothing else: src/EC3D.f90:528-654 without conducting cells), which is then cut into slabs;
 * status 7 otherwise (use one GPU).  The seven-band reading goes by the offsets, not the values: wrap slots may hold
 * nonzero coefficients, they multiply the linear neighbour as on one GPU (a slab's ghost zone is a whole plane, which
 * covers x[r +- 1] and x[r +- sdx] of its first and last rows) */
int ec3d_multi_set_matrix_csr(ec3d_multi_handle mh, int32_t n, const double *valA, const int32_t *irow,
                              const int32_t *jcol);
/* host vectors in the reference's global numbering [Ax | Ay | Az | U], n unknowns (ec3d_multi_size) */
int ec3d_multi_size(ec3d_multi_handle mh, int64_t *n);
int ec3d_multi_upload(ec3d_multi_handle mh, int which, const double *host);
int ec3d_multi_download(ec3d_multi_handle mh, int which, double *host);
int ec3d_multi_solve(ec3d_multi_handle mh, const double *b, double *x, double tolerance, int32_t itmax,
                     int32_t *iter);
int ec3d_multi_solve_resident(ec3d_multi_handle mh, double tolerance, int32_t itmax, int32_t *iter);
/* the time loop around the solve, as ec3d_rhs_step / ec3d_post_update / ec3d_vtk_fields (global ids,
 * global output arrays); the X halo planes are refreshed inside */
int ec3d_multi_rhs_step(ec3d_multi_handle mh, int32_t moving, int32_t nsrc, const int32_t *src_index,
                        const double *src_value);
int ec3d_multi_post_update(ec3d_multi_handle mh);
/* y = A*x over the slabs, host vectors in the global numbering (as ec3d_spmv): parity probe of the slab
 * operators and of the halo exchange together -- the rows the exchange is to fill hold NaN until it has */
int ec3d_multi_spmv(ec3d_multi_handle mh, const double *x, double *y);
int ec3d_multi_true_residual(ec3d_multi_handle mh, double *rel, double *bnorm); /* as ec3d_true_residual */
int ec3d_multi_vtk_fields(ec3d_multi_handle mh, const double *delta, float *field_A, float *field_eddy,
                          float *field_source, float *field_B);
/* ec3d_vtk_fields_begin / _wait over the slabs: _begin enqueues every slab's field kernel and its copy into that
 * slab's pinned buffers and returns; _wait blocks on ONE slab's copy and hands out its part -- cells cell0 ..
 * cell0 + ncells of every vector (consecutive in field_N.vtk, src/utilites.f90:222-289); field_eddy = NULL for a
 * slab that holds no conductor (zeros in the file) */
int ec3d_multi_vtk_fields_begin(ec3d_multi_handle mh, const double *delta, int32_t big_endian, int32_t *slot);
int ec3d_multi_vtk_fields_wait(ec3d_multi_handle mh, int32_t slot, int32_t rank, const float **field_A,
                               const float **field_eddy, const float **field_source, const float **field_B,
                               int64_t *cell0, int64_t *ncells);
/* bench "steps" as ec3d_iterate_begin / ec3d_iterate: every rank's thread enqueues the iterations and
 * returns; ec3d_multi_synchronize drains all devices.  kernel_ms (5 doubles): rank 0's stage averages. */
int ec3d_multi_iterate_begin(ec3d_multi_handle mh);
int ec3d_multi_iterate(ec3d_multi_handle mh, int32_t first_iter, int32_t count, double *kernel_ms);
int ec3d_multi_synchronize(ec3d_multi_handle mh);
/* The instrumented pass with the synchronisation points bracketed as well, for local slab `rank` (0 on a one-process-per-GPU
 * handle): kernel_ms[5] as above; sync_ms[0] / sync_n[0]: per iteration, how long that slab's compute stream stood at its
 * reduction points (collapse of the partial sums + all-gather / event tree; the dot products of src/solvers.f90:31-44) and how
 * many it has; sync_ms[1] / sync_n[1]: the same for the waits for halo planes in front of the SpMV stages (src/solvers.f90:30,
 * :39).  Events on the compute stream around each point: what the NEXT kernel waited there, not the transport's own time. */
int ec3d_multi_iterate_timed(ec3d_multi_handle mh, int32_t first_iter, int32_t count, int32_t rank, double *kernel_ms,
                             double *sync_ms, int32_t *sync_n);
/* one process per GPU (ec3d_multi_create_rank): what the RCCL in use says about the job -- ranks of the communicator the sums
 * travel on (ncclCommCount), library version (ncclGetVersion; -1: the tests' loopback stand-in), and the file the entry points
 * were resolved from (librccl.so.1 of the process / the system, or what EC3D_RCCL_LIB names) */
int ec3d_multi_rccl_info(ec3d_multi_handle mh, int32_t *nranks, int32_t *version, char *path, int32_t path_cap);
/* HIP runtime calls (kernel launches, event records and waits, copies) that rank `rank`'s host thread issued per
 * iteration during the last ec3d_multi_iterate: the host-side price of one pass of src/solvers.f90:24-50 on N GPUs */
int ec3d_multi_api_calls(ec3d_multi_handle mh, int32_t rank, double *per_iteration);
/* The schedule the job runs (one value for all ranks: the exchanges are part of it).  plan: 0 = five launches, halo
 * exchange in front of K1 and K3; 1 = K1 / K3 as interior + boundary launch with the exchange behind the interior one;
 * 2 = K2 / K5 boundary tiles first (A-V slabs); 3 = three launches per iteration (K2 inside K3, K4 as an SpMV kernel, K5
 * inside the next K1 -- every rank >= 32 Mi rows of the single-component operator): AP and R travel instead of P and S;
 * 4 = the same with K4 and K5-in-K1 -- the producers of R and AP -- as boundary + interior launch around the exchange;
 * 5 = 1 and 2 together: K2 / K5 boundary planes first and K1 / K3 interior planes first, the exchange behind two launches
 * (asked for with EC3D_SLAB_PLAN=5, the same on every rank: opt-in until a job of two real devices has verified it).
 * x_every: iterations between two applications of X = X + alpha*P + omega*S (src/solvers.f90:41; 1 = every iteration). */
int ec3d_multi_plan(ec3d_multi_handle mh, int32_t *plan, int32_t *x_every);
/* rows (8 bytes each, per exchanged vector) local slab `rank` sends to / receives from its z-neighbours in ONE halo exchange:
 * a plane per neighbour for the single-component operator; for the A-V system a plane of each of A_x, A_y, A_z and -- only
 * where they hold a conductor cell -- two planes of U (the other rows of the U block are zero in every vector) */
int ec3d_multi_halo_rows(ec3d_multi_handle mh, int32_t rank, int64_t *sent, int64_t *received);

/* ------------------------------------------------------------------------------------------
 * 3. Introspection / measurement
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_pad;     /* rows swept by every kernel (n rounded up to the tile)         */
    int32_t tile;      /* rows per tile = 2 * threads                                   */
    int32_t nblk;      /* workgroups per launch                                         */
    int32_t threads;   /* 256                                                           */
    int32_t xcd_group; /* S in the XCD-aware blockIdx -> tile map (0: plain grid stride) */
    int32_t zm_tpp;    /* > 0: z-marching map, tiles per xy-plane                          */
    int32_t zm_pps;    /*      planes per z segment                                        */
    int32_t ntiles_front; /* tiles swept by the map above (all of them unless structured A-V form)  */
    int32_t ulist_n;   /* structured A-V form: occupied tiles of the U block, visited afterwards,
                          workgroup b taking entries b, b+nblk, ... of ec3d_get_ulist()             */
    int32_t patch_x, patch_y; /* > 0: a tile of this sweep is a patch of patch_x x patch_y grid cells (2-D tiles of   */
    int32_t patch_sdx;        /* the z-marching SpMV kernels on a grid with rows of patch_sdx cells): tile q of a plane
                                 is patch (q % (patch_sdx/patch_x), q / (patch_sdx/patch_x)); thread t owns the cells
                                 2t, 2t + 1 of the patch in row-major order (idle when 2t >= patch_x * patch_y)       */
    int32_t patch_pitch;      /* device rows from one xy plane to the next (>= patch_sdx * patch_sdy) and grid rows   */
    int32_t patch_sdy;        /* per plane: rows of the last patch row beyond patch_sdy do not exist (idle threads);
                                 tile T lies in plane T / zm_tpp, first row of thread t =
                                 (T / zm_tpp) * patch_pitch + (py * patch_y + 2t / patch_x) * patch_sdx + px * patch_x
                                 + 2t % patch_x, (px, py) = the patch's position in the plane                          */
} ec3d_geom;
/* which = 0: K4 (dots R.R, R.R0); 1: SpMV kernels (B.B, initial R.R, AP.R0, AS.S, AS.AS); 2: K2 (dot S.S) */
int ec3d_get_reduction_geometry(ec3d_handle h, int which, ec3d_geom *g);
int ec3d_get_ulist(ec3d_handle h, int32_t *tiles); /* ulist_n entries */
/* Dictionary-form matrices on a grid that divides into 2-D tiles: one byte per patch tile (tile = plane * tiles per
 * plane + patch, as ec3d_geom numbers them), 1 = every class byte of the tile equals the one a plane below -- a
 * z-marching workgroup keeps its class bytes in registers over such a step.  *count = number of flags (0: this matrix
 * has none and the kernels load the class bytes at every step); flags == NULL: the count only; at most cap are written. */
int ec3d_get_class_runs(ec3d_handle h, int64_t *count, uint8_t *flags, int64_t cap);
/* Patch rows per workgroup of one kind of launch on the 2-D tiles: 4, or 8 where two y-adjacent patch columns are marched
 * by one workgroup of 512 threads ("paired": their common boundary travels through LDS; results are the same bits).
 * kind 0: the bare SpMV (k_spmv); 1: K2 inside K3; 2: K5 inside K1; 3: K4 in SpMV form (its launches that leave X alone);
 * 4: the setup residual, K1 and K3.  *rows = 0 on a handle without 2-D tiles.  EC3D_PATCH=2 pairs wherever the grid allows, EC3D_PATCH=1 never. */
int ec3d_get_patch_rows(ec3d_handle h, int kind, int32_t *rows);
/* How K5 inside K1 (three-launch iteration on the 2-D tiles) gets the old AP it forms the new P from: *computed = 1: for the
 * cells of a workgroup's own patch it sums A*P_old again from the old P it holds anyway, and loads AP only on the rim rows,
 * the edge cells and at a segment's first step (8 B per row less to fetch, the same bits: the stored AP is that very sum);
 * 0: AP is loaded everywhere.  Only the undivided single-GPU dictionary cube has the computing form; z-slabs, the
 * five-launch iteration, plain DIA and the structured A-V kernels report 0.  EC3D_K51_AP=0/1 forces either. */
int ec3d_get_k51_ap_form(ec3d_handle h, int32_t *computed);
/* The tiles (512 rows each) every workgroup of a launch visits, in order: workgroup w visits
 * tiles[offsets[w] .. offsets[w+1]).  which as above.
 * Each thread t of a workgroup owns rows tile*512 + 2t, 2t+1 (or the two cells of a patch, ec3d_geom::patch_x) and
 * adds its products in this order -- the summation order the oracle's twin reproduces.  Two-pass: offsets == NULL -> *nwg and *total only. */
int ec3d_get_visit_order(ec3d_handle h, int which, int32_t *nwg, int64_t *total, int32_t *offsets, int32_t *tiles);
/* 1 (default): SpMV kernels walk the z direction per workgroup and keep x[r-kdz], x[r] in registers
 * when a grid plane is a whole number of 512-row tiles; 0: plain tile order. */
int ec3d_set_zmarch(ec3d_handle h, int on);
int ec3d_set_workgroups(ec3d_handle h, int32_t nblk); /* 0 = default; multiple of 8 enables the XCD map */

typedef struct {
    int64_t n, n_pad, nnz;
    int32_t nbands;
    int32_t band_offset[16];
    int64_t tail_rows, tail_entries_padded; /* sliced-ELL tail */
    int64_t device_bytes;
    int32_t dict_classes; /* > 0: bands stored as 1 class byte per row + a table of that many 7-tuples */
} ec3d_matrix_info;
int ec3d_get_matrix_info(ec3d_handle h, ec3d_matrix_info *info);

/* Plain band streams of >= 32 Mi rows: where the driver puts them decides how fast the SpMV runs (1.70 ... 2.01 ms at
 * 512^3 from one allocation to the next), so the library looks at up to 8 placements when such a matrix is first set
 * on a handle (at most ~0.4 s; once per handle and size: the chosen allocation is kept across ec3d_set_matrix_csr /
 * ec3d_assemble_poisson calls of the same size) and keeps the fastest.  This reports what it saw: *tried candidates,
 * their SpMV times in microseconds (the first `cap` of them), and which one was kept; *tried = 0: no probe ran. */
int ec3d_get_band_placement(ec3d_handle h, int32_t cap, double *candidate_us, int32_t *tried, int32_t *kept);

/* Work vectors of >= 32 Mi rows under the three-launch iteration (a handle that owns them and is no z-slab): the physical pages they land on are worth
 * 2-3 % of the iteration at 512^3, so the library looks at up to EC3D_PLACE_VEC (default 6) allocations of vectors + rings
 * when such a matrix is first set on a handle -- a right-hand side of ones iterated on each, at most ~0.3 s, once per handle
 * and size (the chosen allocation is kept for the next matrix of that size) -- and keeps the fastest; vectors and state
 * are left as if nothing had run.  This reports what it saw: *tried candidates, their times per iteration in microseconds
 * (the first `cap`), which one was kept, and what the search cost (*search_ms; may be NULL); *tried = 0: no probe ran. */
int ec3d_get_vector_placement(ec3d_handle h, int32_t cap, double *candidate_us, int32_t *tried, int32_t *kept,
                              double *search_ms);
/* The same search on request: at any size, with `candidates` allocations (>= 2), on a handle that has a matrix, owns its
 * vectors and is no z-slab (4 otherwise).  EVERY work vector is zero afterwards (X, B and the warm start included): call it
 * before uploading anything.  The vectors may live in another allocation afterwards: every pointer ec3d_device_vector
 * returned before this call is invalid, ask again. */
int ec3d_place_vectors(ec3d_handle h, int32_t candidates);

/* Host-only check (no GPU needed, no handle): would ec3d_set_matrix_csr / sprsbcgstabwr_ store this
 * matrix in the structured A-V form?  structured = 0 means bands + tail (still exact, slower on the U
 * couplings).  The test is the one the library runs: every entry of the matrix gen_sparse_matrix builds
 * (src/EC3D.f90:465-1049) must land in a stencil slot, rows stored in ascending column order. */
typedef struct {
    int32_t structured;
    int32_t sdx, sdy, sdz;   /* grid found                                                     */
    int32_t n_cond;          /* conducting cells = U unknowns                                   */
    int32_t classes;         /* distinct 16-coefficient rows (<= 256)                           */
    int32_t plane_pitch;     /* device rows per xy plane (>= sdx*sdy, whole tiles when pitched) */
} ec3d_csr_probe;
int ec3d_probe_csr(int32_t n, const double *valA, const int32_t *irow, const int32_t *jcol,
                   ec3d_csr_probe *out);

/* Host-only as well: would ec3d_multi_set_matrix_csr / sprsbcgstabwr_ under EC3D_NGPU=nranks cut this matrix into
 * nranks z-slabs?  *cuttable = 0 leaves the reason in ec3d_last_error(): neither the structured A-V form nor a
 * single-component 7-point operator, fewer than two planes per rank (A-V) or fewer planes than ranks. */
int ec3d_probe_csr_multi(int32_t n, const double *valA, const int32_t *irow, const int32_t *jcol, int32_t nranks,
                         int32_t *cuttable);

/* Time `reps` back-to-back launches of one kernel with hipEvents on the library's stream and
 * return the average per launch in milliseconds.  kernel: */
enum { EC3D_K_SPMV = 0,   /* y = A p                        72 B/row             */
       EC3D_K1 = 1,       /* AP = A P, AP·R0                80 B/row                          */
       EC3D_K2 = 2,       /* S = R - a AP, S·S              24 B/row                          */
       EC3D_K3 = 3,       /* AS = A S, AS·S, AS·AS          72 B/row                          */
       EC3D_K4 = 4,       /* X, R updates, R·R, R·R0        56 B/row                          */
       EC3D_K5 = 5 };     /* P update                       32 B/row                          */
int ec3d_time_kernel(ec3d_handle h, int kernel, int32_t reps, double *ms_per_launch);

/* Run exactly `iters` BiCGSTAB iterations on the resident b/x (convergence exits disabled),
 * timed with hipEvents on the library's stream; the bench "step". */
int ec3d_time_iterations(ec3d_handle h, int32_t iters, double *ms_total);

/* The same as asynchronous launches for a caller that does its own timing (bench.py):
 * ec3d_iterate_begin sets up R, R0, P from the resident b/x with exits disabled; ec3d_iterate
 * enqueues iterations first_iter .. first_iter+count-1 and returns without synchronising.
 * With kernel_ms != NULL (5 doubles, K1..K5) it brackets every launch with hipEvents on the
 * library's stream, synchronises, and returns each kernel's average duration in ms.
 * On large single-rank problems with 2-D tiles an iteration is three launches: K2 runs inside K3 and K5 inside
 * the NEXT iteration's K1; stages 1 (after the first iteration) and 2 are then empty and report ~0 ms, stage 3 is
 * K2 + K3, stage 5 is K5 + K1 (EC3D_FUSE23=0 EC3D_FUSE51=0 restore five launches). */
int ec3d_iterate_begin(ec3d_handle h);
int ec3d_iterate(ec3d_handle h, int32_t first_iter, int32_t count, double *kernel_ms);
/* which of the two fusions this handle runs (decided by size and tile shape when the matrix is set): *k2_in_k3 = 1:
 * stage 2 launches nothing and stage 3 is K2 + K3 (ec3d_time_kernel(EC3D_K2) then fails with status 5); *k5_in_k1 = 1:
 * stage 5 is K5 + the next iteration's K1 and stage 1 launches K1 only where the previous launch was not the
 * preceding iteration's stage 5; P / AP then alternate between two buffers and ec3d_download / ec3d_device_vector
 * hand out the current one. */
int ec3d_get_fusion(ec3d_handle h, int32_t *k2_in_k3, int32_t *k5_in_k1);
/* iterations between two updates of X on this handle: 1 = X = X + alpha*P + omega*S in every iteration's K4
 * (src/solvers.f90:41 where it stands); D > 1 (three-launch iteration on vectors far beyond the caches): K4 leaves X
 * alone in D - 1 of D iterations and applies the D updates, in order and each as its own two rounded additions, in the
 * D-th -- nothing in the loop reads X, so X is the same bits; an exit applies what is pending before the solve returns */
int ec3d_get_x_interval(ec3d_handle h, int32_t *iterations);
/* second_stream = 1: with the X update deferred, NO K4 touches X; every group of D updates is applied by a launch of its own
 * (k_x_group) on a second HIP stream beside the iterations that follow, P and S kept in rings of two groups -- the same
 * additions in the same order, the same X.  Meant for z-slabs of a multi-GPU job, whose iteration waits for halo planes
 * and gathered sums (EC3D_XASYNC=1; off by default: one card shows 0 ... 2 %).  groups_launched:
 * such launches since the last solve / ec3d_iterate_begin started (tests).
 * second_stream = 2: the same launches on the iteration's OWN stream, each behind the K4 of its group's last iteration
 * (rings of one group): the default of an undivided handle on the three-launch iteration (from 20 Mi rows), where every K4
 * is then the light launch of the SpMV form; EC3D_XASYNC=0 keeps the K4 that applies the group itself. */
int ec3d_get_x_groups(ec3d_handle h, int32_t *second_stream, int32_t *groups_launched);
/* 1: K4 runs as an SpMV kernel that computes AS = A*S again from the S it reads anyway (k4s_x_r_spmv) and K2-in-K3 no
 * longer writes AS -- 16 B per row and iteration less for 13 flops per row; the same spmv code on the same tiles gives the
 * same AS bit for bit.  R.R and R.R0 are then summed in the SpMV kernels' order (ec3d_get_reduction_geometry(h, 0, ...)
 * reports the grid that sums them).  0: the vector-kernel K4 reading the stored AS */
int ec3d_get_k4_form(ec3d_handle h, int32_t *spmv_form);

int ec3d_device_synchronize(ec3d_handle h);

/* How the library writes the one number the reference prints: norm2(R) on the itmax exit (`print*, norm2(R)`,
 * src/solvers.f90:27), in the list-directed format of the toolchain the reference is built with in this image (flang):
 * leading blank, shortest digits, " .5813987794206226" / " 16.27049629976871" / " 9.87654321E-03".  buf >= 40 bytes. */
void ec3d_format_real8(double v, char *buf);
/* List-directed output is compiler specific, and the reference's own Makefile builds with gfortran (src/Makefile:1-28),
 * which writes the same value as one blank and G25.17E3: "  0.58139877942062257     " (and "   12345678901234568.     ").  EC3D_PRINT_STYLE=gfortran makes the
 * library print the itmax line that way (default: flang's, above); this is the formatter.  buf >= 40 bytes. */
void ec3d_format_real8_gfortran(double v, char *buf);

/* ---- Time-harmonic A-V solve (opt-in) ------------------------------------------------------
 * One complex solve (K + j omega M) x^ = b^ per frequency gives the periodic steady state that the time loop reaches
 * after its start-up transient; convention x(t) = Re(x^ e^{j omega t}).  The operator lives on the class bytes of the
 * structured A-V form: re[cls][slot] is the table of ec3d_assemble with every dt term left out (conductor velocity
 * terms stay), m[cls][slot] the unit imaginary table -- C = mu0 sigma on the diagonal of a conducting A row,
 * 0.5 (+-1 / delta_d) or +-2 / delta_d in the A_d slots of a U row -- and im = omega * m, one rounding per entry; the
 * transient table is re + im * 2 / (omega dt) in A rows and re + im / (omega dt) in U rows.  Both tables are made by
 * every ec3d_assemble; the eight complex work vectors (X^, B^, R, R0, P, AP, S, AS: n_pad interleaved (re, im) pairs each,
 * plus one of staging) by ec3d_harmonic_setup only.  Nothing of the real solve -- its vectors, kernels, defaults, bits --
 * is touched before ec3d_harmonic_load.
 * Arithmetic (no contraction, no float atomics; tests/harmonic_numpy.py restates it bit for bit): a product a x is
 * (ar xr - ai xi, ar xi + ai xr), every product and sum rounded on its own; a row adds its terms from +0.0 in ascending
 * column and skips a term whose two coefficients are 0; <a, b> = sum conj(a) b with the row term (ar br + ai bi,
 * ar bi - ai br), each part a fixed-order sum; a / b = ((ar br + ai bi) / d, (ai br - ar bi) / d), d = br br + bi bi.
 * The iteration is src/solvers.f90:3-50 in this arithmetic: the ||b^|| = 0 return, the ||S|| and ||R|| exits, itmax + 1
 * iterations at most, the restart R0 = R, P = R when |rr0_new| / ||b^|| < tol.
 * Refusals: 3 without an A-V system of ec3d_assemble, 5 on a z-slab or a slab of ec3d_multi, EC3D_NULL_E_MATRIX on a
 * bands + tail or CSR handle, 2 for a negative or non-finite omega, a NULL argument, or a call before
 * ec3d_harmonic_setup.  Host vectors are in the reference numbering, length n. */
typedef struct {
    int32_t ready;      /* ec3d_harmonic_setup ran on this matrix                                   */
    int32_t iter;       /* of the last ec3d_harmonic_solve (itmax + 1: no exit)                     */
    int32_t restarts;   /* times R0 = R, P = R fired in it                                          */
    int32_t stop_kind;  /* 1: the ||S|| exit, 2: the ||R|| exit, 0: none, or ||b^|| = 0             */
    double omega;
    double relres;      /* ||R|| / ||b^|| of the recurrence at the exit (||S|| / ||b^|| at an ||S|| exit) */
    double ms;          /* wall time of the last solve                                              */
    int64_t device_bytes; /* what ec3d_harmonic_setup allocated                                     */
} ec3d_harmonic_info;
int ec3d_harmonic_setup(ec3d_handle h, double omega);
/* which: EC3D_VEC_X or EC3D_VEC_B; im == NULL on upload: a real phasor */
int ec3d_harmonic_upload(ec3d_handle h, int which, const double *re, const double *im);
int ec3d_harmonic_download(ec3d_handle h, int which, double *re, double *im);
/* y = (K + j omega M) x.  Uses P and AP of the complex vectors as scratch; xre == NULL: x is the resident X^ */
int ec3d_harmonic_spmv(ec3d_handle h, const double *xre, const double *xim, double *yre, double *yim);
/* from the resident X^; *iter as ec3d_solve reports it, *relres as in ec3d_harmonic_info (either may be NULL) */
int ec3d_harmonic_solve(ec3d_handle h, double tol, int32_t itmax, int32_t *iter, double *relres);
/* ||b^ - A x^|| / ||b^|| of the resident vectors (the absolute norm when ||b^|| = 0); overwrites R, R0, P.  Always the
 * unprojected residual: with ec3d_harmonic_set_null_projection on it shows the floor |q^H b^| / ||b^|| that the solve
 * left in place, not what the solve converged to (ec3d_harmonic_projected_residual) */
int ec3d_harmonic_true_residual(ec3d_handle h, double *rel, double *bnorm);
/* part 0: Re, 1: Im of the phasor into the handle's REAL X and B, after which every observable of the resident
 * fields (ec3d_vtk_fields, probes, ec3d_domain_integrals, ec3d_field_energy, ec3d_domain_linkage) returns that part's:
 * X = the part of x^; B = the part of j omega C A^ on the A rows of conductor cells (-omega C Im A^ / omega C Re A^,
 * omega C being the im table's diagonal entry), the part of b^ elsewhere; both zeroed on the cel_bndX/Y/Z lists as
 * ec3d_post_update zeroes them.  x^ and b^ stay resident. */
int ec3d_harmonic_load(ec3d_handle h, int32_t part);
int ec3d_get_harmonic(ec3d_handle h, ec3d_harmonic_info *out); /* (a function cannot share the struct's name in C) */
/* tests and device-side callers: complex vector `which` (EC3D_VEC_X ... EC3D_VEC_AS) as the kernels hold it, *pairs =
 * n_pad interleaved (re, im) pairs in device numbering */
int ec3d_harmonic_device_vector(ec3d_handle h, int which, double **device_ptr, int64_t *pairs);
/* Left null vectors of K + j omega M taken out of every harmonic solve's initial residual (opt-in; DESIGN.md section
 * 18a).  The complex operator is singular for the reason the transient one is (section 16): a constant U on a connected
 * conducting component is a right null vector, so there is a left null vector w per component, every residual keeps
 * w^H r = w^H b^, and no iterate gets below |w^H b^| / ||w||.  w is complex, so the Q of ec3d_set_null_projection does
 * not serve.  With the setting on, the first ec3d_harmonic_solve on a matrix and omega (or
 * ec3d_harmonic_left_null_vector) takes the components and seed rows m as section 16 does, forms c = A^H (-e_m) by one
 * launch, solves A^H y = c from y = 0 with the complex iteration above around y = A^H x (k_h_spmv_h: row j adds the
 * entries of column j from +0.0 in ascending source row, a term conj(a) x = (ar xr + ai xi, ar xi - ai xr), zero
 * coefficients skipped) to null_tol within 20 n^(1/3) + 2000 iterations, in the work vectors R ... AS, and sets
 * w = y + e_m.  The w are orthonormalised by classical Gram-Schmidt in component order -- c_i = <Q_i, w> with the
 * conjugate on Q_i, all taken first, then subtracted in order; each part divided by sqrt(sum(re^2 + im^2)) -- and one
 * that keeps less than EC3D_NULL_MIN_KEEP of its norm is dropped and counted.  Every solve then replaces R = b^ - A x^
 * by R - sum c_i Q_i, c_i = <Q_i, R>, before R0, P and ||R||^2 are taken; b^, ||b^||, the exits, the restart rule and
 * the iteration's kernels are untouched, and X^ and B^ keep their bytes through the set-up.  A w that did not reach
 * null_tol is never used: the call returns EC3D_NULL_E_SETUP with component and seed row in the error text.  Not
 * reached means no exit within the cap, or an exit of the recurrence that the adjoint system's true residual
 * ||A^H w|| > 2 null_tol ||A^H e_m|| does not bear out (a recurrence residual keeps falling long after the true one has
 * stopped near 1e-14).  Q belongs
 * to the matrix and to omega: a new matrix or ec3d_harmonic_setup with another omega clears it, the same omega keeps
 * it; the setting belongs to the handle.  on = 0 (default): a solve launches and allocates nothing more and returns the
 * same bits as before.  null_tol <= 0: the default 1e-10.  There is no preconditioner for the adjoint solves.
 * Refusals as the other harmonic entry points (3, 5, EC3D_NULL_E_MATRIX, 2 before ec3d_harmonic_setup); a refusal
 * leaves the setting as it was.
 * ec3d_get_harmonic_null: ec3d_null_info as ec3d_get_null_projection fills it (residual = ||A^H w|| / ||w||, removed =
 * sqrt(sum |c_i|^2) / ||b^|| of the last projected solve or projected residual); while Q exists, device_bytes of
 * ec3d_get_harmonic counts it.  ec3d_harmonic_left_null_vector: kept vector `index`, n doubles per part in the
 * reference numbering; builds Q when the setting is on and there is none; an index outside [0, kept) 2.
 * ec3d_harmonic_spmv_h: y = A^H x, P and AP as scratch.  ec3d_harmonic_projected_residual: ||P (b^ - A x^)|| / ||b^||
 * with the handle's Q (2 with the setting off); overwrites R, R0, P; removed may be NULL.
 * ec3d_harmonic_null_restarts: the restart counts of the adjoint solves, EC3D_NULL_MAX_REPORT entries (tests:
 * ec3d_null_info has no field for them). */
int ec3d_harmonic_set_null_projection(ec3d_handle h, int32_t on, double null_tol);
int ec3d_get_harmonic_null(ec3d_handle h, ec3d_null_info *info);
int ec3d_harmonic_left_null_vector(ec3d_handle h, int32_t index, double *re, double *im);
int ec3d_harmonic_spmv_h(ec3d_handle h, const double *xre, const double *xim, double *yre, double *yim);
int ec3d_harmonic_projected_residual(ec3d_handle h, double *rel, double *removed);
int ec3d_harmonic_null_restarts(ec3d_handle h, int32_t *restarts);
/* A batch of harmonic systems solved in lock step (opt-in): nsys systems (omega_s, b^_s, x^_s),
 * 1 <= nsys <= EC3D_HARMONIC_MAX_BATCH, on the handle's one matrix -- a frequency sweep, one frequency with several
 * right-hand sides (equal omega in several systems is allowed), or any mixture.  The systems ride in the launches of
 * ONE iteration, on a grid of (workgroups, nsys): a workgroup takes its system's state, partial sums, table and vectors
 * and runs the body of the single solve's kernel, so every system gets the bits of its own ec3d_harmonic_solve -- x^,
 * iter, restarts, stop_kind, relres -- whatever the others do.  A system that has taken an exit launches workgroups that
 * return at their first load; the batch ends when every system has stopped or itmax + 1 iterations are launched; the
 * host copies all the states back once per 16 iterations.  One tol and one itmax serve the batch.
 * Storage of its own, made by ec3d_harmonic_batch_setup only and freed by nsys = 0, a new matrix or ec3d_destroy: per
 * system the eight complex vectors (zeroed), the (re, omega_s m) table -- built as ec3d_harmonic_setup builds its one --,
 * the partial sums and the state; plus one staging vector.  ec3d_harmonic_setup is not needed and leaves the batch
 * alone; the batch touches nothing of the single solve.
 * ec3d_harmonic_batch_upload / _download: which = EC3D_VEC_X or EC3D_VEC_B of system sys, as ec3d_harmonic_upload.
 * ec3d_harmonic_batch_solve: from the resident x^_s; iter: nsys entries or NULL.  ec3d_get_harmonic_batch: the info of
 * system sys as ec3d_get_harmonic fills it for a single solve; ms and device_bytes are the whole batch's.
 * ec3d_harmonic_batch_select: ec3d_harmonic_setup(h, omega_s), then device copies of x^_s and b^_s into the resident
 * single X^ and B^: every observable of the single solve (ec3d_harmonic_true_residual, ec3d_harmonic_load and what
 * follows it, a further ec3d_harmonic_solve, with the null projection if wanted) then works on system sys.  The batch
 * keeps its vectors.  ec3d_harmonic_batch_device_vector: vector `which` (EC3D_VEC_X ... EC3D_VEC_AS) of system sys, as
 * ec3d_harmonic_device_vector.
 * Refusals: 3, 5 and EC3D_NULL_E_MATRIX as ec3d_harmonic_setup; 2 for nsys outside [0, EC3D_HARMONIC_MAX_BATCH], a NULL,
 * negative or non-finite omega, a sys outside the batch, any call before a batch set-up, and ec3d_harmonic_batch_solve
 * while ec3d_harmonic_set_null_projection is on (Q belongs to ONE omega: the setting is refused, never ignored).  A
 * refusal leaves the batch as it was; a failed allocation frees the whole batch and returns the HIP status. */
#define EC3D_HARMONIC_MAX_BATCH 16
int ec3d_harmonic_batch_setup(ec3d_handle h, int32_t nsys, const double *omega);
int ec3d_harmonic_batch_upload(ec3d_handle h, int32_t sys, int which, const double *re, const double *im);
int ec3d_harmonic_batch_download(ec3d_handle h, int32_t sys, int which, double *re, double *im);
int ec3d_harmonic_batch_solve(ec3d_handle h, double tol, int32_t itmax, int32_t *iter);
int ec3d_get_harmonic_batch(ec3d_handle h, int32_t sys, ec3d_harmonic_info *out);
int ec3d_harmonic_batch_select(ec3d_handle h, int32_t sys);
int ec3d_harmonic_batch_device_vector(ec3d_handle h, int32_t sys, int which, double **device_ptr, int64_t *pairs);
/* The left null vectors inside a batch (opt-in): every system s gets the Q_s of its own omega_s
 * and is solved as ec3d_harmonic_solve solves it with ec3d_harmonic_set_null_projection on -- x^_s, iter, restarts,
 * stop_kind, relres and removed bit for bit.  A setting of the batch, separate from the single solve's (while THAT one is
 * on, ec3d_harmonic_batch_solve is refused as before).  With it on, the first ec3d_harmonic_batch_solve of a batch (or
 * ec3d_harmonic_batch_left_null_vector, ec3d_harmonic_batch_projected_residual) builds the vectors: per conducting
 * component, the adjoint solves of the DISTINCT omegas of the batch run in lock step -- in the work vectors, partials
 * and states of the first systems, the unknown in a staging vector per omega; x^_s and b^_s keep their bytes -- and
 * every step of the single set-up (seed rows, c = A^H (-e_m), the cap, w = y + e_m, the 2 null_tol check of the true
 * residual, classical Gram-Schmidt, EC3D_NULL_MIN_KEEP) follows per omega, so the number of vectors kept is per omega.
 * Systems with bit-equal omega share one set of vectors.  Every solve then takes Q_s out of system s's initial residual
 * between the batch's begin launch and its set-up launch.  A set-up that misses null_tol returns EC3D_NULL_E_SETUP with
 * system, component and seed row in the error text, and no vector is kept.  null_tol <= 0: the default 1e-10.  Another
 * null_tol, a new ec3d_harmonic_batch_setup, nsys = 0, a new matrix or ec3d_destroy frees the vectors; the setting
 * stays with the handle.  on = 0 (default): nothing more is allocated or launched.
 * ec3d_get_harmonic_batch_null: ec3d_null_info as ec3d_get_harmonic_null fills it, for system sys (setup_ms: the whole
 * set-up's; removed: of system sys's last projection); *shares_with (may be NULL): the lowest system with the same omega.
 * ec3d_harmonic_batch_left_null_vector: kept vector `index` of system sys.  ec3d_harmonic_batch_null_restarts: the
 * restart counts of system sys's adjoint solves, EC3D_NULL_MAX_REPORT entries.  ec3d_harmonic_batch_projected_residual:
 * per system ||P_s (b^_s - A_s x^_s)|| / ||b^_s|| and removed (nsys entries each; removed may be NULL); overwrites R,
 * R0, P of every system; 2 with the setting off.  While the vectors exist, device_bytes of ec3d_get_harmonic_batch
 * counts them.
 * ec3d_harmonic_batch_projected_residual runs a projection of its own: behind it `removed` of
 * ec3d_get_harmonic_batch_null is that projection's figure, no longer the last solve's.
 * Refusals: 3, 5 and EC3D_NULL_E_MATRIX as the other batch entry points -- switching off included --; 2 before a batch
 * set-up (only switching OFF needs no batch), for a sys or an index outside, or a NULL. */
int ec3d_harmonic_batch_set_null_projection(ec3d_handle h, int32_t on, double null_tol);
int ec3d_get_harmonic_batch_null(ec3d_handle h, int32_t sys, ec3d_null_info *info, int32_t *shares_with);
int ec3d_harmonic_batch_left_null_vector(ec3d_handle h, int32_t sys, int32_t index, double *re, double *im);
int ec3d_harmonic_batch_null_restarts(ec3d_handle h, int32_t sys, int32_t *restarts);
int ec3d_harmonic_batch_projected_residual(ec3d_handle h, double *rel, double *removed);

#ifdef __cplusplus
}
#endif
#endif
