! ec3d_hip_mod.f90 -- iso_c_binding interface of libec3d_hip.so for a Fortran host (EC3D).
!
! The reference host keeps geometry ingest, coil motion, RHS build and VTK output
! (src/EC3D.f90:86, :157-404, :436-444); matrix assembly (gen_sparse_matrix, :465-1049) and the
! BiCGSTAB-with-restart loop (src/solvers.f90:3-63) run on the MI355X behind these bindings.
! Arrays are passed exactly as the reference holds them (column-major, i fastest):
!   geoPHYS(sdx,sdy,sdz) INTEGER(1), geoPHYS_C(sdx,sdy,sdz) INTEGER, valPHYS(nsub_glob,5) REAL(8),
!   BND(3,2) REAL(8), delta(3) REAL(8)        (src/m_vxc2data.f90:43-52, src/EC3D.f90:60-77)
! Every function returns 0 on success; ec3d_error_text() gives the message otherwise.
module ec3d_hip
    use iso_c_binding
    implicit none
    private
    public :: ec3d_create, ec3d_destroy, ec3d_assemble, ec3d_assemble_poisson, ec3d_set_matrix_csr, &
              ec3d_solve, ec3d_spmv, ec3d_get_cel_bnd, ec3d_error_text, ec3d_set_format, ec3d_set_structured, &
              ec3d_upload, ec3d_download, ec3d_solve_resident, ec3d_rhs_step, ec3d_post_update, &
              ec3d_vtk_fields, EC3D_VEC_X, EC3D_VEC_B, ec3d_true_residual, &
              ec3d_multi_create, ec3d_multi_destroy, ec3d_multi_assemble, ec3d_multi_set_matrix_csr, &
              ec3d_multi_solve, ec3d_multi_upload, ec3d_multi_download, ec3d_multi_solve_resident, &
              ec3d_multi_rhs_step, ec3d_multi_post_update, ec3d_multi_vtk_fields, ec3d_multi_true_residual, &
              ec3d_multi_vtk_fields_begin, ec3d_multi_vtk_fields_wait, ec3d_rccl_unique_id, ec3d_multi_create_rank, &
              ec3d_multi_plan, ec3d_set_preconditioner, ec3d_get_preconditioner, ec3d_precond_apply, &
              EC3D_PRECOND_NONE, EC3D_PRECOND_MG, EC3D_PRECOND_BLOCK_MG, &
              ec3d_set_u_rhs, EC3D_U_RHS_REFERENCE, EC3D_U_RHS_ALL, &
              ec3d_set_precond_precision, ec3d_get_precond_precision, EC3D_PRECOND_FP64, EC3D_PRECOND_FP32, &
              ec3d_set_precond_coarsening, ec3d_get_precond_coarsening, EC3D_COARSEN_REDISCRETIZE, EC3D_COARSEN_AGGREGATE, &
              ec3d_set_precond_grid, ec3d_get_precond_grid, ec3d_domain_integral, ec3d_domain_integrals, &
              ec3d_field_energy_info, ec3d_field_energy, ec3d_domain_link, ec3d_domain_linkage, &
              ec3d_set_guess_history, ec3d_get_guess_history, ec3d_guess_info, EC3D_GUESS_MAX_DEPTH, &
              ec3d_spmv_t, ec3d_set_null_projection, ec3d_get_null_projection, ec3d_left_null_vector, ec3d_null_info, &
              EC3D_NULL_MAX_REPORT, EC3D_NULL_E_MATRIX, EC3D_NULL_E_SETUP, &
              ec3d_set_probes, ec3d_probe_sample, ec3d_probe_record, ec3d_probe_read, ec3d_probe_reset, ec3d_get_probes, &
              ec3d_probe_info, EC3D_PROBE_NCOMP, EC3D_PROBE_E_FULL, &
              ec3d_harmonic_setup, ec3d_harmonic_upload, ec3d_harmonic_download, ec3d_harmonic_spmv, ec3d_harmonic_solve, &
              ec3d_harmonic_true_residual, ec3d_harmonic_load, ec3d_get_harmonic, ec3d_harmonic_info, &
              ec3d_harmonic_set_null_projection, ec3d_get_harmonic_null, ec3d_harmonic_left_null_vector, &
              ec3d_harmonic_spmv_h, ec3d_harmonic_projected_residual, ec3d_harmonic_null_restarts, &
              EC3D_HARMONIC_MAX_BATCH, ec3d_harmonic_batch_setup, ec3d_harmonic_batch_upload, &
              ec3d_harmonic_batch_download, ec3d_harmonic_batch_solve, ec3d_get_harmonic_batch, &
              ec3d_harmonic_batch_select, ec3d_harmonic_batch_device_vector, &
              ec3d_harmonic_batch_set_null_projection, ec3d_get_harmonic_batch_null, &
              ec3d_harmonic_batch_left_null_vector, ec3d_harmonic_batch_null_restarts, &
              ec3d_harmonic_batch_projected_residual

    integer(c_int), parameter :: EC3D_VEC_X = 0, EC3D_VEC_B = 1   ! Uaf, Jaf
    integer(c_int), parameter :: EC3D_PRECOND_NONE = 0, EC3D_PRECOND_MG = 1   ! ec3d_set_preconditioner
    integer(c_int), parameter :: EC3D_PRECOND_BLOCK_MG = 2   ! ... of the structured A-V form (ec3d_assemble)
    integer(c_int), parameter :: EC3D_U_RHS_REFERENCE = 0, EC3D_U_RHS_ALL = 1   ! ec3d_set_u_rhs
    integer(c_int32_t), parameter :: EC3D_PRECOND_FP64 = 0, EC3D_PRECOND_FP32 = 1   ! ec3d_set_precond_precision
    integer(c_int32_t), parameter :: EC3D_COARSEN_REDISCRETIZE = 0, EC3D_COARSEN_AGGREGATE = 1   ! ec3d_set_precond_coarsening

    integer(c_int32_t), parameter :: EC3D_GUESS_MAX_DEPTH = 8   ! ec3d_set_guess_history

    ! what ec3d_get_guess_history reports of the last solve (ec3d_guess_info of include/ec3d_hip.h)
    type, bind(C) :: ec3d_guess_info
        integer(c_int32_t) :: depth, stored, used, kept
        real(c_double) :: res_before, res_after, coef(EC3D_GUESS_MAX_DEPTH)
    end type

    integer(c_int32_t), parameter :: EC3D_NULL_MAX_REPORT = 32   ! ec3d_get_null_projection
    integer(c_int), parameter :: EC3D_NULL_E_MATRIX = 22, EC3D_NULL_E_SETUP = 23   ! ec3d_set_null_projection, a solve's set-up

    ! what ec3d_get_null_projection reports (ec3d_null_info of include/ec3d_hip.h)
    type, bind(C) :: ec3d_null_info
        integer(c_int32_t) :: on, built, found, kept, dropped, reported
        real(c_double) :: null_tol, removed, setup_ms
        integer(c_int64_t) :: seed_row(EC3D_NULL_MAX_REPORT)
        integer(c_int32_t) :: iterations(EC3D_NULL_MAX_REPORT), was_kept(EC3D_NULL_MAX_REPORT)
        real(c_double) :: residual(EC3D_NULL_MAX_REPORT)
    end type

    ! one record of ec3d_domain_integrals (ec3d_domain_integral of include/ec3d_hip.h)
    type, bind(C) :: ec3d_domain_integral
        integer(c_int32_t) :: domain, pad
        integer(c_int64_t) :: cells
        real(c_double) :: sigma, joule_w, force_n(3)
    end type

    ! what ec3d_field_energy returns (ec3d_field_energy_info of include/ec3d_hip.h)
    type, bind(C) :: ec3d_field_energy_info
        integer(c_int64_t) :: cells
        real(c_double) :: energy_b, energy_axis(3), aj_source, aj_eddy
    end type

    ! one record of ec3d_domain_linkage (ec3d_domain_link of include/ec3d_hip.h)
    type, bind(C) :: ec3d_domain_link
        integer(c_int32_t) :: domain, pad
        integer(c_int64_t) :: cells
        real(c_double) :: linkage, jsum(3)
    end type

    integer(c_int32_t), parameter :: EC3D_PROBE_NCOMP = 13   ! values per probe: a(3), eddy(3), source(3), b(3), u
    integer(c_int), parameter :: EC3D_PROBE_E_FULL = 24      ! ec3d_probe_record on a full buffer
    integer(c_int), parameter :: EC3D_HARMONIC_MAX_BATCH = 16   ! systems of one ec3d_harmonic_batch_setup

    ! what ec3d_get_probes reports (ec3d_probe_info of include/ec3d_hip.h)
    type, bind(C) :: ec3d_probe_info
        integer(c_int64_t) :: nprobes, capacity, recorded, device_bytes
    end type

    ! what ec3d_get_harmonic reports (ec3d_harmonic_info of include/ec3d_hip.h)
    type, bind(C) :: ec3d_harmonic_info
        integer(c_int32_t) :: ready, iter, restarts, stop_kind
        real(c_double) :: omega, relres, ms
        integer(c_int64_t) :: device_bytes
    end type

    interface
        integer(c_int) function ec3d_create(h, device) bind(C, name="ec3d_create")
            import :: c_ptr, c_int
            type(c_ptr), intent(out) :: h
            integer(c_int), value :: device
        end function
        integer(c_int) function ec3d_destroy(h) bind(C, name="ec3d_destroy")
            import :: c_ptr, c_int
            type(c_ptr), value :: h
        end function
        integer(c_int) function ec3d_set_format(h, dictionary) bind(C, name="ec3d_set_format")
            import :: c_ptr, c_int
            type(c_ptr), value :: h
            integer(c_int), value :: dictionary
        end function
        ! 0: keep the A-V matrix as bands + tail instead of the structured form (DESIGN.md section 2)
        integer(c_int) function ec3d_set_structured(h, on) bind(C, name="ec3d_set_structured")
            import :: c_ptr, c_int
            type(c_ptr), value :: h
            integer(c_int), value :: on
        end function
        ! replaces CALL gen_sparse_matrix (src/EC3D.f90:115)
        integer(c_int) function ec3d_assemble(h, sdx, sdy, sdz, geoPHYS, geoPHYS_C, valPHYS, nsub_glob, &
                                              BND, delta, dt) bind(C, name="ec3d_assemble")
            import :: c_ptr, c_int, c_int8_t, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sdx, sdy, sdz, nsub_glob
            integer(c_int8_t), intent(in) :: geoPHYS(*)
            integer(c_int32_t), intent(in) :: geoPHYS_C(*)
            real(c_double), intent(in) :: valPHYS(*), BND(*), delta(*)
            real(c_double), value :: dt
        end function
        integer(c_int) function ec3d_assemble_poisson(h, sdx, sdy, sdz, BND, delta) &
                bind(C, name="ec3d_assemble_poisson")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sdx, sdy, sdz
            real(c_double), intent(in) :: BND(*), delta(*)
        end function
        integer(c_int) function ec3d_set_matrix_csr(h, n, valA, irow, jcol) bind(C, name="ec3d_set_matrix_csr")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: n
            real(c_double), intent(in) :: valA(*)
            integer(c_int32_t), intent(in) :: irow(*), jcol(*)
        end function
        ! replaces CALL sprsBCGstabwr(valA, irow, jcol, nCellsGlob, Jaf, Uaf, tolerance, itmax, iter)
        ! (src/EC3D.f90:408); resid_hist may be c_null_ptr
        integer(c_int) function ec3d_solve(h, b, x, tolerance, itmax, iter, resid_hist, hist_cap) &
                bind(C, name="ec3d_solve")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: b(*)
            real(c_double), intent(inout) :: x(*)
            real(c_double), value :: tolerance
            integer(c_int32_t), value :: itmax, hist_cap
            integer(c_int32_t), intent(out) :: iter
            type(c_ptr), value :: resid_hist
        end function
        ! fields resident on the device across time steps (which = EC3D_VEC_X / EC3D_VEC_B)
        integer(c_int) function ec3d_upload(h, which, host) bind(C, name="ec3d_upload")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            integer(c_int), value :: which
            real(c_double), intent(in) :: host(*)
        end function
        integer(c_int) function ec3d_download(h, which, host) bind(C, name="ec3d_download")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            integer(c_int), value :: which
            real(c_double), intent(out) :: host(*)
        end function
        integer(c_int) function ec3d_solve_resident(h, tolerance, itmax, iter, resid_hist, hist_cap) &
                bind(C, name="ec3d_solve_resident")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            real(c_double), value :: tolerance
            integer(c_int32_t), value :: itmax, hist_cap
            integer(c_int32_t), intent(out) :: iter
            type(c_ptr), value :: resid_hist
        end function
        ! replaces src/EC3D.f90:275-404: source scatter (1-based unknown ids), inertial terms, U-row RHS,
        ! zero-fills -- on the resident Jaf / Uaf
        integer(c_int) function ec3d_rhs_step(h, moving, nsrc, src_index, src_value) bind(C, name="ec3d_rhs_step")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: moving, nsrc
            integer(c_int32_t), intent(in) :: src_index(*)
            real(c_double), intent(in) :: src_value(*)
        end function
        ! replaces src/EC3D.f90:412-433
        integer(c_int) function ec3d_post_update(h) bind(C, name="ec3d_post_update")
            import :: c_ptr, c_int
            type(c_ptr), value :: h
        end function
        ! the four point vectors of writeVtk_field (src/utilites.f90:222-289), 3*nCells REAL(4) each
        integer(c_int) function ec3d_vtk_fields(h, delta, fA, fEddy, fSource, fB) bind(C, name="ec3d_vtk_fields")
            import :: c_ptr, c_int, c_double, c_float
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            real(c_float), intent(out) :: fA(*), fEddy(*), fSource(*), fB(*)
        end function
        ! Joule loss [W] and Lorentz force [N] per conducting domain from the resident Uaf, Jaf: the integrals of the
        ! fields above before their rounding to REAL(4), ascending domain id; call after ec3d_post_update.  ndomains
        ! receives the count; cap = room in out (cap = 0 and any out: the count only, status 2 when there are domains)
        integer(c_int) function ec3d_domain_integrals(h, delta, cap, ndomains, out) bind(C, name="ec3d_domain_integrals")
            import :: c_ptr, c_int, c_int32_t, c_double, ec3d_domain_integral
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            integer(c_int32_t), value :: cap
            integer(c_int32_t), intent(out) :: ndomains
            type(ec3d_domain_integral), intent(out) :: out(*)
        end function
        ! magnetic energy of the box [J] and the integral of A.J outside / inside the conductors [J] from the resident Uaf,
        ! Jaf, one streaming pass on the device; call after ec3d_post_update
        integer(c_int) function ec3d_field_energy(h, delta, out) bind(C, name="ec3d_field_energy")
            import :: c_ptr, c_int, c_double, ec3d_field_energy_info
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            type(ec3d_field_energy_info), intent(out) :: out
        end function
        ! flux linkage psi*I [J] and the integral of J [A m] of every non-conducting domain (the air among them), ascending
        ! domain id; cap and ndomains as in ec3d_domain_integrals
        integer(c_int) function ec3d_domain_linkage(h, delta, cap, ndomains, out) bind(C, name="ec3d_domain_linkage")
            import :: c_ptr, c_int, c_int32_t, c_double, ec3d_domain_link
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            integer(c_int32_t), value :: cap
            integer(c_int32_t), intent(out) :: ndomains
            type(ec3d_domain_link), intent(out) :: out(*)
        end function
        ! probes: the fields at chosen cells from the resident Uaf, Jaf -- what field_N.vtk shows there before its rounding
        ! to REAL(4), and U.  cells: 0-based cell numbers i + j*sdx + k*sdx*sdy (i, j, k from 0); capacity: records the
        ! device buffer holds (0: ec3d_probe_sample only); nprobes = 0 clears the set
        integer(c_int) function ec3d_set_probes(h, nprobes, cells, capacity) bind(C, name="ec3d_set_probes")
            import :: c_ptr, c_int, c_int64_t
            type(c_ptr), value :: h
            integer(c_int64_t), value :: nprobes, capacity
            integer(c_int64_t), intent(in) :: cells(*)
        end function
        ! out(nprobes, EC3D_PROBE_NCOMP): ax ay az, eddy x y z, source x y z, bx by bz, u; call after ec3d_post_update
        integer(c_int) function ec3d_probe_sample(h, delta, out) bind(C, name="ec3d_probe_sample")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            real(c_double), intent(out) :: out(*)
        end function
        ! the same sample appended to the record on the device, nothing waits; EC3D_PROBE_E_FULL when the buffer is full
        integer(c_int) function ec3d_probe_record(h, delta, T) bind(C, name="ec3d_probe_record")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            real(c_double), value :: T
        end function
        ! records first .. first + count - 1 (from 0): out(nprobes, EC3D_PROBE_NCOMP, count) and T_out(count)
        integer(c_int) function ec3d_probe_read(h, first, count, T_out, out) bind(C, name="ec3d_probe_read")
            import :: c_ptr, c_int, c_int64_t, c_double
            type(c_ptr), value :: h
            integer(c_int64_t), value :: first, count
            real(c_double), intent(out) :: T_out(*), out(*)
        end function
        integer(c_int) function ec3d_probe_reset(h) bind(C, name="ec3d_probe_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: h
        end function
        integer(c_int) function ec3d_get_probes(h, info) bind(C, name="ec3d_get_probes")
            import :: c_ptr, c_int, ec3d_probe_info
            type(c_ptr), value :: h
            type(ec3d_probe_info), intent(out) :: info
        end function
        ! ec3d_vtk_fields beside the next time step: _begin returns at once (field kernel + copy into a pinned buffer are
        ! enqueued), _wait blocks until that buffer has landed and returns C pointers to 3*ncells REAL(4) each
        ! (c_f_pointer them); big_endian /= 0: already in the byte order of the BINARY legacy-VTK file
        integer(c_int) function ec3d_vtk_fields_begin(h, delta, big_endian, slot) bind(C, name="ec3d_vtk_fields_begin")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: delta(*)
            integer(c_int), value :: big_endian
            integer(c_int), intent(out) :: slot
        end function
        integer(c_int) function ec3d_vtk_fields_wait(h, slot, fA, fEddy, fSource, fB, ncells) &
                bind(C, name="ec3d_vtk_fields_wait")
            import :: c_ptr, c_int, c_int64_t
            type(c_ptr), value :: h
            integer(c_int), value :: slot
            type(c_ptr), intent(out) :: fA, fEddy, fSource, fB
            integer(c_int64_t), intent(out) :: ncells
        end function
        integer(c_int) function ec3d_spmv(h, x, y) bind(C, name="ec3d_spmv")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: x(*)
            real(c_double), intent(out) :: y(*)
        end function
        ! multigrid preconditioner of a matrix from ec3d_assemble_poisson (include/ec3d_hip.h); zeros = defaults
        integer(c_int) function ec3d_set_preconditioner(h, kind, pre, post, coarse_sweeps) &
                bind(C, name="ec3d_set_preconditioner")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int), value :: kind
            integer(c_int32_t), value :: pre, post, coarse_sweeps
        end function
        ! dims(3*levels): sdx, sdy, sdz of every level, finest first
        integer(c_int) function ec3d_get_preconditioner(h, kind, levels, dims) bind(C, name="ec3d_get_preconditioner")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int), intent(out) :: kind
            integer(c_int32_t), intent(out) :: levels
            integer(c_int32_t), intent(out) :: dims(*)
        end function
        ! z = M r, one V-cycle (parity probe)
        integer(c_int) function ec3d_precond_apply(h, r, z) bind(C, name="ec3d_precond_apply")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: r(*)
            real(c_double), intent(out) :: z(*)
        end function
        ! precision of the V-cycle the next ec3d_set_preconditioner(EC3D_PRECOND_MG) builds (include/ec3d_hip.h)
        integer(c_int) function ec3d_set_precond_precision(h, precision) bind(C, name="ec3d_set_precond_precision")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: precision
        end function
        ! setting: the handle's; in_use: that of the hierarchy now set (EC3D_PRECOND_FP64 when there is none)
        integer(c_int) function ec3d_get_precond_precision(h, setting, in_use) bind(C, name="ec3d_get_precond_precision")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), intent(out) :: setting, in_use
        end function
        ! coarsening rule of the hierarchy the next ec3d_set_preconditioner(EC3D_PRECOND_MG) builds (include/ec3d_hip.h)
        integer(c_int) function ec3d_set_precond_coarsening(h, rule) bind(C, name="ec3d_set_precond_coarsening")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: rule
        end function
        ! setting: the handle's; in_use: that of the hierarchy now set; level_kinds: c_loc of an integer(c_int32_t)
        ! array with one entry per level of it (0 = the handle's matrix, 1 = rediscretised, 2 = Galerkin), or c_null_ptr
        integer(c_int) function ec3d_get_precond_coarsening(h, setting, in_use, level_kinds) &
                bind(C, name="ec3d_get_precond_coarsening")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), intent(out) :: setting, in_use
            type(c_ptr), value :: level_kinds
        end function
        ! the matrix of ec3d_set_matrix_csr is a 7-point operator on an sdx x sdy x sdz box, r = i + j sdx + k sdx sdy:
        ! EC3D_PRECOND_MG then builds its hierarchy from the matrix alone (include/ec3d_hip.h); cleared by a new matrix
        integer(c_int) function ec3d_set_precond_grid(h, sdx, sdy, sdz) bind(C, name="ec3d_set_precond_grid")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sdx, sdy, sdz
        end function
        ! dims: the grid now set, zeros when none
        integer(c_int) function ec3d_get_precond_grid(h, dims) bind(C, name="ec3d_get_precond_grid")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), intent(out) :: dims(3)
        end function
        ! start every solve from the projection onto up to `depth` earlier solutions of the matrix (0 = off, the default;
        ! include/ec3d_hip.h): 2 for a depth outside 0 .. EC3D_GUESS_MAX_DEPTH, 4 on a z-slab
        integer(c_int) function ec3d_set_guess_history(h, depth) bind(C, name="ec3d_set_guess_history")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: depth
        end function
        ! of the last solve: pairs projected on, the new pair stored / discarded / the history cleared, the residuals
        integer(c_int) function ec3d_get_guess_history(h, info) bind(C, name="ec3d_get_guess_history")
            import :: c_ptr, c_int, ec3d_guess_info
            type(c_ptr), value :: h
            type(ec3d_guess_info), intent(out) :: info
        end function
        ! y = A^T x on the structured A-V form of ec3d_assemble (parity probe; include/ec3d_hip.h)
        integer(c_int) function ec3d_spmv_t(h, x, y) bind(C, name="ec3d_spmv_t")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: x(*)
            real(c_double), intent(out) :: y(*)
        end function
        ! take the left null vectors of the A-V system out of every solve's initial residual (on = 0: off, the default;
        ! null_tol <= 0: 1e-10; include/ec3d_hip.h): EC3D_NULL_E_MATRIX on a Poisson, CSR or bands + tail matrix, 4 on a z-slab
        integer(c_int) function ec3d_set_null_projection(h, on, null_tol) bind(C, name="ec3d_set_null_projection")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: on
            real(c_double), value :: null_tol
        end function
        ! the setting, the components found / kept / dropped, per component seed row, adjoint iterations and residual
        integer(c_int) function ec3d_get_null_projection(h, info) bind(C, name="ec3d_get_null_projection")
            import :: c_ptr, c_int, ec3d_null_info
            type(c_ptr), value :: h
            type(ec3d_null_info), intent(out) :: info
        end function
        ! kept left null vector `index` (0-based; n doubles, the reference's numbering)
        integer(c_int) function ec3d_left_null_vector(h, index, w) bind(C, name="ec3d_left_null_vector")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: index
            real(c_double), intent(out) :: w(*)
        end function
        ! Time-harmonic solve (K + j omega M) x^ = b^ on the A-V system of ec3d_assemble (include/ec3d_hip.h; opt-in):
        ! set-up at omega [rad/s]; host vectors as separate real and imaginary parts, n doubles each, the reference's numbering
        integer(c_int) function ec3d_harmonic_setup(h, omega) bind(C, name="ec3d_harmonic_setup")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), value :: omega
        end function
        ! which: EC3D_VEC_X or EC3D_VEC_B
        integer(c_int) function ec3d_harmonic_upload(h, which, re, im) bind(C, name="ec3d_harmonic_upload")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            integer(c_int), value :: which
            real(c_double), intent(in) :: re(*), im(*)
        end function
        integer(c_int) function ec3d_harmonic_download(h, which, re, im) bind(C, name="ec3d_harmonic_download")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            integer(c_int), value :: which
            real(c_double), intent(out) :: re(*), im(*)
        end function
        integer(c_int) function ec3d_harmonic_spmv(h, xre, xim, yre, yim) bind(C, name="ec3d_harmonic_spmv")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: xre(*), xim(*)
            real(c_double), intent(out) :: yre(*), yim(*)
        end function
        ! complex BiCGSTAB with restart from the resident x^; iter as ec3d_solve reports it
        integer(c_int) function ec3d_harmonic_solve(h, tol, itmax, iter, relres) bind(C, name="ec3d_harmonic_solve")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            real(c_double), value :: tol
            integer(c_int32_t), value :: itmax
            integer(c_int32_t), intent(out) :: iter
            real(c_double), intent(out) :: relres
        end function
        integer(c_int) function ec3d_harmonic_true_residual(h, rel, bnorm) bind(C, name="ec3d_harmonic_true_residual")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(out) :: rel, bnorm
        end function
        ! part 0 / 1: Re / Im of the phasor into the real X and B; the observables of the resident fields then return it
        integer(c_int) function ec3d_harmonic_load(h, part) bind(C, name="ec3d_harmonic_load")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: part
        end function
        integer(c_int) function ec3d_get_harmonic(h, info) bind(C, name="ec3d_get_harmonic")
            import :: c_ptr, c_int, ec3d_harmonic_info
            type(c_ptr), value :: h
            type(ec3d_harmonic_info), intent(out) :: info
        end function
        ! Left null vectors of K + j omega M out of every harmonic solve's initial residual (include/ec3d_hip.h; opt-in):
        ! on = 1 / 0, null_tol <= 0: 1e-10.  The first ec3d_harmonic_solve on a matrix and omega builds them
        integer(c_int) function ec3d_harmonic_set_null_projection(h, on, null_tol) &
                bind(C, name="ec3d_harmonic_set_null_projection")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: on
            real(c_double), value :: null_tol
        end function
        integer(c_int) function ec3d_get_harmonic_null(h, info) bind(C, name="ec3d_get_harmonic_null")
            import :: c_ptr, c_int, ec3d_null_info
            type(c_ptr), value :: h
            type(ec3d_null_info), intent(out) :: info
        end function
        ! kept vector `index` (0-based), n doubles per part, the reference's numbering
        integer(c_int) function ec3d_harmonic_left_null_vector(h, index, re, im) bind(C, name="ec3d_harmonic_left_null_vector")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: index
            real(c_double), intent(out) :: re(*), im(*)
        end function
        ! y = (K + j omega M)^H x
        integer(c_int) function ec3d_harmonic_spmv_h(h, xre, xim, yre, yim) bind(C, name="ec3d_harmonic_spmv_h")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(in) :: xre(*), xim(*)
            real(c_double), intent(out) :: yre(*), yim(*)
        end function
        ! ||P (b^ - A x^)|| / ||b^|| with the handle's vectors; removed = sqrt(sum |c_i|^2) / ||b^||
        integer(c_int) function ec3d_harmonic_projected_residual(h, rel, removed) &
                bind(C, name="ec3d_harmonic_projected_residual")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(out) :: rel, removed
        end function
        ! the adjoint solves' restart counts, EC3D_NULL_MAX_REPORT entries
        integer(c_int) function ec3d_harmonic_null_restarts(h, restarts) bind(C, name="ec3d_harmonic_null_restarts")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), intent(out) :: restarts(*)
        end function
        ! A batch of harmonic systems (omega_s, b^_s, x^_s) solved in lock step on the one matrix (include/ec3d_hip.h;
        ! opt-in): nsys in [1, EC3D_HARMONIC_MAX_BATCH], nsys = 0 frees the batch; sys is 0-based
        integer(c_int) function ec3d_harmonic_batch_setup(h, nsys, omega) bind(C, name="ec3d_harmonic_batch_setup")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: nsys
            real(c_double), intent(in) :: omega(*)
        end function
        integer(c_int) function ec3d_harmonic_batch_upload(h, sys, which, re, im) bind(C, name="ec3d_harmonic_batch_upload")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
            integer(c_int), value :: which
            real(c_double), intent(in) :: re(*), im(*)
        end function
        integer(c_int) function ec3d_harmonic_batch_download(h, sys, which, re, im) &
                bind(C, name="ec3d_harmonic_batch_download")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
            integer(c_int), value :: which
            real(c_double), intent(out) :: re(*), im(*)
        end function
        ! every system from its resident x^; iter: nsys entries
        integer(c_int) function ec3d_harmonic_batch_solve(h, tol, itmax, iter) bind(C, name="ec3d_harmonic_batch_solve")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            real(c_double), value :: tol
            integer(c_int32_t), value :: itmax
            integer(c_int32_t), intent(out) :: iter(*)
        end function
        ! the report of system sys; ms and device_bytes are the whole batch's
        integer(c_int) function ec3d_get_harmonic_batch(h, sys, info) bind(C, name="ec3d_get_harmonic_batch")
            import :: c_ptr, c_int, c_int32_t, ec3d_harmonic_info
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
            type(ec3d_harmonic_info), intent(out) :: info
        end function
        ! ec3d_harmonic_setup(omega_sys), then x^_sys and b^_sys into the resident single X^ and B^
        integer(c_int) function ec3d_harmonic_batch_select(h, sys) bind(C, name="ec3d_harmonic_batch_select")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
        end function
        ! complex vector `which` (EC3D_VEC_X ... 7) of system sys on the device: pairs = n_pad interleaved (re, im) pairs
        integer(c_int) function ec3d_harmonic_batch_device_vector(h, sys, which, device_ptr, pairs) &
                bind(C, name="ec3d_harmonic_batch_device_vector")
            import :: c_ptr, c_int, c_int32_t, c_int64_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
            integer(c_int), value :: which
            type(c_ptr), intent(out) :: device_ptr
            integer(c_int64_t), intent(out) :: pairs
        end function
        ! The left null vectors inside a batch (include/ec3d_hip.h; opt-in): every system projects with the vectors of
        ! its own omega; null_tol <= 0: 1e-10
        integer(c_int) function ec3d_harmonic_batch_set_null_projection(h, on, null_tol) &
                bind(C, name="ec3d_harmonic_batch_set_null_projection")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: on
            real(c_double), value :: null_tol
        end function
        ! the report of system sys; shares_with: the lowest system with the same omega (C callers may pass NULL for it,
        ! a caller of this interface always receives it)
        integer(c_int) function ec3d_get_harmonic_batch_null(h, sys, info, shares_with) &
                bind(C, name="ec3d_get_harmonic_batch_null")
            import :: c_ptr, c_int, c_int32_t, ec3d_null_info
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
            type(ec3d_null_info), intent(out) :: info
            integer(c_int32_t), intent(out) :: shares_with
        end function
        integer(c_int) function ec3d_harmonic_batch_left_null_vector(h, sys, index, re, im) &
                bind(C, name="ec3d_harmonic_batch_left_null_vector")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys, index
            real(c_double), intent(out) :: re(*), im(*)
        end function
        integer(c_int) function ec3d_harmonic_batch_null_restarts(h, sys, restarts) &
                bind(C, name="ec3d_harmonic_batch_null_restarts")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: sys
            integer(c_int32_t), intent(out) :: restarts(*)
        end function
        ! nsys entries each (C callers may pass NULL for removed; this interface always takes the array)
        integer(c_int) function ec3d_harmonic_batch_projected_residual(h, rel, removed) &
                bind(C, name="ec3d_harmonic_batch_projected_residual")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(out) :: rel(*), removed(*)
        end function
        ! U rows ec3d_rhs_step gives their right-hand side with several conducting domains (include/ec3d_hip.h)
        integer(c_int) function ec3d_set_u_rhs(h, rule) bind(C, name="ec3d_set_u_rhs")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int32_t), value :: rule
        end function
        ! cel_bndX/Y/Z, cel_bndUx/y/z (src/EC3D.f90:758-760, :938-940): which = 0..5
        integer(c_int) function ec3d_get_cel_bnd(h, which, count, list) bind(C, name="ec3d_get_cel_bnd")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: h
            integer(c_int), value :: which
            integer(c_int32_t), intent(out) :: count
            type(c_ptr), value :: list
        end function
        ! ||Jaf - A*Uaf|| / ||Jaf|| of the resident vectors, computed on the device
        integer(c_int) function ec3d_true_residual(h, rel, bnorm) bind(C, name="ec3d_true_residual")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h
            real(c_double), intent(out) :: rel, bnorm
        end function
        ! ---- N GPUs behind one handle (include/ec3d_hip.h section 2c): same arguments as the calls above, global
        ! arrays in the reference's numbering; the library cuts z-slabs and keeps one host thread per GPU.
        ! devices: c_null_ptr for GPUs 0 .. nranks-1, or c_loc of an INTEGER(c_int32_t) list.
        integer(c_int) function ec3d_multi_create(mh, nranks, devices) bind(C, name="ec3d_multi_create")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), intent(out) :: mh
            integer(c_int32_t), value :: nranks
            type(c_ptr), value :: devices
        end function
        ! ---- one process per GPU (mpirun / torch.distributed.run style launch): this process holds rank `rank` of
        ! `nranks` on `device`; RCCL carries the halo planes (ncclSend / ncclRecv on a side stream) and the partial sums
        ! (ncclAllGather).  id_halo, id_sum: two 128-byte RCCL unique ids made by ec3d_rccl_unique_id on ONE rank and
        ! handed to all (e.g. MPI_Bcast of a character(len=1) :: id(128) array).  Every other ec3d_multi_* call then takes
        ! the same GLOBAL arrays on every rank.  as_rank = -1, as_world = 0 (a rehearsal of one rank of a larger job
        ! otherwise, see include/ec3d_hip.h).
        integer(c_int) function ec3d_rccl_unique_id(id128) bind(C, name="ec3d_rccl_unique_id")
            import :: c_int, c_char
            character(kind=c_char), intent(out) :: id128(128)
        end function
        integer(c_int) function ec3d_multi_create_rank(mh, rank, nranks, device, id_halo, id_sum, as_rank, as_world) &
                bind(C, name="ec3d_multi_create_rank")
            import :: c_ptr, c_int, c_int32_t, c_char
            type(c_ptr), intent(out) :: mh
            integer(c_int32_t), value :: rank, nranks, device, as_rank, as_world
            character(kind=c_char), intent(in) :: id_halo(128), id_sum(128)
        end function
        ! the schedule the job runs (0 .. 4, include/ec3d_hip.h) and the iterations between two X updates
        integer(c_int) function ec3d_multi_plan(mh, plan, x_every) bind(C, name="ec3d_multi_plan")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: mh
            integer(c_int32_t), intent(out) :: plan, x_every
        end function
        integer(c_int) function ec3d_multi_destroy(mh) bind(C, name="ec3d_multi_destroy")
            import :: c_ptr, c_int
            type(c_ptr), value :: mh
        end function
        integer(c_int) function ec3d_multi_assemble(mh, sdx, sdy, sdz, geoPHYS, geoPHYS_C, valPHYS, nsub_glob, &
                                                    BND, delta, dt) bind(C, name="ec3d_multi_assemble")
            import :: c_ptr, c_int, c_int8_t, c_int32_t, c_double
            type(c_ptr), value :: mh
            integer(c_int32_t), value :: sdx, sdy, sdz, nsub_glob
            integer(c_int8_t), intent(in) :: geoPHYS(*)
            integer(c_int32_t), intent(in) :: geoPHYS_C(*)
            real(c_double), intent(in) :: valPHYS(*), BND(*), delta(*)
            real(c_double), value :: dt
        end function
        integer(c_int) function ec3d_multi_set_matrix_csr(mh, n, valA, irow, jcol) &
                bind(C, name="ec3d_multi_set_matrix_csr")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: mh
            integer(c_int32_t), value :: n
            real(c_double), intent(in) :: valA(*)
            integer(c_int32_t), intent(in) :: irow(*), jcol(*)
        end function
        ! replaces CALL sprsBCGstabwr(valA, irow, jcol, n, Jaf, Uaf, tolerance, itmax, iter)   (src/EC3D.f90:408)
        integer(c_int) function ec3d_multi_solve(mh, b, x, tolerance, itmax, iter) bind(C, name="ec3d_multi_solve")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: mh
            real(c_double), intent(in) :: b(*)
            real(c_double), intent(inout) :: x(*)
            real(c_double), value :: tolerance
            integer(c_int32_t), value :: itmax
            integer(c_int32_t), intent(out) :: iter
        end function
        integer(c_int) function ec3d_multi_upload(mh, which, host) bind(C, name="ec3d_multi_upload")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: mh
            integer(c_int), value :: which
            real(c_double), intent(in) :: host(*)
        end function
        integer(c_int) function ec3d_multi_download(mh, which, host) bind(C, name="ec3d_multi_download")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: mh
            integer(c_int), value :: which
            real(c_double), intent(out) :: host(*)
        end function
        integer(c_int) function ec3d_multi_solve_resident(mh, tolerance, itmax, iter) &
                bind(C, name="ec3d_multi_solve_resident")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: mh
            real(c_double), value :: tolerance
            integer(c_int32_t), value :: itmax
            integer(c_int32_t), intent(out) :: iter
        end function
        integer(c_int) function ec3d_multi_rhs_step(mh, moving, nsrc, src_index, src_value) &
                bind(C, name="ec3d_multi_rhs_step")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: mh
            integer(c_int32_t), value :: moving, nsrc
            integer(c_int32_t), intent(in) :: src_index(*)
            real(c_double), intent(in) :: src_value(*)
        end function
        integer(c_int) function ec3d_multi_post_update(mh) bind(C, name="ec3d_multi_post_update")
            import :: c_ptr, c_int
            type(c_ptr), value :: mh
        end function
        integer(c_int) function ec3d_multi_vtk_fields(mh, delta, fA, fEddy, fSource, fB) &
                bind(C, name="ec3d_multi_vtk_fields")
            import :: c_ptr, c_int, c_double, c_float
            type(c_ptr), value :: mh
            real(c_double), intent(in) :: delta(*)
            real(c_float), intent(out) :: fA(*), fEddy(*), fSource(*), fB(*)   ! 3*nCells each, the WHOLE grid
        end function
        ! the overlapped output over the slabs: _begin on all of them, _wait per slab (rank = 0 .. nranks-1): that
        ! slab's cells cell0 .. cell0+ncells-1 of every vector; fEddy = c_null_ptr for a slab without conductor
        integer(c_int) function ec3d_multi_vtk_fields_begin(mh, delta, big_endian, slot) &
                bind(C, name="ec3d_multi_vtk_fields_begin")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: mh
            real(c_double), intent(in) :: delta(*)
            integer(c_int), value :: big_endian
            integer(c_int), intent(out) :: slot
        end function
        integer(c_int) function ec3d_multi_vtk_fields_wait(mh, slot, rank, fA, fEddy, fSource, fB, cell0, ncells) &
                bind(C, name="ec3d_multi_vtk_fields_wait")
            import :: c_ptr, c_int, c_int64_t
            type(c_ptr), value :: mh
            integer(c_int), value :: slot, rank
            type(c_ptr), intent(out) :: fA, fEddy, fSource, fB
            integer(c_int64_t), intent(out) :: cell0, ncells
        end function
        integer(c_int) function ec3d_multi_true_residual(mh, rel, bnorm) bind(C, name="ec3d_multi_true_residual")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: mh
            real(c_double), intent(out) :: rel, bnorm
        end function
        function ec3d_last_error_c() bind(C, name="ec3d_last_error") result(p)
            import :: c_ptr
            type(c_ptr) :: p
        end function
    end interface

contains

    function ec3d_error_text() result(txt)
        character(len=:), allocatable :: txt
        character(kind=c_char), pointer :: s(:)
        type(c_ptr) :: p
        integer :: n
        p = ec3d_last_error_c()
        txt = ''
        if (.not. c_associated(p)) return
        call c_f_pointer(p, s, [4096])
        n = 0
        do while (n < 4096)
            if (s(n + 1) == c_null_char) exit
            n = n + 1
        end do
        allocate (character(len=n) :: txt)
        txt = transfer(s(1:n), txt)
    end function

end module ec3d_hip
