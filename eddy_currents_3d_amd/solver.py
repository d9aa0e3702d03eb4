"""ctypes host over the C ABI of libec3d_hip.so (include/ec3d_hip.h).

Mirrors the reference's interface for the hot path:

* :func:`sprsBCGstabWR` — same name, argument order and meaning as
  ``SUBROUTINE sprsBCGstabWR (valA, irow, jcol, n, b, x, tolerance, itmax, iter)``
  (/root/reference/src/solvers.f90:3): 1-based CSR, ``x`` is updated in place (warm start),
  ``iter`` is returned.
* :class:`EC3DSolver` — the native handle API (assembly on the device, resident vectors,
  residual history, timing hooks).

No fallback: if the shared library or a HIP device is missing this raises :class:`EC3DError`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.environ.get("EC3D_LIB") or os.path.join(PKG, "libec3d_hip.so")   # EC3D_LIB: another build (A/B timing)


class EC3DError(RuntimeError):
    pass


class Geom(C.Structure):
    _fields_ = [("n_pad", C.c_int32), ("tile", C.c_int32), ("nblk", C.c_int32),
                ("threads", C.c_int32), ("xcd_group", C.c_int32), ("zm_tpp", C.c_int32),
                ("zm_pps", C.c_int32), ("ntiles_front", C.c_int32), ("ulist_n", C.c_int32),
                ("patch_x", C.c_int32), ("patch_y", C.c_int32), ("patch_sdx", C.c_int32),
                ("patch_pitch", C.c_int32), ("patch_sdy", C.c_int32)]


class MatrixInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_pad", C.c_int64), ("nnz", C.c_int64), ("nbands", C.c_int32),
                ("band_offset", C.c_int32 * 16), ("tail_rows", C.c_int64),
                ("tail_entries_padded", C.c_int64), ("device_bytes", C.c_int64),
                ("dict_classes", C.c_int32)]


class DomainIntegral(C.Structure):
    """ec3d_domain_integral of include/ec3d_hip.h."""
    _fields_ = [("domain", C.c_int32), ("pad", C.c_int32), ("cells", C.c_int64), ("sigma", C.c_double),
                ("joule_w", C.c_double), ("force_n", C.c_double * 3)]


class FieldEnergy(C.Structure):
    """ec3d_field_energy_info of include/ec3d_hip.h."""
    _fields_ = [("cells", C.c_int64), ("energy_b", C.c_double), ("energy_axis", C.c_double * 3),
                ("aj_source", C.c_double), ("aj_eddy", C.c_double)]


class DomainLink(C.Structure):
    """ec3d_domain_link of include/ec3d_hip.h."""
    _fields_ = [("domain", C.c_int32), ("pad", C.c_int32), ("cells", C.c_int64), ("linkage", C.c_double),
                ("jsum", C.c_double * 3)]


class ProbeInfo(C.Structure):
    """ec3d_probe_info of include/ec3d_hip.h."""
    _fields_ = [("nprobes", C.c_int64), ("capacity", C.c_int64), ("recorded", C.c_int64), ("device_bytes", C.c_int64)]


class GuessInfo(C.Structure):
    """ec3d_guess_info of include/ec3d_hip.h."""
    _fields_ = [("depth", C.c_int32), ("stored", C.c_int32), ("used", C.c_int32), ("kept", C.c_int32),
                ("res_before", C.c_double), ("res_after", C.c_double), ("coef", C.c_double * 8)]


class NullInfo(C.Structure):
    """ec3d_null_info of include/ec3d_hip.h."""
    _fields_ = [("on", C.c_int32), ("built", C.c_int32), ("found", C.c_int32), ("kept", C.c_int32),
                ("dropped", C.c_int32), ("reported", C.c_int32), ("null_tol", C.c_double), ("removed", C.c_double),
                ("setup_ms", C.c_double), ("seed_row", C.c_int64 * 32), ("iterations", C.c_int32 * 32),
                ("was_kept", C.c_int32 * 32), ("residual", C.c_double * 32)]


class HarmonicInfo(C.Structure):
    """ec3d_harmonic_info of include/ec3d_hip.h."""
    _fields_ = [("ready", C.c_int32), ("iter", C.c_int32), ("restarts", C.c_int32), ("stop_kind", C.c_int32),
                ("omega", C.c_double), ("relres", C.c_double), ("ms", C.c_double), ("device_bytes", C.c_int64)]


class CsrProbe(C.Structure):
    _fields_ = [("structured", C.c_int32), ("sdx", C.c_int32), ("sdy", C.c_int32), ("sdz", C.c_int32),
                ("n_cond", C.c_int32), ("classes", C.c_int32), ("plane_pitch", C.c_int32)]


VEC = dict(X=0, B=1, R=2, R0=3, P=4, AP=5, S=6, AS=7)
VTK_SLOTS = 3   # EC3D_VTK_SLOTS of include/ec3d_hip.h: pinned buffers of the overlapped field output
KERNEL = dict(spmv=0, k1=1, k2=2, k3=3, k4=4, k5=5)
# algorithmic bytes per row of each kernel with 7 bands
KERNEL_BYTES_PER_ROW = dict(spmv=72, k1=80, k2=24, k3=72, k4=56, k5=32)

EXPORTS = ["sprsbcgstabwr_", "ec3d_invalidate", "ec3d_create", "ec3d_destroy", "ec3d_last_error",
           "ec3d_set_matrix_csr", "ec3d_assemble", "ec3d_assemble_poisson", "ec3d_solve",
           "ec3d_upload", "ec3d_download", "ec3d_device_vector", "ec3d_solve_resident", "ec3d_spmv",
           "ec3d_export_csr", "ec3d_get_cel_bnd", "ec3d_get_reduction_geometry",
           "ec3d_set_workgroups", "ec3d_get_matrix_info", "ec3d_time_kernel", "ec3d_time_iterations",
           "ec3d_iterate_begin", "ec3d_iterate", "ec3d_get_fusion", "ec3d_get_x_interval", "ec3d_get_x_groups", "ec3d_get_k4_form", "ec3d_get_band_placement", "ec3d_get_vector_placement", "ec3d_place_vectors", "ec3d_set_format", "ec3d_set_stream",
           "ec3d_assemble_poisson_slab", "ec3d_vector_layout", "ec3d_adopt_vectors",
           "ec3d_dist_configure", "ec3d_dist_step", "ec3d_dist_set_boundary_rows", "ec3d_read_state_async", "ec3d_read_state", "ec3d_get_restart_count", "ec3d_set_zmarch", "ec3d_can_overlap",
           "ec3d_rhs_step", "ec3d_post_update", "ec3d_assemble_slab", "ec3d_vtk_fields", "ec3d_vtk_fields_begin", "ec3d_vtk_fields_wait",
           "ec3d_set_structured", "ec3d_get_row_map", "ec3d_get_ulist", "ec3d_probe_csr",
           "ec3d_device_synchronize", "ec3d_format_real8",
           "ec3d_multi_create", "ec3d_multi_destroy", "ec3d_multi_ranks", "ec3d_multi_slab", "ec3d_multi_set_format",
           "ec3d_multi_assemble_poisson", "ec3d_multi_assemble", "ec3d_multi_set_matrix_csr", "ec3d_multi_size",
           "ec3d_multi_upload", "ec3d_multi_download", "ec3d_multi_solve", "ec3d_multi_solve_resident",
           "ec3d_multi_rhs_step", "ec3d_multi_post_update", "ec3d_multi_vtk_fields", "ec3d_multi_vtk_fields_begin",
           "ec3d_multi_vtk_fields_wait", "ec3d_multi_iterate_begin",
           "ec3d_multi_iterate", "ec3d_multi_synchronize", "ec3d_true_residual", "ec3d_multi_true_residual", "ec3d_get_visit_order", "ec3d_probe_csr_multi", "ec3d_multi_spmv", "ec3d_multi_api_calls", "ec3d_multi_plan", "ec3d_multi_halo_rows", "ec3d_rccl_unique_id", "ec3d_multi_create_rank", "ec3d_format_real8_gfortran", "ec3d_multi_iterate_timed", "ec3d_multi_rccl_info",
           "ec3d_set_preconditioner", "ec3d_get_preconditioner", "ec3d_precond_apply", "ec3d_set_u_rhs",
           "ec3d_set_precond_precision", "ec3d_get_precond_precision", "ec3d_set_precond_coarsening",
           "ec3d_get_precond_coarsening", "ec3d_set_precond_grid", "ec3d_get_precond_grid",
           "ec3d_domain_integrals", "ec3d_field_energy", "ec3d_domain_linkage", "ec3d_get_class_runs", "ec3d_get_patch_rows", "ec3d_get_k51_ap_form", "ec3d_set_guess_history", "ec3d_get_guess_history",
           "ec3d_spmv_t", "ec3d_set_null_projection", "ec3d_get_null_projection", "ec3d_left_null_vector",
           "ec3d_set_null_precond", "ec3d_get_null_precond", "ec3d_null_precond_apply",
           "ec3d_set_probes", "ec3d_probe_sample", "ec3d_probe_record", "ec3d_probe_read", "ec3d_probe_reset",
           "ec3d_get_probes",
           "ec3d_harmonic_setup", "ec3d_harmonic_upload", "ec3d_harmonic_download", "ec3d_harmonic_spmv",
           "ec3d_harmonic_solve", "ec3d_harmonic_true_residual", "ec3d_harmonic_load", "ec3d_get_harmonic",
           "ec3d_harmonic_device_vector",
           "ec3d_harmonic_set_null_projection", "ec3d_get_harmonic_null", "ec3d_harmonic_left_null_vector",
           "ec3d_harmonic_spmv_h", "ec3d_harmonic_projected_residual", "ec3d_harmonic_null_restarts",
           "ec3d_harmonic_batch_setup", "ec3d_harmonic_batch_upload", "ec3d_harmonic_batch_download",
           "ec3d_harmonic_batch_solve", "ec3d_get_harmonic_batch", "ec3d_harmonic_batch_select",
           "ec3d_harmonic_batch_device_vector",
           "ec3d_harmonic_batch_set_null_projection", "ec3d_get_harmonic_batch_null",
           "ec3d_harmonic_batch_left_null_vector", "ec3d_harmonic_batch_null_restarts",
           "ec3d_harmonic_batch_projected_residual"]
HARMONIC_MAX_BATCH = 16   # EC3D_HARMONIC_MAX_BATCH of include/ec3d_hip.h
PROBE_NCOMP = 13     # EC3D_PROBE_NCOMP of include/ec3d_hip.h: a[3], eddy[3], source[3], b[3], u
PROBE_E_FULL = 24    # EC3D_PROBE_E_FULL: ec3d_probe_record on a full buffer
U_RHS = {"reference": 0, "all": 1}   # EC3D_U_RHS_* of include/ec3d_hip.h
PRECOND = {"none": 0, "mg": 1, "block-mg": 2}   # EC3D_PRECOND_* of include/ec3d_hip.h
PRECOND_E_MATRIX, PRECOND_E_COARSE = 20, 21   # ec3d_set_preconditioner's refusals
NULL_PRECOND = {"none": 0, "block-mg": 1, "block-mg-a": 2}   # EC3D_NULL_PRECOND_* of include/ec3d_hip.h
NULL_PRECOND_MAX_LEVELS = 16
NULL_E_MATRIX, NULL_E_SETUP = 22, 23   # ec3d_set_null_projection's refusal, a set-up that did not reach null_tol
PRECOND_PRECISION = {"fp64": 0, "fp32": 1}   # EC3D_PRECOND_FP64 / _FP32 of include/ec3d_hip.h
PRECOND_COARSENING = {"rediscretize": 0, "aggregate": 1}   # EC3D_COARSEN_REDISCRETIZE / _AGGREGATE

_f64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i8 = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")
_lib = None


def torch_hip_runtime():
    """Path of the libamdhip64.so that PyTorch-ROCm bundles, or None (no torch installed, or it bundles none)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return cand if os.path.exists(cand) else None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (soname
    libamdhip64.so.7, the same as /opt/rocm's).  If this library pulled in the system copy first and
    torch were imported later (dist.py, bench.py), the process would hold two runtimes and torch would
    see no GPU.  So when torch is installed but not imported yet, load ITS runtime first; our DT_NEEDED
    then resolves to it by soname.  EC3D_HIP_RUNTIME=system keeps /opt/rocm's (torch-free processes)."""
    import sys
    if "torch" in sys.modules or os.environ.get("EC3D_HIP_RUNTIME") == "system":
        return
    cand = torch_hip_runtime()
    if cand:
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen libec3d_hip.so and declare every prototype of include/ec3d_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIBPATH
    if not os.path.exists(p):
        raise EC3DError(f"{p} not built: run `python -m eddy_currents_3d_amd.build` "
                        "(there is no CPU fallback)")
    _share_hip_runtime_with_torch()
    L = C.CDLL(p)
    if os.environ.get("EC3D_LIB"):
        # another (older) build for a same-box A/B timing (tools/ab_perf.py): entry points added since are absent
        # there; calling one raises AttributeError, declaring it must not
        class _Tolerant:
            def __init__(self, lib):
                object.__setattr__(self, "_lib", lib)

            def __getattr__(self, name):
                try:
                    return getattr(self._lib, name)
                except AttributeError:
                    class _Missing:
                        argtypes = restype = None

                        def __call__(self, *a):
                            raise EC3DError(f"{p} does not export {name}")
                    return _Missing()
        L = _Tolerant(L)
    hp = C.c_void_p
    L.ec3d_last_error.restype = C.c_char_p
    L.ec3d_create.argtypes = [C.POINTER(hp), C.c_int]
    L.ec3d_destroy.argtypes = [hp]
    L.ec3d_set_matrix_csr.argtypes = [hp, C.c_int32, _f64, _i32, _i32]
    L.ec3d_assemble.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, _i8, _i32, _f64, C.c_int32, _f64,
                                _f64, C.c_double]
    L.ec3d_assemble_poisson.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, _f64, _f64]
    L.ec3d_solve.argtypes = [hp, _f64, _f64, C.c_double, C.c_int32, C.POINTER(C.c_int32), hp, C.c_int32]
    L.ec3d_upload.argtypes = [hp, C.c_int, _f64]
    L.ec3d_download.argtypes = [hp, C.c_int, _f64]
    L.ec3d_device_vector.argtypes = [hp, C.c_int, C.POINTER(hp), C.POINTER(C.c_int64)]
    L.ec3d_solve_resident.argtypes = [hp, C.c_double, C.c_int32, C.POINTER(C.c_int32), hp, C.c_int32]
    L.ec3d_spmv.argtypes = [hp, _f64, _f64]
    L.ec3d_set_preconditioner.argtypes = [hp, C.c_int, C.c_int32, C.c_int32, C.c_int32]
    L.ec3d_get_preconditioner.argtypes = [hp, C.POINTER(C.c_int), C.POINTER(C.c_int32), hp]
    L.ec3d_precond_apply.argtypes = [hp, _f64, _f64]
    L.ec3d_set_u_rhs.argtypes = [hp, C.c_int32]
    L.ec3d_set_precond_precision.argtypes = [hp, C.c_int32]
    L.ec3d_get_precond_precision.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ec3d_set_precond_coarsening.argtypes = [hp, C.c_int32]
    L.ec3d_get_precond_coarsening.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), hp]
    L.ec3d_set_precond_grid.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32]
    L.ec3d_get_precond_grid.argtypes = [hp, hp]
    L.ec3d_set_guess_history.argtypes = [hp, C.c_int32]
    L.ec3d_get_guess_history.argtypes = [hp, C.POINTER(GuessInfo)]
    L.ec3d_spmv_t.argtypes = [hp, _f64, _f64]
    L.ec3d_set_null_projection.argtypes = [hp, C.c_int32, C.c_double]
    L.ec3d_get_null_projection.argtypes = [hp, C.POINTER(NullInfo)]
    L.ec3d_left_null_vector.argtypes = [hp, C.c_int32, _f64]
    L.ec3d_set_null_precond.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.ec3d_get_null_precond.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_double)]
    L.ec3d_null_precond_apply.argtypes = [hp, _f64, _f64]
    L.ec3d_export_csr.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), hp, hp, hp]
    L.ec3d_get_cel_bnd.argtypes = [hp, C.c_int, C.POINTER(C.c_int32), hp]
    L.ec3d_get_reduction_geometry.argtypes = [hp, C.c_int, C.POINTER(Geom)]
    L.ec3d_set_zmarch.argtypes = [hp, C.c_int]
    L.ec3d_can_overlap.argtypes = [hp]
    L.ec3d_assemble_slab.argtypes = [hp] + [C.c_int32] * 7 + [_i8, _i32, _f64, C.c_int32, _f64, _f64, C.c_double]
    L.ec3d_rhs_step.argtypes = [hp, C.c_int32, C.c_int32, _i32, _f64]
    L.ec3d_post_update.argtypes = [hp]
    L.ec3d_vtk_fields.argtypes = [hp, _f64, hp, hp, hp, hp]
    L.ec3d_vtk_fields_begin.argtypes = [hp, _f64, C.c_int32, C.POINTER(C.c_int32)]
    L.ec3d_domain_integrals.argtypes = [hp, _f64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(DomainIntegral)]
    L.ec3d_field_energy.argtypes = [hp, _f64, C.POINTER(FieldEnergy)]
    L.ec3d_domain_linkage.argtypes = [hp, _f64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(DomainLink)]
    L.ec3d_set_probes.argtypes = [hp, C.c_int64, C.c_void_p, C.c_int64]
    L.ec3d_probe_sample.argtypes = [hp, _f64, C.c_void_p]
    L.ec3d_probe_record.argtypes = [hp, _f64, C.c_double]
    L.ec3d_probe_read.argtypes = [hp, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.ec3d_probe_reset.argtypes = [hp]
    L.ec3d_get_probes.argtypes = [hp, C.POINTER(ProbeInfo)]
    L.ec3d_harmonic_setup.argtypes = [hp, C.c_double]
    L.ec3d_harmonic_upload.argtypes = [hp, C.c_int, C.c_void_p, C.c_void_p]
    L.ec3d_harmonic_download.argtypes = [hp, C.c_int, _f64, _f64]
    L.ec3d_harmonic_spmv.argtypes = [hp, C.c_void_p, C.c_void_p, _f64, _f64]
    L.ec3d_harmonic_solve.argtypes = [hp, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.ec3d_harmonic_true_residual.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ec3d_harmonic_load.argtypes = [hp, C.c_int32]
    L.ec3d_get_harmonic.argtypes = [hp, C.POINTER(HarmonicInfo)]
    L.ec3d_harmonic_device_vector.argtypes = [hp, C.c_int, C.POINTER(hp), C.POINTER(C.c_int64)]
    L.ec3d_harmonic_set_null_projection.argtypes = [hp, C.c_int32, C.c_double]
    L.ec3d_get_harmonic_null.argtypes = [hp, C.POINTER(NullInfo)]
    L.ec3d_harmonic_left_null_vector.argtypes = [hp, C.c_int32, _f64, _f64]
    L.ec3d_harmonic_spmv_h.argtypes = [hp, C.c_void_p, C.c_void_p, _f64, _f64]
    L.ec3d_harmonic_projected_residual.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ec3d_harmonic_null_restarts.argtypes = [hp, _i32]
    L.ec3d_harmonic_batch_setup.argtypes = [hp, C.c_int32, C.c_void_p]
    L.ec3d_harmonic_batch_upload.argtypes = [hp, C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
    L.ec3d_harmonic_batch_download.argtypes = [hp, C.c_int32, C.c_int, _f64, _f64]
    L.ec3d_harmonic_batch_solve.argtypes = [hp, C.c_double, C.c_int32, C.c_void_p]
    L.ec3d_get_harmonic_batch.argtypes = [hp, C.c_int32, C.POINTER(HarmonicInfo)]
    L.ec3d_harmonic_batch_select.argtypes = [hp, C.c_int32]
    L.ec3d_harmonic_batch_device_vector.argtypes = [hp, C.c_int32, C.c_int, C.POINTER(hp), C.POINTER(C.c_int64)]
    L.ec3d_harmonic_batch_set_null_projection.argtypes = [hp, C.c_int32, C.c_double]
    L.ec3d_get_harmonic_batch_null.argtypes = [hp, C.c_int32, C.POINTER(NullInfo), C.POINTER(C.c_int32)]
    L.ec3d_harmonic_batch_left_null_vector.argtypes = [hp, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.ec3d_harmonic_batch_null_restarts.argtypes = [hp, C.c_int32, C.c_void_p]
    L.ec3d_harmonic_batch_projected_residual.argtypes = [hp, C.c_void_p, C.c_void_p]
    L.ec3d_vtk_fields_wait.argtypes = [hp, C.c_int32] + [C.POINTER(C.POINTER(C.c_float))] * 4 + [C.POINTER(C.c_int64)]
    L.ec3d_set_workgroups.argtypes = [hp, C.c_int32]
    L.ec3d_get_matrix_info.argtypes = [hp, C.POINTER(MatrixInfo)]
    L.ec3d_time_kernel.argtypes = [hp, C.c_int, C.c_int32, C.POINTER(C.c_double)]
    L.ec3d_time_iterations.argtypes = [hp, C.c_int32, C.POINTER(C.c_double)]
    L.ec3d_device_synchronize.argtypes = [hp]
    L.ec3d_format_real8.argtypes = [C.c_double, C.c_char_p]
    L.ec3d_format_real8.restype = None
    L.ec3d_iterate_begin.argtypes = [hp]
    L.ec3d_iterate.argtypes = [hp, C.c_int32, C.c_int32, hp]
    L.ec3d_get_fusion.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ec3d_get_x_interval.argtypes = [hp, C.POINTER(C.c_int32)]
    L.ec3d_get_x_groups.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ec3d_get_k4_form.argtypes = [hp, C.POINTER(C.c_int32)]
    L.ec3d_get_band_placement.argtypes = [hp, C.c_int32, hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ec3d_get_vector_placement.argtypes = [hp, C.c_int32, hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.ec3d_place_vectors.argtypes = [hp, C.c_int32]
    L.ec3d_set_format.argtypes = [hp, C.c_int]
    L.ec3d_set_structured.argtypes = [hp, C.c_int]
    L.ec3d_get_row_map.argtypes = [hp, _i32]
    L.ec3d_dist_set_boundary_rows.argtypes = [hp, C.c_int32, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"),
                                              np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"),
                                              C.POINTER(C.c_int32)]
    L.ec3d_probe_csr.argtypes = [C.c_int32, _f64, _i32, _i32, C.POINTER(CsrProbe)]
    L.ec3d_probe_csr_multi.argtypes = [C.c_int32, _f64, _i32, _i32, C.c_int32, C.POINTER(C.c_int32)]
    L.ec3d_get_ulist.argtypes = [hp, _i32]
    L.ec3d_get_class_runs.argtypes = [hp, C.POINTER(C.c_int64), hp, C.c_int64]
    L.ec3d_get_patch_rows.argtypes = [hp, C.c_int, C.POINTER(C.c_int32)]
    L.ec3d_get_k51_ap_form.argtypes = [hp, C.POINTER(C.c_int32)]
    L.ec3d_set_stream.argtypes = [hp, hp]
    L.ec3d_assemble_poisson_slab.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f64, _f64]
    L.ec3d_vector_layout.argtypes = [hp] + [C.POINTER(C.c_int64)] * 4
    L.ec3d_adopt_vectors.argtypes = [hp, hp]
    L.ec3d_dist_configure.argtypes = [hp, C.c_int32, hp, hp]
    L.ec3d_dist_step.argtypes = [hp, C.c_int32, C.c_int32, C.c_double]
    L.ec3d_read_state_async.argtypes = [hp, C.c_void_p]
    L.ec3d_read_state.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.ec3d_get_restart_count.argtypes = [hp, C.POINTER(C.c_int32)]
    L.ec3d_get_visit_order.argtypes = [hp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), hp, hp]
    L.ec3d_true_residual.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ec3d_multi_true_residual.argtypes = [hp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ec3d_multi_create.argtypes = [C.POINTER(hp), C.c_int32, hp]
    L.ec3d_multi_destroy.argtypes = [hp]
    L.ec3d_multi_ranks.argtypes = [hp]
    L.ec3d_multi_slab.argtypes = [hp, C.c_int32, C.POINTER(hp), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ec3d_multi_set_format.argtypes = [hp, C.c_int, C.c_int]
    L.ec3d_multi_assemble_poisson.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, _f64, _f64]
    L.ec3d_multi_assemble.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, _i8, _i32, _f64, C.c_int32, _f64,
                                      _f64, C.c_double]
    L.ec3d_multi_set_matrix_csr.argtypes = [hp, C.c_int32, _f64, _i32, _i32]
    L.ec3d_multi_size.argtypes = [hp, C.POINTER(C.c_int64)]
    L.ec3d_multi_upload.argtypes = [hp, C.c_int, _f64]
    L.ec3d_multi_download.argtypes = [hp, C.c_int, _f64]
    L.ec3d_multi_solve.argtypes = [hp, _f64, _f64, C.c_double, C.c_int32, C.POINTER(C.c_int32)]
    L.ec3d_multi_solve_resident.argtypes = [hp, C.c_double, C.c_int32, C.POINTER(C.c_int32)]
    L.ec3d_multi_rhs_step.argtypes = [hp, C.c_int32, C.c_int32, _i32, _f64]
    L.ec3d_multi_post_update.argtypes = [hp]
    L.ec3d_multi_spmv.argtypes = [hp, _f64, _f64]
    L.ec3d_multi_vtk_fields.argtypes = [hp, _f64, hp, hp, hp, hp]
    L.ec3d_multi_vtk_fields_begin.argtypes = [hp, _f64, C.c_int32, C.POINTER(C.c_int32)]
    L.ec3d_multi_vtk_fields_wait.argtypes = ([hp, C.c_int32, C.c_int32] + [C.POINTER(C.POINTER(C.c_float))] * 4 +
                                             [C.POINTER(C.c_int64)] * 2)
    L.ec3d_multi_iterate_begin.argtypes = [hp]
    L.ec3d_multi_iterate.argtypes = [hp, C.c_int32, C.c_int32, hp]
    L.ec3d_multi_synchronize.argtypes = [hp]
    L.ec3d_multi_api_calls.argtypes = [hp, C.c_int32, C.POINTER(C.c_double)]
    L.ec3d_multi_iterate_timed.argtypes = [hp, C.c_int32, C.c_int32, C.c_int32, hp, hp, hp]
    L.ec3d_multi_rccl_info.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    L.ec3d_multi_plan.argtypes = [hp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ec3d_multi_halo_rows.argtypes = [hp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ec3d_rccl_unique_id.argtypes = [C.c_char_p]
    L.ec3d_multi_create_rank.argtypes = [C.POINTER(hp), C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, C.c_int32,
                                         C.c_int32]
    L.sprsbcgstabwr_.argtypes = [_f64, _i32, _i32, C.POINTER(C.c_int32), _f64, _f64,
                                 C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sprsbcgstabwr_.restype = None
    L.ec3d_invalidate.restype = None
    if path is None:
        _lib = L
    return L


def _chk(L, rc, what):
    if rc != 0:
        e = EC3DError(f"{what} failed ({rc}): {L.ec3d_last_error().decode()}")
        e.status = rc
        raise e


def probe_csr(valA, irow, jcol):
    """Host-only (no GPU): how would the library store this CSR matrix?  Returns a CsrProbe; `.structured`
    says whether the class-coded A-V form applies (include/ec3d_hip.h, ec3d_probe_csr)."""
    L = load_library()
    out = CsrProbe()
    irow = np.ascontiguousarray(irow, np.int32)
    rc = L.ec3d_probe_csr(len(irow) - 1, np.ascontiguousarray(valA, np.float64), irow,
                          np.ascontiguousarray(jcol, np.int32), C.byref(out))
    if rc:
        raise EC3DError(f"ec3d_probe_csr failed ({rc})")
    return out


def probe_csr_multi(valA, irow, jcol, nranks: int):
    """Host-only: (cuttable, reason) -- would the library cut this CSR matrix into `nranks` z-slabs
    (EC3DMulti.set_matrix_csr, the drop-in symbol under EC3D_NGPU)?"""
    L = load_library()
    ok = C.c_int32(0)
    irow = np.ascontiguousarray(irow, np.int32)
    rc = L.ec3d_probe_csr_multi(len(irow) - 1, np.ascontiguousarray(valA, np.float64), irow,
                                np.ascontiguousarray(jcol, np.int32), int(nranks), C.byref(ok))
    if rc:
        raise EC3DError(f"ec3d_probe_csr_multi failed ({rc})")
    return bool(ok.value), ("" if ok.value else L.ec3d_last_error().decode())


def sprsBCGstabWR(valA, irow, jcol, n, b, x, tolerance, itmax):
    """Drop-in for the reference solver (src/solvers.f90:3, called at src/EC3D.f90:408).

    ``valA`` f64[nnz], ``irow`` i32[n+1] and ``jcol`` i32[nnz] are the reference's 1-based CSR;
    ``x`` (f64[n], C-contiguous) is the warm start and receives the solution in place.
    Returns ``iter``.  Goes through the exported F77 symbol ``sprsbcgstabwr_`` itself."""
    L = load_library()
    if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
        raise TypeError("x must be a C-contiguous float64 ndarray (updated in place)")
    it = C.c_int32(0)
    L.sprsbcgstabwr_(np.ascontiguousarray(valA, np.float64), np.ascontiguousarray(irow, np.int32),
                     np.ascontiguousarray(jcol, np.int32), C.byref(C.c_int32(int(n))),
                     np.ascontiguousarray(b, np.float64), x, C.byref(C.c_double(float(tolerance))),
                     C.byref(C.c_int32(int(itmax))), C.byref(it))
    return it.value


class EC3DSolver:
    """Handle API of include/ec3d_hip.h (one HIP device, one stream)."""

    def __init__(self, device: int = 0, nblk: int | None = None, dictionary: bool | None = None,
                 structured: bool | None = None):
        self.L = load_library()
        self.h = C.c_void_p()
        _chk(self.L, self.L.ec3d_create(C.byref(self.h), device), "ec3d_create")
        if nblk:
            self.set_workgroups(nblk)
        if dictionary is not None:
            self.set_format(dictionary)
        if structured is not None:
            _chk(self.L, self.L.ec3d_set_structured(self.h, int(bool(structured))), "ec3d_set_structured")

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.ec3d_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- matrix ---------------------------------------------------------------------------
    def set_matrix_csr(self, valA, irow, jcol):
        irow = np.ascontiguousarray(irow, np.int32)
        _chk(self.L, self.L.ec3d_set_matrix_csr(self.h, len(irow) - 1, np.ascontiguousarray(valA, np.float64),
                                                irow, np.ascontiguousarray(jcol, np.int32)),
             "ec3d_set_matrix_csr")

    def assemble(self, geoPHYS, geoPHYS_C, valPHYS, BND, delta, dt):
        """geoPHYS/geoPHYS_C: [sdz, sdy, sdx] (C order == Fortran (i,j,k)); valPHYS (nsub_glob, 5);
        BND (3, 2).  Replaces gen_sparse_matrix (src/EC3D.f90:465-1049)."""
        sdz, sdy, sdx = geoPHYS.shape
        vp = np.asarray(valPHYS, np.float64)
        _chk(self.L, self.L.ec3d_assemble(
            self.h, sdx, sdy, sdz, np.ascontiguousarray(geoPHYS, np.int8).reshape(-1),
            np.ascontiguousarray(geoPHYS_C, np.int32).reshape(-1),
            np.ascontiguousarray(vp.T).reshape(-1), vp.shape[0],
            np.ascontiguousarray(np.asarray(BND, np.float64).T).reshape(-1),
            np.ascontiguousarray(delta, np.float64), float(dt)), "ec3d_assemble")

    def assemble_slab(self, sdz_global, e0, e1, k0, k1, geoPHYS_ext, geoPHYS_C_ext, valPHYS, BND, delta, dt):
        """One z-slab of the A-V system on the extended grid [e0, e1) (owned planes [k0, k1) + 2 halo
        planes per interior side); geoPHYS_C_ext numbers the extended slab's conducting cells locally."""
        nz, sdy, sdx = geoPHYS_ext.shape
        assert nz == e1 - e0
        vp = np.asarray(valPHYS, np.float64)
        _chk(self.L, self.L.ec3d_assemble_slab(
            self.h, sdx, sdy, sdz_global, e0, e1, k0, k1,
            np.ascontiguousarray(geoPHYS_ext, np.int8).reshape(-1),
            np.ascontiguousarray(geoPHYS_C_ext, np.int32).reshape(-1),
            np.ascontiguousarray(vp.T).reshape(-1), vp.shape[0],
            np.ascontiguousarray(np.asarray(BND, np.float64).T).reshape(-1),
            np.ascontiguousarray(delta, np.float64), float(dt)), "ec3d_assemble_slab")

    def ulist(self):
        """Occupied tiles of the U block (structured A-V form), in the order the kernels visit them."""
        k = self.geometry(0).ulist_n
        t = np.zeros(max(k, 1), np.int32)
        _chk(self.L, self.L.ec3d_get_ulist(self.h, t), "ec3d_get_ulist")
        return t[:k]

    def row_map(self):
        """Device row of every unknown of the reference's numbering (identity unless structured)."""
        m = np.empty(self.n, np.int32)
        _chk(self.L, self.L.ec3d_get_row_map(self.h, m), "ec3d_get_row_map")
        return m

    def set_format(self, dictionary: bool):
        """True (default): 1 class byte per row + coefficient table when the operator allows it;
        False: plain DIA coefficient streams.  Call before assembling / setting the matrix."""
        _chk(self.L, self.L.ec3d_set_format(self.h, int(bool(dictionary))), "ec3d_set_format")

    def assemble_poisson(self, sdx, sdy, sdz, delta=(0.00333, 0.00333, 0.00333), bnd=-0.95, slab=None):
        """Non-conducting Ax block (src/EC3D.f90:528-654).  slab=(k0, k1): only planes [k0, k1)."""
        BND = np.full(6, float(bnd)) if np.isscalar(bnd) else np.ascontiguousarray(
            np.asarray(bnd, np.float64).T).reshape(-1)
        d = np.ascontiguousarray(delta, np.float64)
        if slab is None:
            _chk(self.L, self.L.ec3d_assemble_poisson(self.h, sdx, sdy, sdz, BND, d), "ec3d_assemble_poisson")
        else:
            _chk(self.L, self.L.ec3d_assemble_poisson_slab(self.h, sdx, sdy, sdz, int(slab[0]), int(slab[1]),
                                                           BND, d), "ec3d_assemble_poisson_slab")

    def export_csr(self):
        n, nnz = C.c_int32(0), C.c_int64(0)
        _chk(self.L, self.L.ec3d_export_csr(self.h, C.byref(n), C.byref(nnz), None, None, None), "ec3d_export_csr")
        irow = np.empty(n.value + 1, np.int32)
        jcol = np.empty(nnz.value, np.int32)
        valA = np.empty(nnz.value, np.float64)
        _chk(self.L, self.L.ec3d_export_csr(self.h, C.byref(n), C.byref(nnz), irow.ctypes.data,
                                            jcol.ctypes.data, valA.ctypes.data), "ec3d_export_csr")
        return valA, irow, jcol

    def cel_bnd(self):
        out = []
        for w in range(6):
            k = C.c_int32(0)
            _chk(self.L, self.L.ec3d_get_cel_bnd(self.h, w, C.byref(k), None), "ec3d_get_cel_bnd")
            a = np.empty(max(k.value, 1), np.int32)
            _chk(self.L, self.L.ec3d_get_cel_bnd(self.h, w, C.byref(k), a.ctypes.data), "ec3d_get_cel_bnd")
            out.append(a[:k.value])
        return out

    @property
    def info(self) -> MatrixInfo:
        mi = MatrixInfo()
        _chk(self.L, self.L.ec3d_get_matrix_info(self.h, C.byref(mi)), "ec3d_get_matrix_info")
        return mi

    @property
    def n(self) -> int:
        return int(self.info.n)

    def geometry(self, which: int = 0) -> Geom:
        """Reduction geometry of the vector kernels (which=0) or of the SpMV kernels (which=1)."""
        g = Geom()
        _chk(self.L, self.L.ec3d_get_reduction_geometry(self.h, which, C.byref(g)), "ec3d_get_reduction_geometry")
        return g

    def visit_order(self, which: int = 0):
        """(offsets[nwg + 1], tiles): the 512-row tiles every workgroup of the vector kernels (0) / SpMV kernels
        (1) visits, in order -- the summation order of the dot products."""
        nwg, tot = C.c_int32(0), C.c_int64(0)
        _chk(self.L, self.L.ec3d_get_visit_order(self.h, which, C.byref(nwg), C.byref(tot), None, None),
             "ec3d_get_visit_order")
        off = np.zeros(nwg.value + 1, np.int32)
        tiles = np.zeros(max(tot.value, 1), np.int32)
        _chk(self.L, self.L.ec3d_get_visit_order(self.h, which, C.byref(nwg), C.byref(tot), off.ctypes.data,
                                                 tiles.ctypes.data), "ec3d_get_visit_order")
        return off, tiles[:tot.value]

    def class_runs(self) -> np.ndarray:
        """One byte per 2-D tile of a dictionary-form matrix: 1 = the tile's class bytes equal those of the tile a plane
        below (the z-marching kernels then keep theirs in registers).  Empty: the matrix has no such flags."""
        cnt = C.c_int64(0)
        _chk(self.L, self.L.ec3d_get_class_runs(self.h, C.byref(cnt), None, 0), "ec3d_get_class_runs")
        out = np.zeros(cnt.value, np.uint8)
        if cnt.value:
            _chk(self.L, self.L.ec3d_get_class_runs(self.h, C.byref(cnt), out.ctypes.data, out.size), "ec3d_get_class_runs")
        return out

    def patch_rows(self, kind: int = 0) -> int:
        """Patch rows per workgroup of a launch kind on the 2-D tiles (0: bare SpMV; 1: K2 inside K3; 2: K5 inside K1; 3: K4
        in SpMV form; 4: setup residual, K1, K3): 8 where y-adjacent patch columns are paired, 4 otherwise, 0 without 2-D
        tiles."""
        rows = C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_patch_rows(self.h, int(kind), C.byref(rows)), "ec3d_get_patch_rows")
        return rows.value

    def k51_ap_form(self) -> int:
        """1 where K5 inside K1 sums the old A*P of a workgroup's own patch again from the old P instead of loading the stored
        AP there (EC3D_K51_AP; the undivided dictionary cube on 2-D tiles only), 0 where it loads AP everywhere."""
        v = C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_k51_ap_form(self.h, C.byref(v)), "ec3d_get_k51_ap_form")
        return v.value

    def set_zmarch(self, on: bool):
        _chk(self.L, self.L.ec3d_set_zmarch(self.h, int(bool(on))), "ec3d_set_zmarch")

    def set_workgroups(self, nblk: int):
        _chk(self.L, self.L.ec3d_set_workgroups(self.h, int(nblk)), "ec3d_set_workgroups")

    # ---- solve ----------------------------------------------------------------------------
    def solve(self, b, x0, tolerance, itmax, hist_cap: int = 0):
        """One reference solve (src/solvers.f90:3-50).  Returns (x, iter, hist[hist_cap, 2])."""
        x = np.array(x0, dtype=np.float64, copy=True)
        it = C.c_int32(0)
        hist = np.full((max(hist_cap, 1), 2), np.nan)
        _chk(self.L, self.L.ec3d_solve(self.h, np.ascontiguousarray(b, np.float64), x, float(tolerance),
                                       int(itmax), C.byref(it), hist.ctypes.data if hist_cap else None,
                                       hist_cap), "ec3d_solve")
        return x, it.value, hist[:hist_cap]

    def upload(self, which: str, a):
        _chk(self.L, self.L.ec3d_upload(self.h, VEC[which], np.ascontiguousarray(a, np.float64)), "ec3d_upload")

    def download(self, which: str):
        a = np.empty(self.n)
        _chk(self.L, self.L.ec3d_download(self.h, VEC[which], a), "ec3d_download")
        return a

    def device_vector(self, which: str):
        p, n = C.c_void_p(), C.c_int64(0)
        _chk(self.L, self.L.ec3d_device_vector(self.h, VEC[which], C.byref(p), C.byref(n)), "ec3d_device_vector")
        return p.value, n.value

    def solve_resident(self, tolerance, itmax, hist_cap: int = 0):
        it = C.c_int32(0)
        hist = np.full((max(hist_cap, 1), 2), np.nan)
        _chk(self.L, self.L.ec3d_solve_resident(self.h, float(tolerance), int(itmax), C.byref(it),
                                                hist.ctypes.data if hist_cap else None, hist_cap),
             "ec3d_solve_resident")
        return it.value, hist[:hist_cap]

    # ---- time-loop field work on the resident vectors (src/EC3D.f90:275-404, :412-433) --------
    def rhs_step(self, src_index, src_value, moving: bool = False):
        """Jaf for this step: source scatter (1-based unknown ids, values from the host's source
        functions), inertial terms, U-row right-hand sides, cel_bnd* zero-fills."""
        idx = np.ascontiguousarray(src_index, np.int32)
        val = np.ascontiguousarray(src_value, np.float64)
        _chk(self.L, self.L.ec3d_rhs_step(self.h, int(bool(moving)), len(idx), idx if len(idx) else np.zeros(1, np.int32),
                                          val if len(val) else np.zeros(1)), "ec3d_rhs_step")

    def post_update(self):
        _chk(self.L, self.L.ec3d_post_update(self.h), "ec3d_post_update")

    def vtk_fields(self, delta, ncells: int, conducting: bool, zero_eddy: bool = False):
        """float32 point vectors of field_N.vtk (src/utilites.f90:222-289) from the resident X, B.
        Returns dict(A, eddy (None without conductors), source, B), each (ncells, 3); ncells = the cells the
        handle owns.  zero_eddy: start the eddy field from zeros (a z-slab that holds no conductor)."""
        mk = lambda: np.empty((ncells, 3), np.float32)
        fa, fs, fb = mk(), mk(), mk()
        fe = (np.zeros((ncells, 3), np.float32) if zero_eddy else mk()) if conducting else None
        _chk(self.L, self.L.ec3d_vtk_fields(self.h, np.ascontiguousarray(delta, np.float64), fa.ctypes.data,
                                            fe.ctypes.data if conducting else None, fs.ctypes.data,
                                            fb.ctypes.data), "ec3d_vtk_fields")
        return dict(A=fa, eddy=fe, source=fs, B=fb)

    def domain_integrals(self, delta):
        """Joule loss and Lorentz force per conducting domain from the resident X, B (ec3d_domain_integrals): the
        integrals of the fields field_N.vtk shows, in float64, summed on the device.  A list, ascending domain id, of
        dict(domain, cells, sigma [S/m], joule_w [W], force_n [N], numpy array of 3); empty without conductors.
        Meaningful after post_update of a step."""
        d = np.ascontiguousarray(delta, np.float64)
        n = C.c_int32(0)
        _chk(self.L, self.L.ec3d_domain_integrals(self.h, d, 0, C.byref(n), None), "ec3d_domain_integrals")
        if n.value == 0:
            return []
        out = (DomainIntegral * n.value)()
        _chk(self.L, self.L.ec3d_domain_integrals(self.h, d, n.value, C.byref(n), out), "ec3d_domain_integrals")
        return [dict(domain=int(r.domain), cells=int(r.cells), sigma=float(r.sigma), joule_w=float(r.joule_w),
                     force_n=np.array(r.force_n[:], np.float64)) for r in out[:n.value]]

    def field_energy(self, delta):
        """Magnetic energy of the box and the integral of A.J from the resident X, B (ec3d_field_energy), in float64,
        summed on the device in a fixed order: dict(cells, energy_b [J], energy_axis (numpy array of 3: the x, y, z
        parts of energy_b), aj_source [J] (outside the conductors), aj_eddy [J] (inside)).  Meaningful after
        post_update of a step."""
        r = FieldEnergy()
        _chk(self.L, self.L.ec3d_field_energy(self.h, np.ascontiguousarray(delta, np.float64), C.byref(r)),
             "ec3d_field_energy")
        return dict(cells=int(r.cells), energy_b=float(r.energy_b), energy_axis=np.array(r.energy_axis[:], np.float64),
                    aj_source=float(r.aj_source), aj_eddy=float(r.aj_eddy))

    def domain_linkage(self, delta):
        """Flux linkage of every non-conducting domain (the coils, the plain bodies and the air) from the resident X, B
        (ec3d_domain_linkage).  A list, ascending domain id, of dict(domain, cells, linkage [J] (psi * I), jsum [A m],
        numpy array of 3).  Meaningful after post_update of a step."""
        d = np.ascontiguousarray(delta, np.float64)
        n = C.c_int32(0)
        _chk(self.L, self.L.ec3d_domain_linkage(self.h, d, 0, C.byref(n), None), "ec3d_domain_linkage")
        if n.value == 0:
            return []
        out = (DomainLink * n.value)()
        _chk(self.L, self.L.ec3d_domain_linkage(self.h, d, n.value, C.byref(n), out), "ec3d_domain_linkage")
        return [dict(domain=int(r.domain), cells=int(r.cells), linkage=float(r.linkage),
                     jsum=np.array(r.jsum[:], np.float64)) for r in out[:n.value]]

    # ---- probes: the fields at chosen cells (ec3d_set_probes ... ec3d_get_probes) --------------
    def set_probes(self, cells, capacity: int = 0):
        """The probe set: 0-based cell numbers i + j*sdx + k*sdx*sdy in any order, duplicates allowed
        (eddy_currents_3d_amd.probes builds lines and boxes); ``capacity``: records the device buffer holds (0:
        probe_sample only).  An empty list clears the set.  A new assemble clears it too."""
        cells = np.ascontiguousarray(cells, np.int64).reshape(-1)
        _chk(self.L, self.L.ec3d_set_probes(self.h, len(cells), cells.ctypes.data if len(cells) else None, int(capacity)),
             "ec3d_set_probes")

    def probes(self):
        """dict(nprobes, capacity, recorded, device_bytes) of the probe set (ec3d_get_probes)."""
        r = ProbeInfo()
        _chk(self.L, self.L.ec3d_get_probes(self.h, C.byref(r)), "ec3d_get_probes")
        return dict(nprobes=int(r.nprobes), capacity=int(r.capacity), recorded=int(r.recorded),
                    device_bytes=int(r.device_bytes))

    @staticmethod
    def _probe_dict(v):
        """(..., 13, nprobes) as the library lays it out -> dict of a, eddy, source, b (..., nprobes, 3), u (..., nprobes)."""
        m = np.moveaxis(v, -2, -1)
        return dict(a=np.ascontiguousarray(m[..., 0:3]), eddy=np.ascontiguousarray(m[..., 3:6]),
                    source=np.ascontiguousarray(m[..., 6:9]), b=np.ascontiguousarray(m[..., 9:12]),
                    u=np.ascontiguousarray(m[..., 12]))

    def probe_sample(self, delta):
        """The fields at the probes from the resident X, B (ec3d_probe_sample), in float64: dict of a, eddy, source, b
        of shape (nprobes, 3) and u of shape (nprobes,) -- what field_N.vtk shows at those cells before its rounding to
        float32, and the scalar potential.  Meaningful after post_update of a step."""
        n = self.probes()["nprobes"]
        out = np.empty((PROBE_NCOMP, n), np.float64)
        _chk(self.L, self.L.ec3d_probe_sample(self.h, np.ascontiguousarray(delta, np.float64), out.ctypes.data),
             "ec3d_probe_sample")
        return self._probe_dict(out)

    def probe_record(self, delta, T: float):
        """Append the same sample to the record on the device WITHOUT waiting (ec3d_probe_record); ``T`` is kept with
        it.  Raises EC3DError with status PROBE_E_FULL when the buffer is full."""
        _chk(self.L, self.L.ec3d_probe_record(self.h, np.ascontiguousarray(delta, np.float64), float(T)),
             "ec3d_probe_record")

    def probe_read(self, first: int = 0, count: int | None = None):
        """Records [first, first + count) (default: all from ``first``) with one copy (ec3d_probe_read): (T, dict) with
        T of shape (count,) and the arrays of probe_sample with a leading step axis."""
        q = self.probes()
        if count is None:
            count = max(q["recorded"] - int(first), 0)
        T = np.empty(max(int(count), 0), np.float64)
        out = np.empty((max(int(count), 0), PROBE_NCOMP, q["nprobes"]), np.float64)
        _chk(self.L, self.L.ec3d_probe_read(self.h, int(first), int(count), T.ctypes.data, out.ctypes.data),
             "ec3d_probe_read")
        return T, self._probe_dict(out)

    def probe_reset(self):
        """recorded = 0; the set and the buffer stay (ec3d_probe_reset)."""
        _chk(self.L, self.L.ec3d_probe_reset(self.h), "ec3d_probe_reset")

    def vtk_fields_begin(self, delta, big_endian: bool = True) -> int:
        """Start the field output of this step WITHOUT waiting (ec3d_vtk_fields_begin): the field kernel on the
        handle's stream, the copy into one of two pinned host buffers on a side stream.  Returns the slot to hand to
        :meth:`vtk_fields_wait`; the caller goes on with the next step's rhs_step / solve_resident."""
        slot = C.c_int32(0)
        _chk(self.L, self.L.ec3d_vtk_fields_begin(self.h, np.ascontiguousarray(delta, np.float64), int(big_endian),
                                                  C.byref(slot)), "ec3d_vtk_fields_begin")
        return slot.value

    def vtk_fields_wait(self, slot: int, big_endian: bool = True):
        """Block until slot's copy has landed; dict(A, eddy (None without conductors), source, B) of (ncells, 3)
        arrays that VIEW the library's pinned buffer (dtype '>f4' when big_endian): valid until the third
        vtk_fields_begin after the one that returned this slot (VTK_SLOTS buffers, taken in turn)."""
        p = [C.POINTER(C.c_float)() for _ in range(4)]
        n = C.c_int64(0)
        _chk(self.L, self.L.ec3d_vtk_fields_wait(self.h, slot, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3]),
                                                 C.byref(n)), "ec3d_vtk_fields_wait")
        dt = np.dtype(">f4") if big_endian else np.dtype(np.float32)

        def view(q):
            if not q:
                return None
            return np.ctypeslib.as_array(q, shape=(n.value * 3,)).view(dt).reshape(n.value, 3)
        return dict(A=view(p[0]), eddy=view(p[1]), source=view(p[2]), B=view(p[3]))

    def true_residual(self):
        """(||B - A X|| / ||B||, ||B||) of the resident vectors, computed on the device."""
        rel, bn = C.c_double(0), C.c_double(0)
        _chk(self.L, self.L.ec3d_true_residual(self.h, C.byref(rel), C.byref(bn)), "ec3d_true_residual")
        return rel.value, bn.value

    def spmv(self, x):
        y = np.empty(self.n)
        _chk(self.L, self.L.ec3d_spmv(self.h, np.ascontiguousarray(x, np.float64), y), "ec3d_spmv")
        return y

    def spmv_t(self, x):
        """y = A^T x through the transposed kernel of the structured A-V form (ec3d_spmv_t): a row's terms in ascending
        source row.  EC3DError with .status NULL_E_MATRIX on any other matrix form, 4 on a z-slab."""
        y = np.empty(self.n)
        _chk(self.L, self.L.ec3d_spmv_t(self.h, np.ascontiguousarray(x, np.float64), y), "ec3d_spmv_t")
        return y

    # ---- time-harmonic solve (ec3d_harmonic_*) ---------------------------
    @staticmethod
    def _parts(z, n):
        z = np.asarray(z)
        if z.shape != (n,):
            raise ValueError(f"expected a vector of {n} entries, got shape {z.shape}")
        return np.ascontiguousarray(z.real, np.float64), np.ascontiguousarray(z.imag, np.float64)

    @staticmethod
    def _complex(re, im):
        z = np.empty(len(re), np.complex128)     # (re + 1j * im would turn a -0.0 into +0.0)
        z.real, z.imag = re, im
        return z

    def harmonic_setup(self, omega: float):
        """The operator K + j omega M on this handle's A-V system and, on the first call, the complex work vectors
        (ec3d_harmonic_setup).  EC3DError with .status 3 / 5 / NULL_E_MATRIX on a handle that has no undivided
        structured A-V system, 2 for a negative or non-finite omega."""
        _chk(self.L, self.L.ec3d_harmonic_setup(self.h, float(omega)), "ec3d_harmonic_setup")

    def harmonic_upload(self, which: str, z):
        """X^ or B^ from a complex (or real) vector in the reference numbering."""
        re, im = self._parts(z, self.n)
        _chk(self.L, self.L.ec3d_harmonic_upload(self.h, VEC[which], re.ctypes.data, im.ctypes.data), "ec3d_harmonic_upload")

    def harmonic_download(self, which: str):
        re, im = np.empty(self.n), np.empty(self.n)
        _chk(self.L, self.L.ec3d_harmonic_download(self.h, VEC[which], re, im), "ec3d_harmonic_download")
        return self._complex(re, im)

    def harmonic_spmv(self, x=None):
        """(K + j omega M) x; x = None: the resident X^."""
        yre, yim = np.empty(self.n), np.empty(self.n)
        if x is None:
            rc = self.L.ec3d_harmonic_spmv(self.h, None, None, yre, yim)
        else:
            re, im = self._parts(x, self.n)
            rc = self.L.ec3d_harmonic_spmv(self.h, re.ctypes.data, im.ctypes.data, yre, yim)
        _chk(self.L, rc, "ec3d_harmonic_spmv")
        return self._complex(yre, yim)

    def harmonic_solve(self, tolerance: float, itmax: int):
        """Complex BiCGSTAB with restart from the resident X^ (src/solvers.f90:3-50).  Returns (iter, relres)."""
        it, rr = C.c_int32(0), C.c_double(0)
        _chk(self.L, self.L.ec3d_harmonic_solve(self.h, float(tolerance), int(itmax), C.byref(it), C.byref(rr)),
             "ec3d_harmonic_solve")
        return it.value, rr.value

    def harmonic_true_residual(self):
        """(||b^ - A x^|| / ||b^||, ||b^||) of the resident complex vectors."""
        rel, bn = C.c_double(0), C.c_double(0)
        _chk(self.L, self.L.ec3d_harmonic_true_residual(self.h, C.byref(rel), C.byref(bn)), "ec3d_harmonic_true_residual")
        return rel.value, bn.value

    def harmonic_load(self, part: int):
        """Re (0) or Im (1) of the phasor into the real X and B: every observable of the resident fields then returns
        that part's (ec3d_harmonic_load)."""
        _chk(self.L, self.L.ec3d_harmonic_load(self.h, int(part)), "ec3d_harmonic_load")

    def harmonic_info(self):
        """dict(ready, omega, iter, restarts, stop_kind, relres, ms, device_bytes) (ec3d_get_harmonic)."""
        r = HarmonicInfo()
        _chk(self.L, self.L.ec3d_get_harmonic(self.h, C.byref(r)), "ec3d_get_harmonic")
        return dict(ready=bool(r.ready), omega=float(r.omega), iter=int(r.iter), restarts=int(r.restarts),
                    stop_kind=int(r.stop_kind), relres=float(r.relres), ms=float(r.ms), device_bytes=int(r.device_bytes))

    def harmonic_device_vector(self, which: str):
        """(device address, n_pad) of a complex work vector: interleaved (re, im) pairs in device numbering."""
        p, n = C.c_void_p(), C.c_int64(0)
        _chk(self.L, self.L.ec3d_harmonic_device_vector(self.h, VEC[which], C.byref(p), C.byref(n)),
             "ec3d_harmonic_device_vector")
        return p.value, n.value

    def harmonic_set_null_projection(self, on: bool = True, null_tol: float = 1e-10):
        """Take the left null vectors of K + j omega M out of every harmonic solve's initial residual, so that
        tolerances below |q^H b^| / ||b^|| can be reached (ec3d_harmonic_set_null_projection).
        The first harmonic_solve on a matrix and omega finds one complex vector per connected conducting component by
        an adjoint solve to ``null_tol``.  The setting stays with the handle; the vectors go with the matrix and with
        omega.  EC3DError with the .status of the other harmonic calls on a refusal, the setting then as it was; a
        solve whose set-up misses ``null_tol`` raises with .status NULL_E_SETUP."""
        _chk(self.L, self.L.ec3d_harmonic_set_null_projection(self.h, 1 if on else 0, float(null_tol)),
             "ec3d_harmonic_set_null_projection")

    def harmonic_null_projection(self):
        """The dict of null_projection() for the harmonic operator's vectors (ec3d_get_harmonic_null): residual =
        ||A^H w|| / ||w||, removed = sqrt(sum |c_i|^2) / ||b^|| of the last projected solve; every component also has
        ``restarts``, its adjoint solve's restart count."""
        g = NullInfo()
        _chk(self.L, self.L.ec3d_get_harmonic_null(self.h, C.byref(g)), "ec3d_get_harmonic_null")
        rs = np.zeros(32, np.int32)
        _chk(self.L, self.L.ec3d_harmonic_null_restarts(self.h, rs), "ec3d_harmonic_null_restarts")
        comps = [dict(seed_row=int(g.seed_row[i]), iterations=int(g.iterations[i]), residual=float(g.residual[i]),
                      kept=bool(g.was_kept[i]), restarts=int(rs[i])) for i in range(int(g.reported))]
        return dict(on=bool(g.on), built=bool(g.built), found=int(g.found), kept=int(g.kept), dropped=int(g.dropped),
                    null_tol=float(g.null_tol), removed=float(g.removed), setup_ms=float(g.setup_ms), components=comps)

    def harmonic_left_null_vector(self, index: int = 0):
        """Kept left null vector ``index`` of K + j omega M (complex, unit norm, the reference numbering); builds the
        vectors when the projection is on and they do not exist yet."""
        re, im = np.empty(self.n), np.empty(self.n)
        _chk(self.L, self.L.ec3d_harmonic_left_null_vector(self.h, int(index), re, im), "ec3d_harmonic_left_null_vector")
        return self._complex(re, im)

    def harmonic_spmv_h(self, x=None):
        """(K + j omega M)^H x; x = None: the resident X^."""
        yre, yim = np.empty(self.n), np.empty(self.n)
        if x is None:
            rc = self.L.ec3d_harmonic_spmv_h(self.h, None, None, yre, yim)
        else:
            re, im = self._parts(x, self.n)
            rc = self.L.ec3d_harmonic_spmv_h(self.h, re.ctypes.data, im.ctypes.data, yre, yim)
        _chk(self.L, rc, "ec3d_harmonic_spmv_h")
        return self._complex(yre, yim)

    def harmonic_projected_residual(self):
        """(||P (b^ - A x^)|| / ||b^||, removed) with the handle's left null vectors: what a projected solve converges
        to, where harmonic_true_residual shows the floor."""
        rel, rem = C.c_double(0), C.c_double(0)
        _chk(self.L, self.L.ec3d_harmonic_projected_residual(self.h, C.byref(rel), C.byref(rem)),
             "ec3d_harmonic_projected_residual")
        return rel.value, rem.value

    # ---- a batch of harmonic systems in lock step (ec3d_harmonic_batch_*) ----
    def harmonic_batch_setup(self, omegas):
        """A batch of len(omegas) systems (omega_s, b^_s, x^_s), at most HARMONIC_MAX_BATCH, on this handle's A-V system,
        with storage of its own (ec3d_harmonic_batch_setup); equal omegas are allowed; an empty list frees the batch.
        EC3DError with .status 3 / 5 / NULL_E_MATRIX as harmonic_setup, 2 for too many systems or a negative or
        non-finite omega; the batch is then as it was."""
        w = np.ascontiguousarray(omegas, np.float64).reshape(-1)
        _chk(self.L, self.L.ec3d_harmonic_batch_setup(self.h, len(w), w.ctypes.data if len(w) else None),
             "ec3d_harmonic_batch_setup")
        self._harmonic_batch_nsys = len(w)

    def harmonic_batch_upload(self, sys: int, which: str, z):
        """X^ or B^ of system ``sys`` from a complex (or real) vector in the reference numbering."""
        re, im = self._parts(z, self.n)
        _chk(self.L, self.L.ec3d_harmonic_batch_upload(self.h, int(sys), VEC[which], re.ctypes.data, im.ctypes.data),
             "ec3d_harmonic_batch_upload")

    def harmonic_batch_download(self, sys: int, which: str):
        re, im = np.empty(self.n), np.empty(self.n)
        _chk(self.L, self.L.ec3d_harmonic_batch_download(self.h, int(sys), VEC[which], re, im), "ec3d_harmonic_batch_download")
        return self._complex(re, im)

    def harmonic_batch_solve(self, tolerance: float, itmax: int):
        """Every system of the batch from its resident X^, in lock step: each gets the bits of its own harmonic_solve.
        Returns [(iter, relres), ...], one per system.  EC3DError with .status 2 while harmonic_set_null_projection
        is on."""
        it = np.zeros(HARMONIC_MAX_BATCH, np.int32)
        _chk(self.L, self.L.ec3d_harmonic_batch_solve(self.h, float(tolerance), int(itmax), it.ctypes.data),
             "ec3d_harmonic_batch_solve")
        out, r = [], HarmonicInfo()
        while len(out) < HARMONIC_MAX_BATCH and self.L.ec3d_get_harmonic_batch(self.h, len(out), C.byref(r)) == 0:
            out.append((int(it[len(out)]), float(r.relres)))     # (the first system outside the batch ends the list)
        return out

    def harmonic_batch_info(self, sys: int):
        """The dict of harmonic_info() for system ``sys``; ms and device_bytes are the whole batch's
        (ec3d_get_harmonic_batch)."""
        r = HarmonicInfo()
        _chk(self.L, self.L.ec3d_get_harmonic_batch(self.h, int(sys), C.byref(r)), "ec3d_get_harmonic_batch")
        return dict(ready=bool(r.ready), omega=float(r.omega), iter=int(r.iter), restarts=int(r.restarts),
                    stop_kind=int(r.stop_kind), relres=float(r.relres), ms=float(r.ms), device_bytes=int(r.device_bytes))

    def harmonic_batch_select(self, sys: int):
        """harmonic_setup(omega_sys) and device copies of system ``sys``'s x^ and b^ into the resident single X^ and B^:
        harmonic_true_residual, harmonic_load and every observable behind it, and a further harmonic_solve then work on
        that system.  The batch keeps its vectors."""
        _chk(self.L, self.L.ec3d_harmonic_batch_select(self.h, int(sys)), "ec3d_harmonic_batch_select")

    def harmonic_batch_device_vector(self, sys: int, which: str):
        """(device address, n_pad) of a complex work vector of system ``sys``."""
        p, n = C.c_void_p(), C.c_int64(0)
        _chk(self.L, self.L.ec3d_harmonic_batch_device_vector(self.h, int(sys), VEC[which], C.byref(p), C.byref(n)),
             "ec3d_harmonic_batch_device_vector")
        return p.value, n.value

    # ---- the left null vectors inside a batch ----
    def harmonic_batch_set_null_projection(self, on: bool = True, null_tol: float = 1e-10):
        """Take the left null vectors of every system's own K + j omega_s M out of its initial residual in
        harmonic_batch_solve (ec3d_harmonic_batch_set_null_projection): each system then gets the bits of its own
        harmonic_solve with harmonic_set_null_projection on.  A setting of the batch, separate from the single solve's;
        needs a batch (switching off does not).  The first solve of a batch builds the vectors, the adjoint solves of
        the batch's distinct omegas in lock step; a set-up that misses ``null_tol`` raises with .status NULL_E_SETUP."""
        _chk(self.L, self.L.ec3d_harmonic_batch_set_null_projection(self.h, 1 if on else 0, float(null_tol)),
             "ec3d_harmonic_batch_set_null_projection")

    def harmonic_batch_null_projection(self, sys: int):
        """The dict of harmonic_null_projection() for system ``sys`` (ec3d_get_harmonic_batch_null): setup_ms is the
        whole set-up's, removed that of the system's last projection; ``shares_with``: the lowest system with the same
        omega, whose vectors this system uses."""
        g, sw = NullInfo(), C.c_int32(-1)
        _chk(self.L, self.L.ec3d_get_harmonic_batch_null(self.h, int(sys), C.byref(g), C.byref(sw)), "ec3d_get_harmonic_batch_null")
        rs = np.zeros(32, np.int32)
        _chk(self.L, self.L.ec3d_harmonic_batch_null_restarts(self.h, int(sys), rs.ctypes.data), "ec3d_harmonic_batch_null_restarts")
        comps = [dict(seed_row=int(g.seed_row[i]), iterations=int(g.iterations[i]), residual=float(g.residual[i]),
                      kept=bool(g.was_kept[i]), restarts=int(rs[i])) for i in range(int(g.reported))]
        return dict(on=bool(g.on), built=bool(g.built), found=int(g.found), kept=int(g.kept), dropped=int(g.dropped),
                    null_tol=float(g.null_tol), removed=float(g.removed), setup_ms=float(g.setup_ms), components=comps,
                    shares_with=int(sw.value))

    def harmonic_batch_left_null_vector(self, sys: int, index: int = 0):
        """Kept left null vector ``index`` of system ``sys``'s operator (complex, unit norm, the reference numbering);
        builds the batch's vectors when the projection is on and they do not exist yet."""
        re, im = np.empty(self.n), np.empty(self.n)
        _chk(self.L, self.L.ec3d_harmonic_batch_left_null_vector(self.h, int(sys), int(index), re.ctypes.data, im.ctypes.data),
             "ec3d_harmonic_batch_left_null_vector")
        return self._complex(re, im)

    def harmonic_batch_projected_residual(self):
        """[(||P_s (b^_s - A_s x^_s)|| / ||b^_s||, removed_s), ...], one per system, with each system's own vectors."""
        rel, rem = np.zeros(HARMONIC_MAX_BATCH), np.zeros(HARMONIC_MAX_BATCH)
        _chk(self.L, self.L.ec3d_harmonic_batch_projected_residual(self.h, rel.ctypes.data, rem.ctypes.data),
             "ec3d_harmonic_batch_projected_residual")
        return [(float(rel[k]), float(rem[k])) for k in range(getattr(self, "_harmonic_batch_nsys", 0))]

    def set_u_rhs(self, rule: str = "reference"):
        """Which U rows rhs_step gives their right-hand side with several conducting domains: "reference" (default)
        only the rows n <= max siznod, as src/EC3D.f90:374-392 does; "all" every U row, the consistent form and a
        departure from the reference.  Identical with one domain.  Kept across assemblies."""
        if rule not in U_RHS:
            raise ValueError(f"u_rhs must be one of {sorted(U_RHS)}, not {rule!r}")
        _chk(self.L, self.L.ec3d_set_u_rhs(self.h, U_RHS[rule]), "ec3d_set_u_rhs")

    # ---- preconditioner ("mg": a matrix from assemble_poisson, or a 7-point matrix from set_matrix_csr with its grid;
    # "block-mg": the structured A-V form) ------------------------------------------------------------------------
    def set_preconditioner(self, kind: str = "mg", pre: int = 2, post: int = 2, coarse_sweeps: int = 0,
                           precision: str | None = None, coarsening: str | None = None, grid=None):
        """"mg": solves run the right-preconditioned iteration with one multigrid V-cycle as M; "block-mg": the same
        iteration on the A-V system of assemble, M one Galerkin V-cycle per A block and Gauss-Seidel sweeps on U;
        "none": the reference's iteration.  Zeros select the library's defaults.  ``precision`` ("fp64" or "fp32"):
        set_precond_precision(precision) first -- the handle keeps it, unless the call is refused; None leaves the
        handle's setting as it is.  ``coarsening`` ("rediscretize" or "aggregate"): set_precond_coarsening likewise.
        ``grid`` ((sdx, sdy, sdz)): set_precond_grid(*grid) likewise -- the matrix from set_matrix_csr is a 7-point
        operator on that box, and "mg" builds its hierarchy from the matrix alone.
        Refusal: EC3DError with .status PRECOND_E_MATRIX or PRECOND_E_COARSE (2 for a grid that does not fit the
        matrix), the handle unchanged."""
        undo = []   # a refusal leaves the handle unchanged, the settings given here included
        try:
            if precision is not None:
                undo.append((self.set_precond_precision, self.precond_precision()[0]))
                self.set_precond_precision(precision)
            if coarsening is not None:
                undo.append((self.set_precond_coarsening, self._coarsening_setting()))
                self.set_precond_coarsening(coarsening)
            if grid is not None:
                before = self.precond_grid()
                self.set_precond_grid(*grid)
                undo.append((lambda g: self.set_precond_grid(*g), before or (0, 0, 0)))
            _chk(self.L, self.L.ec3d_set_preconditioner(self.h, PRECOND[kind], pre, post, coarse_sweeps),
                 "ec3d_set_preconditioner")
        except (EC3DError, ValueError):
            for setter, before in undo:
                setter(before)
            raise

    def set_precond_precision(self, precision: str = "fp64"):
        """Precision of the V-cycle the next set_preconditioner("mg") builds: "fp64" (default) or "fp32" (M in single
        precision, the outer iteration unchanged in fp64; "block-mg" is then refused).  Kept across assemblies and
        set_preconditioner("none"); a hierarchy already set is not rebuilt."""
        if precision not in PRECOND_PRECISION:
            raise ValueError(f"precision must be one of {sorted(PRECOND_PRECISION)}, not {precision!r}")
        _chk(self.L, self.L.ec3d_set_precond_precision(self.h, PRECOND_PRECISION[precision]),
             "ec3d_set_precond_precision")

    def precond_precision(self):
        """(setting, in_use): the handle's setting and the precision of the hierarchy now set ("fp64" without one)."""
        setting, in_use = C.c_int32(0), C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_precond_precision(self.h, C.byref(setting), C.byref(in_use)),
             "ec3d_get_precond_precision")
        name = {v: k for k, v in PRECOND_PRECISION.items()}
        return name[setting.value], name[in_use.value]

    def set_precond_coarsening(self, rule: str = "rediscretize"):
        """Coarsening rule of the hierarchy the next set_preconditioner("mg") builds: "rediscretize" (default: an axis
        halves while it is even and >= 8, other boxes are refused with PRECOND_E_COARSE) or "aggregate" (every axis is
        ceil-halved, levels below the first odd or short one are Galerkin products in band form: every box gets a
        hierarchy).  Kept across assemblies and set_preconditioner("none"); a hierarchy already set is not rebuilt;
        "block-mg" ignores it."""
        if rule not in PRECOND_COARSENING:
            raise ValueError(f"coarsening must be one of {sorted(PRECOND_COARSENING)}, not {rule!r}")
        _chk(self.L, self.L.ec3d_set_precond_coarsening(self.h, PRECOND_COARSENING[rule]),
             "ec3d_set_precond_coarsening")

    def set_precond_grid(self, sdx: int, sdy: int, sdz: int):
        """The matrix set_matrix_csr put on the handle is a 7-point operator on an sdx x sdy x sdz box, rows numbered
        r = i + j sdx + k sdx sdy: set_preconditioner("mg") then builds a hierarchy from it (all coarse levels Galerkin)
        instead of refusing.  Belongs to the matrix: a new matrix or assembly clears it; (0, 0, 0) clears it too.
        EC3DError with .status 2, nothing changed: no matrix from set_matrix_csr, an extent < 2, sdx sdy sdz != n."""
        _chk(self.L, self.L.ec3d_set_precond_grid(self.h, int(sdx), int(sdy), int(sdz)), "ec3d_set_precond_grid")

    def precond_grid(self):
        """(sdx, sdy, sdz) as set_precond_grid left it, or None."""
        dims = np.zeros(3, np.int32)
        _chk(self.L, self.L.ec3d_get_precond_grid(self.h, dims.ctypes.data), "ec3d_get_precond_grid")
        return tuple(int(a) for a in dims) if dims.any() else None

    def set_guess_history(self, depth: int):
        """Start every solve from the projection onto up to `depth` (0 .. 8; 0 = off, the default) earlier solutions of
        this matrix (ec3d_set_guess_history of include/ec3d_hip.h).  The depth stays with the handle; a new matrix,
        place_vectors and a change of the depth drop the stored pairs.  EC3DError with .status 2 for a depth out of
        range, 4 on a z-slab."""
        _chk(self.L, self.L.ec3d_set_guess_history(self.h, int(depth)), "ec3d_set_guess_history")

    def guess_history(self):
        """Of the last solve: dict(depth, stored, used, kept, res_before, res_after, coef) -- pairs held now, pairs the
        projection ran on, 1 / 0 / -1 = the new pair was stored / discarded / the history cleared, ||b - A x|| / ||b||
        in front of and behind the projection, and its `used` coefficients."""
        g = GuessInfo()
        _chk(self.L, self.L.ec3d_get_guess_history(self.h, C.byref(g)), "ec3d_get_guess_history")
        return dict(depth=int(g.depth), stored=int(g.stored), used=int(g.used), kept=int(g.kept),
                    res_before=float(g.res_before), res_after=float(g.res_after),
                    coef=np.array(g.coef[:max(int(g.used), 0)], dtype=np.float64))

    def set_null_projection(self, on: bool = True, null_tol: float = 1e-10, precond: str | None = None, pre: int = 0,
                            post: int = 0, coarse_sweeps: int = 0):
        """Take the left null vectors of the A-V system out of every solve's initial residual, so that tolerances
        below |w.b| / ||w|| ||b|| can be reached (ec3d_set_null_projection of include/ec3d_hip.h).  The first solve on
        a matrix finds one vector per connected conducting component by an adjoint solve to ``null_tol``.  The setting
        stays with the handle, the vectors with the matrix.  EC3DError with .status NULL_E_MATRIX on a Poisson, CSR or
        bands + tail matrix, 4 on a z-slab; the setting is then off.  A solve whose set-up misses ``null_tol`` raises
        with .status NULL_E_SETUP.  ``precond`` ("none", "block-mg" or "block-mg-a"; None leaves the setting as it is):
        the preconditioner of the adjoint solves (ec3d_set_null_precond) -- the transposed block multigrid, or with
        "block-mg-a" the A blocks' hierarchy of A as it stands --, with ``pre`` / ``post`` / ``coarse_sweeps`` sweeps
        (0: the defaults of set_preconditioner).  EC3DError with .status PRECOND_E_MATRIX when the block hierarchy
        refuses the matrix; the setting then stays as it was."""
        if precond is not None:
            _chk(self.L, self.L.ec3d_set_null_precond(self.h, NULL_PRECOND[precond], int(pre), int(post), int(coarse_sweeps)),
                 "ec3d_set_null_precond")
        _chk(self.L, self.L.ec3d_set_null_projection(self.h, 1 if on else 0, float(null_tol)), "ec3d_set_null_projection")

    def null_projection(self):
        """dict(on, built, found, kept, dropped, null_tol, removed, setup_ms, components): components = per conducting
        component (the first 32) dict(seed_row, iterations, residual, kept) -- the U row the adjoint solve was seeded
        with (0-based, the reference's numbering), its iterations, ||A^T w|| / ||w||; removed = ||Q^T R|| / ||b|| of
        the last solve."""
        g = NullInfo()
        _chk(self.L, self.L.ec3d_get_null_projection(self.h, C.byref(g)), "ec3d_get_null_projection")
        comps = [dict(seed_row=int(g.seed_row[i]), iterations=int(g.iterations[i]), residual=float(g.residual[i]),
                      kept=bool(g.was_kept[i])) for i in range(int(g.reported))]
        return dict(on=bool(g.on), built=bool(g.built), found=int(g.found), kept=int(g.kept), dropped=int(g.dropped),
                    null_tol=float(g.null_tol), removed=float(g.removed), setup_ms=float(g.setup_ms), components=comps)

    def null_precond(self):
        """(kind, [(sdx, sdy, sdz) per level, finest first], hierarchy_ms): the preconditioner of the adjoint solves that
        is set, and the hierarchy the last set-up built (no level when none was built) with the time spent building it."""
        kind, levels, ms = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        dims = np.zeros(3 * NULL_PRECOND_MAX_LEVELS, np.int32)
        _chk(self.L, self.L.ec3d_get_null_precond(self.h, C.byref(kind), C.byref(levels), dims.ctypes.data, C.byref(ms)),
             "ec3d_get_null_precond")
        name = {v: k for k, v in NULL_PRECOND.items()}[kind.value]
        return name, [tuple(int(a) for a in dims[3 * l:3 * l + 3]) for l in range(levels.value)], float(ms.value)

    def null_precond_apply(self, r):
        """z = N r on host vectors (the reference's numbering), N the preconditioner of the adjoint solves that is set;
        N is built for the call and released."""
        z = np.empty(self.n)
        _chk(self.L, self.L.ec3d_null_precond_apply(self.h, np.ascontiguousarray(r, np.float64), z), "ec3d_null_precond_apply")
        return z

    def left_null_vector(self, index: int = 0):
        """Kept left null vector ``index`` (unit norm, the reference's numbering); builds the vectors when the
        projection is on and they do not exist yet."""
        w = np.empty(self.n)
        _chk(self.L, self.L.ec3d_left_null_vector(self.h, int(index), w), "ec3d_left_null_vector")
        return w

    def _coarsening_setting(self):
        setting = C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_precond_coarsening(self.h, C.byref(setting), None, None),
             "ec3d_get_precond_coarsening")
        return {v: k for k, v in PRECOND_COARSENING.items()}[setting.value]

    def precond_coarsening(self):
        """(setting, in_use, kinds): the handle's setting, the rule of the hierarchy now set ("rediscretize" without
        one, "aggregate" for "block-mg") and per level of it 0 = the handle's matrix, 1 = rediscretised, 2 = Galerkin."""
        setting, in_use = C.c_int32(0), C.c_int32(0)
        levels = len(self.preconditioner()[1])
        kinds = np.zeros(max(levels, 1), np.int32)
        _chk(self.L, self.L.ec3d_get_precond_coarsening(self.h, C.byref(setting), C.byref(in_use), kinds.ctypes.data),
             "ec3d_get_precond_coarsening")
        name = {v: k for k, v in PRECOND_COARSENING.items()}
        return name[setting.value], name[in_use.value], [int(k) for k in kinds[:levels]]

    def preconditioner(self):
        """(kind, [(sdx, sdy, sdz) per level, finest first])"""
        kind, levels = C.c_int(0), C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_preconditioner(self.h, C.byref(kind), C.byref(levels), None),
             "ec3d_get_preconditioner")
        dims = np.zeros(3 * max(levels.value, 1), np.int32)
        _chk(self.L, self.L.ec3d_get_preconditioner(self.h, C.byref(kind), C.byref(levels), dims.ctypes.data),
             "ec3d_get_preconditioner")
        name = {v: k for k, v in PRECOND.items()}[kind.value]
        return name, [tuple(int(a) for a in dims[3 * l:3 * l + 3]) for l in range(levels.value)]

    def precond_apply(self, r):
        """z = M r on host vectors (the reference's numbering)."""
        z = np.empty(self.n)
        _chk(self.L, self.L.ec3d_precond_apply(self.h, np.ascontiguousarray(r, np.float64), z), "ec3d_precond_apply")
        return z

    # ---- measurement ----------------------------------------------------------------------
    def time_kernel(self, name: str, reps: int = 20) -> float:
        ms = C.c_double(0)
        _chk(self.L, self.L.ec3d_time_kernel(self.h, KERNEL[name], reps, C.byref(ms)), "ec3d_time_kernel")
        return ms.value

    def time_iterations(self, iters: int) -> float:
        ms = C.c_double(0)
        _chk(self.L, self.L.ec3d_time_iterations(self.h, iters, C.byref(ms)), "ec3d_time_iterations")
        return ms.value

    def iterate_begin(self):
        _chk(self.L, self.L.ec3d_iterate_begin(self.h), "ec3d_iterate_begin")

    def iterate(self, first_iter: int, count: int, per_kernel: bool = False):
        """Enqueue `count` iterations (exits disabled).  per_kernel=True: synchronises and returns
        the average duration of K1..K5 in ms (hipEvents on the library's stream)."""
        if not per_kernel:
            _chk(self.L, self.L.ec3d_iterate(self.h, first_iter, count, None), "ec3d_iterate")
            return None
        ms = np.zeros(5)
        _chk(self.L, self.L.ec3d_iterate(self.h, first_iter, count, ms.ctypes.data), "ec3d_iterate")
        return dict(zip(("k1", "k2", "k3", "k4", "k5"), ms.tolist()))

    # ---- multi-rank building blocks (see dist.py) -------------------------------------------
    def set_stream(self, stream_ptr: int | None):
        _chk(self.L, self.L.ec3d_set_stream(self.h, C.c_void_p(stream_ptr or 0)), "ec3d_set_stream")

    def vector_layout(self):
        g, n, npad, halo = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _chk(self.L, self.L.ec3d_vector_layout(self.h, C.byref(g), C.byref(n), C.byref(npad), C.byref(halo)),
             "ec3d_vector_layout")
        return dict(ghost=g.value, n=n.value, n_pad=npad.value, halo=halo.value)

    def adopt_vectors(self, device_ptr: int):
        _chk(self.L, self.L.ec3d_adopt_vectors(self.h, C.c_void_p(device_ptr)), "ec3d_adopt_vectors")

    def dist_configure(self, nranks: int, lsum_ptr: int, gsum_ptr: int):
        _chk(self.L, self.L.ec3d_dist_configure(self.h, nranks, C.c_void_p(lsum_ptr), C.c_void_p(gsum_ptr)),
             "ec3d_dist_configure")

    def dist_step(self, stage: int, it: int = 0, tol: float = 0.0):
        _chk(self.L, self.L.ec3d_dist_step(self.h, stage, it, float(tol)), "ec3d_dist_step")

    def dist_set_boundary_rows(self, ranges):
        """ranges: [(lo, hi)] device rows this rank sends in a halo exchange; enables the K2/K5 split stages."""
        lo = np.ascontiguousarray([r[0] for r in ranges] or [0], np.int64)
        hi = np.ascontiguousarray([r[1] for r in ranges] or [0], np.int64)
        on = C.c_int32(0)
        _chk(self.L, self.L.ec3d_dist_set_boundary_rows(self.h, len(ranges), lo, hi, C.byref(on)),
             "ec3d_dist_set_boundary_rows")
        return bool(on.value)

    def can_overlap(self) -> bool:
        return bool(self.L.ec3d_can_overlap(self.h))

    def read_state_async(self, pinned_int32_ptr: int):
        """Enqueue a copy of the stop flag into pinned host memory (see include/ec3d_hip.h)."""
        _chk(self.L, self.L.ec3d_read_state_async(self.h, C.c_void_p(pinned_int32_ptr)), "ec3d_read_state_async")

    def read_state(self):
        si, sk, bn = C.c_int32(0), C.c_int32(0), C.c_double(0)
        _chk(self.L, self.L.ec3d_read_state(self.h, C.byref(si), C.byref(sk), C.byref(bn)), "ec3d_read_state")
        return si.value, sk.value, bn.value

    def fusion(self):
        """(K2 inside K3, K5 inside the next K1) as 0/1: which launches one iteration of this handle is made of."""
        a, b = C.c_int32(0), C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_fusion(self.h, C.byref(a), C.byref(b)), "ec3d_get_fusion")
        return a.value, b.value

    def x_interval(self) -> int:
        """Iterations between two updates of X (ec3d_get_x_interval): 1, or D when K4 defers the update."""
        d = C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_x_interval(self.h, C.byref(d)), "ec3d_get_x_interval")
        return d.value

    def x_groups(self):
        """(how, launches so far): whether the groups of deferred X updates are applied by launches of their own instead of
        by every D-th K4 -- 0: no; 1: on a second stream beside the iteration; 2: on the iteration's own stream, behind the
        K4 of each group's last iteration (ec3d_get_x_groups)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_x_groups(self.h, C.byref(a), C.byref(b)), "ec3d_get_x_groups")
        return a.value, b.value

    def k4_as_spmv(self) -> bool:
        """K4 computes AS = A*S again instead of reading a stored AS (ec3d_get_k4_form)."""
        d = C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_k4_form(self.h, C.byref(d)), "ec3d_get_k4_form")
        return bool(d.value)

    def band_placement(self):
        """(candidate SpMV times in us, index kept) of the placement probe of plain band streams; ([], -1): none ran."""
        us = np.zeros(16)
        tried, kept = C.c_int32(0), C.c_int32(-1)
        _chk(self.L, self.L.ec3d_get_band_placement(self.h, 16, us.ctypes.data, C.byref(tried), C.byref(kept)),
             "ec3d_get_band_placement")
        return [float(v) for v in us[:tried.value]], kept.value

    def vector_placement(self):
        """(candidate iteration times in us, index kept, search time in ms) of the placement probe of the work vectors
        (ec3d_get_vector_placement); ([], -1, 0.0): none ran."""
        us = np.zeros(16)
        tried, kept, ms = C.c_int32(0), C.c_int32(-1), C.c_double(0.0)
        _chk(self.L, self.L.ec3d_get_vector_placement(self.h, 16, us.ctypes.data, C.byref(tried), C.byref(kept), C.byref(ms)),
             "ec3d_get_vector_placement")
        return [float(v) for v in us[:tried.value]], kept.value, ms.value

    def place_vectors(self, candidates: int = 4):
        """Run the placement search of the work vectors now (ec3d_place_vectors): every vector is zero afterwards."""
        _chk(self.L, self.L.ec3d_place_vectors(self.h, candidates), "ec3d_place_vectors")
        return self.vector_placement()

    def restart_count(self) -> int:
        """Times the restart of src/solvers.f90:47-49 fired in the last solve (counted on the device)."""
        k = C.c_int32(0)
        _chk(self.L, self.L.ec3d_get_restart_count(self.h, C.byref(k)), "ec3d_get_restart_count")
        return k.value

    def synchronize(self):
        _chk(self.L, self.L.ec3d_device_synchronize(self.h), "ec3d_device_synchronize")


class _SlabView(EC3DSolver):
    """A slab of an EC3DMulti as an EC3DSolver for introspection (geometry, info, read_state); the multi
    handle owns it."""

    def __init__(self, L, h):
        self.L, self.h = L, h

    def close(self):
        self.h = C.c_void_p()

    __del__ = close


class EC3DMulti:
    """N GPUs behind one handle (include/ec3d_hip.h section 2c): the library cuts the grid into z-slabs, keeps
    one host thread per slab and moves halo planes and partial sums between the devices itself.  Host vectors
    are in the reference's global numbering.  devices=None: GPUs 0 .. nranks-1 (raises "needs N devices" when
    the machine has fewer); a list may name one GPU several times (several slabs on one card)."""

    def __init__(self, nranks: int, devices=None, dictionary: bool | None = None, structured: bool | None = None):
        self.L = load_library()
        self.h = C.c_void_p()
        dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
        if dev is not None and len(dev) != nranks:
            raise ValueError("devices must name one device per rank")
        _chk(self.L, self.L.ec3d_multi_create(C.byref(self.h), int(nranks), None if dev is None else dev.ctypes.data),
             "ec3d_multi_create")
        self.nranks = int(nranks)
        self.rank = None           # (set on the handle of ONE rank of a one-process-per-GPU job: for_rank)
        if dictionary is not None or structured is not None:
            _chk(self.L, self.L.ec3d_multi_set_format(self.h, -1 if dictionary is None else int(bool(dictionary)),
                                                      -1 if structured is None else int(bool(structured))),
                 "ec3d_multi_set_format")

    @staticmethod
    def rccl_unique_id() -> bytes:
        """A fresh RCCL unique id (128 bytes; ec3d_rccl_unique_id): made on ONE rank, handed to all."""
        L = load_library()
        buf = C.create_string_buffer(128)
        _chk(L, L.ec3d_rccl_unique_id(buf), "ec3d_rccl_unique_id")
        return buf.raw

    @classmethod
    def for_rank(cls, rank: int, world: int, device: int, id_halo: bytes, id_sum: bytes, dictionary: bool | None = None,
                 structured: bool | None = None, rehearse=None):
        """One process per GPU (ec3d_multi_create_rank): this process's slab of a `world`-rank job on `device`, RCCL
        between the ranks, the iteration loop enqueued from C++.  Same methods as the one-process handle; host vectors are
        global on every rank (download / solve fill this rank's planes only).  rehearse=(as_rank, as_world): one rank of
        a larger job on one GPU, its neighbours mapped to itself -- for timing."""
        self = cls.__new__(cls)
        self.L = load_library()
        self.h = C.c_void_p()
        ar, aw = rehearse if rehearse else (-1, 0)
        if len(id_halo) != 128 or len(id_sum) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        _chk(self.L, self.L.ec3d_multi_create_rank(C.byref(self.h), int(rank), int(world), int(device), id_halo, id_sum,
                                                   int(ar), int(aw)), "ec3d_multi_create_rank")
        self.nranks = 1            # LOCAL slabs (slab(0) is this rank's)
        self.rank, self.world = int(rank), int(world)
        if dictionary is not None or structured is not None:
            _chk(self.L, self.L.ec3d_multi_set_format(self.h, -1 if dictionary is None else int(bool(dictionary)),
                                                      -1 if structured is None else int(bool(structured))),
                 "ec3d_multi_set_format")
        return self

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.ec3d_multi_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def assemble_poisson(self, sdx, sdy, sdz, delta=(0.00333, 0.00333, 0.00333), bnd=-0.95):
        BND = np.full(6, float(bnd)) if np.isscalar(bnd) else np.ascontiguousarray(
            np.asarray(bnd, np.float64).T).reshape(-1)
        _chk(self.L, self.L.ec3d_multi_assemble_poisson(self.h, sdx, sdy, sdz, BND,
                                                        np.ascontiguousarray(delta, np.float64)),
             "ec3d_multi_assemble_poisson")

    def assemble(self, geoPHYS, geoPHYS_C, valPHYS, BND, delta, dt):
        """Same arguments as EC3DSolver.assemble (the GLOBAL tables)."""
        sdz, sdy, sdx = geoPHYS.shape
        vp = np.asarray(valPHYS, np.float64)
        _chk(self.L, self.L.ec3d_multi_assemble(
            self.h, sdx, sdy, sdz, np.ascontiguousarray(geoPHYS, np.int8).reshape(-1),
            np.ascontiguousarray(geoPHYS_C, np.int32).reshape(-1),
            np.ascontiguousarray(vp.T).reshape(-1), vp.shape[0],
            np.ascontiguousarray(np.asarray(BND, np.float64).T).reshape(-1),
            np.ascontiguousarray(delta, np.float64), float(dt)), "ec3d_multi_assemble")

    def set_matrix_csr(self, valA, irow, jcol):
        irow = np.ascontiguousarray(irow, np.int32)
        _chk(self.L, self.L.ec3d_multi_set_matrix_csr(self.h, len(irow) - 1, np.ascontiguousarray(valA, np.float64),
                                                      irow, np.ascontiguousarray(jcol, np.int32)),
             "ec3d_multi_set_matrix_csr")

    @property
    def n(self) -> int:
        n = C.c_int64(0)
        _chk(self.L, self.L.ec3d_multi_size(self.h, C.byref(n)), "ec3d_multi_size")
        return n.value

    def slab(self, rank: int):
        """(EC3DSolver view of rank's slab, k0, k1)."""
        h, k0, k1 = C.c_void_p(), C.c_int32(0), C.c_int32(0)
        _chk(self.L, self.L.ec3d_multi_slab(self.h, rank, C.byref(h), C.byref(k0), C.byref(k1)), "ec3d_multi_slab")
        return _SlabView(self.L, h), k0.value, k1.value

    def upload(self, which: str, a):
        a = np.ascontiguousarray(a, np.float64)
        if a.size != self.n:
            raise ValueError(f"expected {self.n} entries (global numbering)")
        _chk(self.L, self.L.ec3d_multi_upload(self.h, VEC[which], a), "ec3d_multi_upload")

    def download(self, which: str):
        a = np.zeros(self.n)
        _chk(self.L, self.L.ec3d_multi_download(self.h, VEC[which], a), "ec3d_multi_download")
        return a

    def solve(self, b, x0, tolerance, itmax):
        """One reference solve (src/solvers.f90:3-50) on all slabs.  Returns (x, iter)."""
        x = np.array(x0, dtype=np.float64, copy=True)
        it = C.c_int32(0)
        _chk(self.L, self.L.ec3d_multi_solve(self.h, np.ascontiguousarray(b, np.float64), x, float(tolerance),
                                             int(itmax), C.byref(it)), "ec3d_multi_solve")
        return x, it.value

    def solve_resident(self, tolerance, itmax, hist_cap: int = 0):
        """Returns (iter, hist) like EC3DSolver.solve_resident; the history is not kept on slabs (empty)."""
        it = C.c_int32(0)
        _chk(self.L, self.L.ec3d_multi_solve_resident(self.h, float(tolerance), int(itmax), C.byref(it)),
             "ec3d_multi_solve_resident")
        return it.value, np.zeros((0, 2))

    def true_residual(self):
        rel, bn = C.c_double(0), C.c_double(0)
        _chk(self.L, self.L.ec3d_multi_true_residual(self.h, C.byref(rel), C.byref(bn)), "ec3d_multi_true_residual")
        return rel.value, bn.value

    def spmv(self, x):
        y = np.zeros(self.n)
        _chk(self.L, self.L.ec3d_multi_spmv(self.h, np.ascontiguousarray(x, np.float64), y), "ec3d_multi_spmv")
        return y

    def rhs_step(self, src_index, src_value, moving: bool = False):
        idx = np.ascontiguousarray(src_index, np.int32)
        val = np.ascontiguousarray(src_value, np.float64)
        _chk(self.L, self.L.ec3d_multi_rhs_step(self.h, int(bool(moving)), len(idx),
                                                idx if len(idx) else np.zeros(1, np.int32),
                                                val if len(val) else np.zeros(1)), "ec3d_multi_rhs_step")

    def post_update(self):
        _chk(self.L, self.L.ec3d_multi_post_update(self.h), "ec3d_multi_post_update")

    def vtk_fields(self, delta, ncells: int, conducting: bool):
        mk = lambda: np.empty((ncells, 3), np.float32)
        fa, fs, fb = mk(), mk(), mk()
        fe = mk() if conducting else None
        _chk(self.L, self.L.ec3d_multi_vtk_fields(self.h, np.ascontiguousarray(delta, np.float64), fa.ctypes.data,
                                                  fe.ctypes.data if conducting else None, fs.ctypes.data,
                                                  fb.ctypes.data), "ec3d_multi_vtk_fields")
        return dict(A=fa, eddy=fe, source=fs, B=fb)

    def vtk_fields_begin(self, delta, big_endian: bool = True) -> int:
        """EC3DSolver.vtk_fields_begin on every slab (ec3d_multi_vtk_fields_begin): nothing waits; returns the slot."""
        slot = C.c_int32(0)
        _chk(self.L, self.L.ec3d_multi_vtk_fields_begin(self.h, np.ascontiguousarray(delta, np.float64), int(big_endian),
                                                        C.byref(slot)), "ec3d_multi_vtk_fields_begin")
        return slot.value

    def vtk_fields_wait(self, slot: int, big_endian: bool = True):
        """dict(A, eddy (None without conductors), source, B); each value is a LIST with one (cells of the slab, 3)
        view per slab, in z order -- together the cells of field_N.vtk in file order (vtk.field_vtk_pieces writes such
        lists part by part; vtk.join_parts makes one array of them).  A slab that holds no conductor contributes
        zeros to eddy.  The views are valid until the third vtk_fields_begin after the one that returned the slot."""
        dt = np.dtype(">f4") if big_endian else np.dtype(np.float32)
        parts = {k: [] for k in ("A", "eddy", "source", "B")}
        at = 0
        for r in range(self.nranks):
            p = [C.POINTER(C.c_float)() for _ in range(4)]
            c0, n = C.c_int64(0), C.c_int64(0)
            _chk(self.L, self.L.ec3d_multi_vtk_fields_wait(self.h, slot, r, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]),
                                                           C.byref(p[3]), C.byref(c0), C.byref(n)),
                 "ec3d_multi_vtk_fields_wait")
            if r == 0 and getattr(self, "rank", None) is not None:
                at = c0.value      # one process per GPU: this rank's slab starts where the ranks below it end
                self.first_cell = at
            if c0.value != at:
                raise EC3DError("ec3d_multi_vtk_fields_wait: the slabs do not tile the grid")
            at += n.value
            for k, q in zip(("A", "eddy", "source", "B"), p):
                parts[k].append(np.ctypeslib.as_array(q, shape=(n.value * 3,)).view(dt).reshape(n.value, 3)
                                if q else None)
        if all(e is None for e in parts["eddy"]):
            parts["eddy"] = None
        else:
            parts["eddy"] = [e if e is not None else np.zeros(a.shape, dt) for e, a in zip(parts["eddy"], parts["A"])]
        return parts

    def iterate_begin(self):
        _chk(self.L, self.L.ec3d_multi_iterate_begin(self.h), "ec3d_multi_iterate_begin")

    def iterate(self, first_iter: int, count: int, per_kernel: bool = False):
        if not per_kernel:
            _chk(self.L, self.L.ec3d_multi_iterate(self.h, first_iter, count, None), "ec3d_multi_iterate")
            return None
        ms = np.zeros(5)
        _chk(self.L, self.L.ec3d_multi_iterate(self.h, first_iter, count, ms.ctypes.data), "ec3d_multi_iterate")
        return dict(zip(("k1", "k2", "k3", "k4", "k5"), ms.tolist()))

    def synchronize(self):
        _chk(self.L, self.L.ec3d_multi_synchronize(self.h), "ec3d_multi_synchronize")

    def plan(self):
        """(plan, x_every): the schedule the job runs (ec3d_multi_plan): 0 five launches, 1 K1 / K3 interior + boundary,
        2 K2 / K5 boundary first, 3 three launches per iteration; iterations between two X updates."""
        pl, xe = C.c_int32(0), C.c_int32(0)
        _chk(self.L, self.L.ec3d_multi_plan(self.h, C.byref(pl), C.byref(xe)), "ec3d_multi_plan")
        return pl.value, xe.value

    def halo_rows(self, rank: int = 0):
        """(sent, received): rows local slab `rank` moves in ONE halo exchange of a vector (ec3d_multi_halo_rows)."""
        a, b = C.c_int64(0), C.c_int64(0)
        _chk(self.L, self.L.ec3d_multi_halo_rows(self.h, int(rank), C.byref(a), C.byref(b)), "ec3d_multi_halo_rows")
        return a.value, b.value

    def iterate_timed(self, first_iter: int, count: int, rank: int = 0):
        """The instrumented pass with the synchronisation points bracketed too (ec3d_multi_iterate_timed): ({stage: ms},
        {"reduction_points": (ms per iteration, points per iteration), "halo_waits": (...)}) for local slab `rank`."""
        ms = np.zeros(5)
        sm = np.zeros(2)
        sn = np.zeros(2, np.int32)
        _chk(self.L, self.L.ec3d_multi_iterate_timed(self.h, first_iter, count, rank, ms.ctypes.data, sm.ctypes.data,
                                                     sn.ctypes.data), "ec3d_multi_iterate_timed")
        return ({f"k{i + 1}": float(ms[i]) for i in range(5)},
                {"reduction_points": (float(sm[0]), int(sn[0])), "halo_waits": (float(sm[1]), int(sn[1]))})

    def rccl_info(self):
        """(ranks of the communicator as RCCL counts them, RCCL version, file of the library) of a for_rank handle."""
        n, v = C.c_int32(0), C.c_int32(0)
        buf = C.create_string_buffer(512)
        _chk(self.L, self.L.ec3d_multi_rccl_info(self.h, C.byref(n), C.byref(v), buf, 512), "ec3d_multi_rccl_info")
        return n.value, v.value, buf.value.decode()

    def api_calls(self, rank: int) -> float:
        """HIP runtime calls per iteration rank `rank`'s host thread issued in the last iterate()."""
        v = C.c_double(0.0)
        _chk(self.L, self.L.ec3d_multi_api_calls(self.h, rank, C.byref(v)), "ec3d_multi_api_calls")
        return v.value
