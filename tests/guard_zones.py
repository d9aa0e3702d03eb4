"""Helpers for tests/test_gpu_memory_contract.py: look at the memory around and between the rows of the work vectors.

Every work vector is [ghost | n_pad | ghost] doubles (csrc/ec3d_context.hip, ec3d_prepare_vectors).  The kernels store to
rows [0, n) only; the ghosts and rows [n, n_pad) are read and have to stay zero.  In the structured A-V form some rows below
n belong to no unknown -- the rows between two xy planes when a plane starts on a tile boundary, and the slots of the
grid-shaped U block that hold no conducting cell -- and have to stay zero as well.

    adopted(E, build, margin)   a handle that works on a torch tensor, with a NaN canary before and behind the eight vectors
                                (mark_padding: a finite mark in rows [n, n_pad), so that a stray store of +0.0 shows too)
    zones(layout, pitch_info)   index arrays into ONE vector's [ghost | n_pad | ghost]
    peek(ptr, count)            doubles of library-owned device memory, through hipMemcpy of the process's HIP runtime
    owned_block / rings         the eight vectors / the ring buffers of a handle that owns its vectors
    findings / assert_clean     what is not zero BYTES in the zones (a -0.0 counts), what is not the canary in the margins

No test lives here (the name does not start with test_)."""
import contextlib
import ctypes as C
import os

import numpy as np

CANARY = 0x7FF8C0DE5AFE0001        # a quiet NaN no computation produces: exponent all ones, quiet bit, a payload
MARK = 0x3FF0000000000000          # 1.0: a finite mark for rows [n, n_pad), which no kernel stores to
NVEC = 8
NAMES = ("X", "B", "R", "R0", "P", "AP", "S", "AS")


def round_up(a, m):
    return (a + m - 1) // m * m


# ---- adopted vectors ------------------------------------------------------------------------------------------------
class Adopted:
    """s: the handle; store: margin + 8 * len + margin doubles of torch memory, the library works on the middle part."""

    def __init__(self, E, build, margin=None, device=0, mark_padding=False, **handle_args):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.s = E.EC3DSolver(device=device, **handle_args)
        try:
            self.s.set_stream(self.stream.cuda_stream)           # stream order as in dist.py (HipSlabOps)
            build(self.s)
            self.layout = lay = self.s.vector_layout()
            self.len = 2 * lay["ghost"] + lay["n_pad"]
            self.margin = round_up(self.len, 64) if margin is None else int(margin)
            # a multiple of 64 doubles keeps the 512-byte alignment the library's own allocation has
            assert self.margin % 64 == 0 and self.margin >= self.len
            with torch.cuda.stream(self.stream):
                self.store = torch.zeros(2 * self.margin + NVEC * self.len, dtype=torch.float64, device=self.device)
                bits = self.store.view(torch.int64)
                bits[:self.margin] = CANARY
                bits[self.margin + NVEC * self.len:] = CANARY
                if mark_padding:
                    rows = bits[self.margin:self.margin + NVEC * self.len].view(NVEC, self.len)
                    rows[:, lay["ghost"] + lay["n"]:lay["ghost"] + lay["n_pad"]] = MARK
            self.marked = bool(mark_padding)
            self.stream.synchronize()
            assert self.store.data_ptr() % 512 == 0
            self.s.adopt_vectors(self.store.data_ptr() + 8 * self.margin)
        except BaseException:
            self.close()
            raise

    def read(self):
        """(lower margin, the eight vectors as [8, len], upper margin) as uint64 bit patterns, after everything enqueued."""
        self.s.synchronize()
        self.stream.synchronize()
        with self.torch.cuda.stream(self.stream):
            host = self.store.cpu()
        bits = host.numpy().view(np.uint64)
        m, k = self.margin, NVEC * self.len
        return bits[:m], bits[m:m + k].reshape(NVEC, self.len), bits[m + k:]

    def close(self):
        """Detach the library from the torch-owned stream and vectors BEFORE torch frees them (SlabSolver.close)."""
        s = getattr(self, "s", None)
        if s is not None and getattr(s, "h", None) and s.h.value:
            try:
                self.stream.synchronize()
                s.set_stream(None)
            finally:
                s.close()
        self.s = None
        self.store = None


@contextlib.contextmanager
def adopted(E, build, margin=None, mark_padding=False, **handle_args):
    a = Adopted(E, build, margin, mark_padding=mark_padding, **handle_args)
    try:
        yield a
    finally:
        a.close()


# ---- zones ----------------------------------------------------------------------------------------------------------
def pitch_info(s, plane_cells):
    """What a structured A-V handle reports about its rows: dict(plane, pitch, block, hidden), or None for any other form.
    plane: cells of an xy plane (the caller's grid); pitch: rows from one plane to the next (the handle's largest band
    offset, ec3d_get_matrix_info); block: rows of a component block; hidden: device rows below n that no unknown of the
    reference's numbering lives in (ec3d_get_row_map) -- the rows between planes and the empty slots of the U block."""
    lay, mi = s.vector_layout(), s.info
    if lay["n"] == mi.n:            # device rows == reference unknowns: bands + tail, or a single-component grid
        return None
    pitch = int(mi.band_offset[mi.nbands - 1])
    assert mi.nbands == 7 and pitch >= plane_cells and lay["n"] % (4 * pitch) == 0
    assert pitch == plane_cells or pitch == round_up(plane_cells, 512)
    hidden = np.setdiff1d(np.arange(lay["n"], dtype=np.int64), s.row_map().astype(np.int64))
    return dict(plane=int(plane_cells), pitch=pitch, block=lay["n"] // 4, hidden=hidden)


def zones(layout, pitch_info=None):
    """{name: indices into one vector's [ghost | n_pad | ghost]} of everything no kernel may leave a mark in."""
    g, n, n_pad = layout["ghost"], layout["n"], layout["n_pad"]
    z = {"lower ghost": np.arange(0, g, dtype=np.int64),
         "rows n..n_pad": np.arange(g + n, g + n_pad, dtype=np.int64),
         "upper ghost": np.arange(g + n_pad, g + n_pad + g, dtype=np.int64)}
    if pitch_info is not None:
        r = np.arange(n, dtype=np.int64)
        gap = r[r % pitch_info["pitch"] >= pitch_info["plane"]]
        assert np.all(np.isin(gap, pitch_info["hidden"]))
        z["rows between planes"] = g + gap
        z["empty U slots"] = g + np.setdiff1d(pitch_info["hidden"], gap)
    return z


# ---- library-owned memory -------------------------------------------------------------------------------------------
_hip = None


def _runtime():
    """The HIP runtime this process already holds: the one PyTorch bundles, which the library shares
    (solver._share_hip_runtime_with_torch); opening the same file again gives the same runtime."""
    global _hip
    if _hip is None:
        from eddy_currents_3d_amd import solver
        solver.load_library()
        path = solver.torch_hip_runtime()
        assert path and os.environ.get("EC3D_HIP_RUNTIME") != "system"
        _hip = C.CDLL(path)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    return _hip


def peek(ptr, count):
    """count doubles at device address ptr, as uint64 bit patterns.  The caller has synchronised the handle."""
    out = np.empty(int(count), np.uint64)
    rc = _runtime().hipMemcpy(out.ctypes.data, C.c_void_p(int(ptr)), out.nbytes, 2)      # hipMemcpyDeviceToHost
    assert rc == 0, f"hipMemcpy: {rc}"
    return out


def poke(ptr, values):
    """peek's counterpart (the teeth of the tests: a mark put INSIDE the handle's own block)."""
    v = np.ascontiguousarray(values, np.float64)
    rc = _runtime().hipMemcpy(C.c_void_p(int(ptr)), v.ctypes.data, v.nbytes, 1)          # hipMemcpyHostToDevice
    assert rc == 0, f"hipMemcpy: {rc}"


def owned_block(s):
    """(address of the block, the eight vectors of a handle that owns them as [8, len] bit patterns)."""
    s.synchronize()
    lay = s.vector_layout()
    ln = 2 * lay["ghost"] + lay["n_pad"]
    base = s.device_vector("X")[0] - 8 * lay["ghost"]
    return base, peek(base, NVEC * ln).reshape(NVEC, ln)


def rings(s):
    """{name: [ghost | n_pad | ghost] bit patterns} of the ring buffers the handle hands out NOW as P, AP and S: those that
    lie outside the block of the eight vectors (ec3d_spare_pair lays each out like a vector)."""
    s.synchronize()
    lay = s.vector_layout()
    ln = 2 * lay["ghost"] + lay["n_pad"]
    base = s.device_vector("X")[0] - 8 * lay["ghost"]
    out = {}
    for name in ("P", "AP", "S"):
        p = s.device_vector(name)[0]
        if not base <= p < base + 8 * NVEC * ln:
            out[f"ring {name} @{p:#x}"] = peek(p - 8 * lay["ghost"], ln)
    return out


# ---- the check ------------------------------------------------------------------------------------------------------
def _describe(bits):
    return f"{bits:#018x} ({np.array([bits], np.uint64).view(np.float64)[0]!r})"


def findings(vectors, z, names=NAMES):
    """One line per (vector, zone) that holds a byte other than zero."""
    out = []
    for v, name in zip(vectors, names):
        for zone, idx in z.items():
            bad = idx[v[idx] != 0]
            if len(bad):
                out.append(f"{name}: {zone}: {len(bad)} of {len(idx)} not zero bytes, first at vector index {int(bad[0])}"
                           f" (row {int(bad[0]) - int(z['lower ghost'].size)}): {_describe(int(v[bad[0]]))}")
    return out


def assert_clean(target, z, where=""):
    """target: an Adopted (margins and block), or a handle that owns its vectors (block and current ring buffers)."""
    if isinstance(target, Adopted):
        lo, vec, hi = target.read()
        found = [f"{side} margin: {int((m != CANARY).sum())} doubles overwritten, first at {int(np.flatnonzero(m != CANARY)[0])}: "
                 f"{_describe(int(m[np.flatnonzero(m != CANARY)[0]]))}"
                 for side, m in (("lower", lo), ("upper", hi)) if np.any(m != CANARY)]
        if target.marked:        # rows [n, n_pad) hold the mark instead of zeros: intact, bit for bit
            pad = z["rows n..n_pad"]
            z = {k: v for k, v in z.items() if k != "rows n..n_pad"}
            for v, name in zip(vec, NAMES):
                bad = pad[v[pad] != MARK]
                if len(bad):
                    found.append(f"{name}: rows n..n_pad: {len(bad)} of {len(pad)} marks overwritten, first at row "
                                 f"{int(bad[0]) - int(z['lower ghost'].size)}: {_describe(int(v[bad[0]]))}")
        found += findings(vec, z)
    else:
        found = findings(owned_block(target)[1], z)
        for name, buf in rings(target).items():
            found += findings([buf], z, names=(name,))
    assert not found, where + ":\n  " + "\n  ".join(found)
