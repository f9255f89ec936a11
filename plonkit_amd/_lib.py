"""ctypes binding of include/plonkit_amd.h (lib/libplonkit_amd.so).

Arrays cross as numpy uint64 ([n,4] Fr Montgomery, [n,8] G1 affine, [12] Jacobian) or as raw device
pointers (ints / torch tensors).  Nothing here computes: every function forwards to the C ABI, and
a missing library or a missing GPU raises — there is no Python or CPU fallback.
"""
import collections
import ctypes
import sys
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "lib", "libplonkit_amd.so")
_lib = None

ERR_NAMES = {1: "PLK_ERR_ARG", 2: "PLK_ERR_SIZE", 3: "PLK_ERR_SRS", 4: "PLK_ERR_HIP", 5: "PLK_ERR_UNSAT",
             6: "PLK_ERR_FORMAT", 7: "PLK_ERR_IO"}


class PlkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, code), msg))
        self.code = code


def lib_path():
    return _SO


def lib():
    """Loads the shared library; raises loudly if it has not been built (python -m plonkit_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError("plonkit_amd: %s is missing — build it with `python -m plonkit_amd.build` "
                              "(hipcc, gfx950). There is no fallback implementation." % _SO)
        # PyTorch-ROCm ships its own libamdhip64; if /opt/rocm's copy (our DT_NEEDED) is mapped first, torch's
        # later HIP initialisation finds "No HIP GPUs".  Import torch first so that one runtime serves both.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(_SO)
        L.plk_last_error.restype = ctypes.c_char_p
        L.plk_version.restype = ctypes.c_char_p
        L.plk_srs_size.restype = ctypes.c_uint64
        if hasattr(L, "plk_key_chunk_points"):
            L.plk_key_chunk_points.restype = ctypes.c_uint64
        if hasattr(L, "plk_setup_domain_size"):
            L.plk_setup_domain_size.restype = ctypes.c_uint64
        L.plk_r1cs_num_constraints.restype = ctypes.c_uint64
        L.plk_r1cs_num_variables.restype = ctypes.c_uint64
        L.plk_r1cs_long_lc_terms.restype = ctypes.c_uint32
        L.plk_vkset_keys.restype = ctypes.c_uint32
        L.plk_vkset_tables.restype = ctypes.c_uint32
        L.plk_vkset_keys.argtypes = L.plk_vkset_tables.argtypes = L.plk_vkset_free.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def last_error():
    return lib().plk_last_error().decode()


def _check(rc):
    if rc != 0:
        raise PlkError(rc, last_error())


def have_gpu():
    return lib().plk_device_count() > 0


def _np(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _fr_vectors(arrays, who, allow_empty=False):
    """numpy (len, 4) uint64 Montgomery vectors of one common length, C-contiguous; anything else raises ValueError"""
    out = []
    for i, a in enumerate(arrays):
        if a is None:
            raise ValueError("%s: vector %d is None" % (who, i))
        v = np.asarray(a)
        if v.dtype != np.uint64 or v.ndim != 2 or v.shape[1] != 4:
            raise ValueError("%s: vector %d must be a (len, 4) uint64 array of Montgomery Fr, got %s %s" % (who, i, v.dtype, v.shape))
        if v.shape[0] != np.asarray(arrays[0]).shape[0]:
            raise ValueError("%s: vectors of different lengths (%d and %d)" % (who, np.asarray(arrays[0]).shape[0], v.shape[0]))
        if v.shape[0] == 0 and not allow_empty:
            raise ValueError("%s: vector %d is empty" % (who, i))
        out.append(np.ascontiguousarray(v))
    return out


def _devptr(x):
    """torch tensor / int -> void*"""
    if hasattr(x, "data_ptr"):
        return ctypes.c_void_p(x.data_ptr())
    return ctypes.c_void_p(int(x))


def _stream(s):
    if s is None:
        return ctypes.c_void_p(0)
    if hasattr(s, "cuda_stream"):
        return ctypes.c_void_p(s.cuda_stream)
    return ctypes.c_void_p(int(s))


MSM_PATHS = ("empty", "naive", "short", "short_fallback", "ordinary")      # PLK_MSM_PATH_*


class MsmShape(ctypes.Structure):
    """plk_msm_shape (include/plonkit_amd.h)"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("path", "batch", "table_copies", "window_bits", "windows", "bucket_sets", "fine_bits", "coarse_bins",
                                               "accumulate_variant", "prephase", "reduce_lanes", "pieces")] + [("piece_terms", ctypes.c_uint64)]


COPY_OK, COPY_NOT_A_LABEL, COPY_NOT_BIJECTIVE, COPY_BROKEN = 0, 1, 2, 3      # PLK_COPY_*

# the verdict of the copy-constraint checks: cell = (col, row) of the lowest offender (None for COPY_OK), image = the cell sigma sends it
# to (COPY_BROKEN only)
CopyReport = collections.namedtuple("CopyReport", "kind cell image")


class _CopyReportStruct(ctypes.Structure):
    """plk_copy_report (include/plonkit_amd.h)"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("kind", "col", "row", "col2", "row2")]

    def report(self):
        return CopyReport(int(self.kind), (int(self.col), int(self.row)) if self.kind != COPY_OK else None,
                          (int(self.col2), int(self.row2)) if self.kind == COPY_BROKEN else None)


TRANSCRIPT_CONCURRENT = 1                                             # PLK_TRANSCRIPT_CONCURRENT (never set by the Python tables)


class TranscriptOps:
    """A Fiat-Shamir transcript of the caller's (plk_transcript_ops): subclass it and override begin().  begin() returns a fresh
    transcript object with absorb_fr(bytes32), absorb_g1(bytes64) and challenge() -> bytes32; the bytes are the ABI's in-memory
    elements (4 / 8 little-endian u64 limbs, Montgomery form; the point at infinity is 64 zero bytes).  If that object has an
    end() method it is called once when the library is done with it, on every way out.  The call order is prove_by_steps's
    (include/plonkit_amd.h).  An exception raised in any of them ends the library call and is re-raised from the
    Python call that made it."""

    def begin(self):
        raise NotImplementedError("TranscriptOps.begin")


class _TranscriptOpsStruct(ctypes.Structure):
    """plk_transcript_ops (include/plonkit_amd.h)"""
    _BEGIN = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    _ABSORB = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p)
    _END = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)
    _fields_ = [("user", ctypes.c_void_p), ("begin", _BEGIN), ("absorb_fr", _ABSORB), ("absorb_g1", _ABSORB), ("challenge", _ABSORB),
                ("end", _END), ("flags", ctypes.c_uint32)]


class _TranscriptTable:
    """The ctypes trampolines around a TranscriptOps object.  Whoever hands `.struct` to the library keeps this object alive for as
    long as the library may call back.  An exception inside a callback is caught here (it cannot cross the C frames), makes the
    callback return nonzero, and is raised again by reraise() once the C call is back."""

    def __init__(self, obj):
        if not callable(getattr(obj, "begin", None)):
            raise TypeError("a transcript must have a begin() method (see TranscriptOps), got %r" % (obj,))
        self.obj = obj
        self.error = None
        self._live = {}                                               # state handle -> the object begin() returned
        self._next = 1
        S = _TranscriptOpsStruct
        self._keep = (S._BEGIN(self._begin), S._ABSORB(self._absorb_fr), S._ABSORB(self._absorb_g1), S._ABSORB(self._challenge), S._END(self._end))
        self.struct = S(None, *self._keep, 0)

    def _guard(self, fn):
        try:
            fn()
            return 0
        except BaseException as e:                                    # noqa: B902 — nothing may unwind into the C frames
            if self.error is None:
                self.error = e
            return -1

    def _begin(self, user, state_out):
        def run():
            t = self.obj.begin()
            handle, self._next = self._next, self._next + 1
            self._live[handle] = t
            state_out[0] = handle
        return self._guard(run)

    def _absorb_fr(self, state, ptr):
        return self._guard(lambda: self._live[state].absorb_fr(ctypes.string_at(ptr, 32)))

    def _absorb_g1(self, state, ptr):
        return self._guard(lambda: self._live[state].absorb_g1(ctypes.string_at(ptr, 64)))

    def _challenge(self, state, out):
        def run():
            c = bytes(self._live[state].challenge())
            if len(c) != 32:
                raise ValueError("a transcript's challenge() must return 32 bytes, got %d" % len(c))
            ctypes.memmove(out, c, 32)
        return self._guard(run)

    def _end(self, user, state):
        t = self._live.pop(state, None)
        if callable(getattr(t, "end", None)):
            self._guard(t.end)

    def reraise(self):
        e, self.error = self.error, None
        if e is not None:
            raise e


def _table_of(transcript):
    return None if transcript is None else _TranscriptTable(transcript)


def _finish(rc, table):
    """the end of a C call that took a transcript table: the callback's own exception first, then the library's error"""
    if table is not None:
        table.reraise()
    _check(rc)


class Context:
    """plk_ctx: one GPU.  Mirrors where the reference builds `Worker::new()` (src/plonk.rs:41,47,183)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().plk_create(ctypes.c_int32(device), ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            lib().plk_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().plk_synchronize(self._h))

    def set_transcript(self, transcript):
        """plk_ctx_set_transcript: every proof of this context takes its challenges from `transcript` (a TranscriptOps; None: the
        built-in Keccak transcript again).  The trampolines live as long as the context holds them."""
        table = _table_of(transcript)
        _check(lib().plk_ctx_set_transcript(self._h, ctypes.byref(table.struct) if table is not None else None))
        self._transcript = table

    def _finish_prove(self, rc):
        _finish(rc, getattr(self, "_transcript", None))

    # ---- SRS
    def srs_upload(self, bases):
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        assert bases.ndim == 2 and bases.shape[1] == 8
        _check(lib().plk_srs_upload(self._h, _np(bases), ctypes.c_uint64(bases.shape[0])))

    def srs_set_dev(self, ptr, n):
        _check(lib().plk_srs_set_dev(self._h, _devptr(ptr), ctypes.c_uint64(n)))

    def srs_size(self):
        return lib().plk_srs_size(self._h)

    # multi-GPU commitments of the prover: this rank's SRS slice starts at global index `first_index`; `combine`
    # receives a writable uint64[count, 12] array of Jacobian partial sums and must replace it by the all-ranks sums
    def set_commit_shard(self, first_index, combine):
        if combine is None:
            self._combine_cb = None
            _check(lib().plk_set_commit_shard(self._h, ctypes.c_uint64(0), None, None))
            return
        proto = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32)

        def trampoline(_user, ptr, count):
            try:
                combine(np.ctypeslib.as_array(ptr, shape=(count, 12)))
                return 0
            except Exception as exc:                                  # never let an exception cross the C boundary
                sys.stderr.write("commit combiner failed: %r\n" % (exc,))
                return 4
        self._combine_cb = proto(trampoline)                          # keep the callback object alive
        _check(lib().plk_set_commit_shard(self._h, ctypes.c_uint64(first_index), self._combine_cb, None))

    # the same exchange built into the library (comm.cpp): RCCL all-gather + host EC sum, no Python in the loop
    def comm_init(self, rank, world, unique_id, first_index):
        assert len(unique_id) == 128
        _check(lib().plk_comm_init(self._h, ctypes.c_int32(rank), ctypes.c_int32(world), bytes(unique_id), ctypes.c_uint64(first_index)))

    def comm_init_tcp(self, rank, world, port, first_index):
        _check(lib().plk_comm_init_tcp(self._h, ctypes.c_int32(rank), ctypes.c_int32(world), ctypes.c_uint16(port), ctypes.c_uint64(first_index)))

    def comm_set_mode(self, mode):
        """"replicate" (every rank proves, commitments split) or "scatter" (owner computes: rank 0 proves, the others comm_serve); every
        rank of the communicator must choose the same"""
        _check(lib().plk_comm_set_mode(self._h, ctypes.c_int32({"replicate": 0, "scatter": 1}[mode])))

    def comm_serve(self):
        """worker ranks of a scatter-mode communicator: commit what the owner sends until it calls comm_stop_workers; returns the batches served"""
        n = ctypes.c_uint64(0)
        _check(lib().plk_comm_serve(self._h, ctypes.byref(n)))
        return int(n.value)

    def comm_stop_workers(self):
        _check(lib().plk_comm_stop_workers(self._h))

    def comm_set_shard(self, first_index):
        _check(lib().plk_comm_set_shard(self._h, ctypes.c_uint64(first_index)))

    def msm_finish_sharded(self):
        """finish + the built-in exchange: affine commitment over all ranks' shards"""
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().plk_msm_g1_finish_sharded(self._h, _np(out)))
        return out

    def comm_selftest(self):
        """header broadcast + one grouped ring step over the RCCL communicator, checked byte by byte (every rank calls it)"""
        _check(lib().plk_comm_selftest(self._h))

    def comm_scatter_selftest(self, log_n, iterations):
        """the scatter step of owner-computes mode through the real RCCL branch on one GPU (one-rank communicator, rank 0 receiving its own
        share), the scalars still being written when the step is called; returns the number of iterations whose commitment differs (0 = pass)"""
        bad = ctypes.c_uint32(0)
        _check(lib().plk_comm_scatter_selftest(self._h, ctypes.c_uint32(log_n), ctypes.c_uint32(iterations), ctypes.byref(bad)))
        return bad.value

    def comm_nccl_count(self):
        """ranks RCCL itself counts in this context's communicator (ncclCommCount); 0 without an RCCL communicator"""
        k = ctypes.c_int32(0)
        _check(lib().plk_comm_nccl_count(self._h, ctypes.byref(k)))
        return k.value

    def comm_destroy(self):
        _check(lib().plk_comm_destroy(self._h))

    def comm_info(self):
        r, w, x = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_uint64(0)
        _check(lib().plk_comm_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(x)))
        return r.value, w.value, x.value

    # Lagrange-form key (`prove -l`): second resident SRS used by prove() for commit_using_values
    def srs_lagrange_upload(self, bases):
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        assert bases.ndim == 2 and bases.shape[1] == 8
        _check(lib().plk_srs_lagrange_upload(self._h, _np(bases), ctypes.c_uint64(bases.shape[0])))

    def srs_lagrange_set_dev(self, ptr, n):
        _check(lib().plk_srs_lagrange_set_dev(self._h, _devptr(ptr), ctypes.c_uint64(n)))

    def srs_lagrange_clear(self):
        _check(lib().plk_srs_lagrange_clear(self._h))

    def srs_lagrange_size(self):
        return lib().plk_srs_lagrange_size(self._h)

    def srs_generate(self, n, start=0, tau=42):
        """Crs::crs_42 on the GPU (src/plonk.rs:30-48): resident SRS <- tau^(start+i) * G."""
        _check(lib().plk_srs_generate(self._h, ctypes.c_uint64(n), ctypes.c_uint64(start), ctypes.c_uint32(tau)))

    def srs_generate_fr(self, n, start, tau_mont):
        t = np.ascontiguousarray(tau_mont, dtype=np.uint64)
        _check(lib().plk_srs_generate_fr(self._h, ctypes.c_uint64(n), ctypes.c_uint64(start), _np(t)))

    def srs_precompute(self):
        """builds the MSM's fixed-base table of the resident key(s) now instead of at the first commitment"""
        _check(lib().plk_srs_precompute(self._h))

    def share_srs_from(self, owner):
        """borrow `owner`'s resident key(s) and MSM fixed-base table(s) (same device): a second context for proofs in flight
        beside `owner`'s costs workspace only.  `owner` must outlive this context's use of the key."""
        _check(lib().plk_ctx_share_srs(self._h, owner._h))
        self._srs_owner = owner                                       # keep the lender alive

    def srs_download(self, offset, n):
        out = np.zeros((n, 8), dtype=np.uint64)
        _check(lib().plk_srs_download(self._h, ctypes.c_uint64(offset), ctypes.c_uint64(n), _np(out)))
        return out

    # ---- key files on the GPU (Crs::read / Crs::write): the points are decoded, checked and encoded by kernels
    def srs_load_key(self, data, first=0, count=0, lagrange=False):
        """key-file bytes -> resident key (points [first, first + count) of it; count = 0: all from `first`); every point of the
        file is checked.  Returns (points in the file, the 256 G2 bytes).  A refused point raises PlkError with `.bad_index` = the
        lowest refused index, and the resident key stays what it was."""
        buf = np.frombuffer(data, dtype=np.uint8)                     # bytes, bytearray, memoryview, uint8 array: no copy
        n, bad, g2 = ctypes.c_uint64(0), ctypes.c_uint64(0), np.zeros(256, dtype=np.uint8)
        rc = lib().plk_srs_load_key(self._h, _np(buf), ctypes.c_uint64(buf.size), ctypes.c_uint64(first), ctypes.c_uint64(count),
                                    ctypes.c_uint32(1 if lagrange else 0), ctypes.byref(n), _np(g2), ctypes.byref(bad))
        if rc != 0:
            e = PlkError(rc, last_error())
            e.bad_index = bad.value if bad.value != 2**64 - 1 else None
            raise e
        return n.value, g2.tobytes()

    def srs_store_key(self, g2_bytes, lagrange=False):
        """the resident key (or the Lagrange-form one) as key-file bytes"""
        g2 = np.frombuffer(bytes(g2_bytes), dtype=np.uint8)
        assert g2.shape == (256,)
        flags, n = ctypes.c_uint32(1 if lagrange else 0), ctypes.c_uint64(0)
        _check(lib().plk_srs_store_key(self._h, flags, _np(g2), None, ctypes.c_uint64(0), ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        _check(lib().plk_srs_store_key(self._h, flags, _np(g2), _np(out), ctypes.c_uint64(n.value), ctypes.byref(n)))
        return out.tobytes()

    def g1_decode_dev(self, bytes_ptr, n, points_ptr, stream=None):
        """n x 64 file bytes -> n x G1 affine on the device; raises PlkError (`.bad_index`) if a point is refused"""
        bad = ctypes.c_uint64(0)
        rc = lib().plk_g1_decode_dev(self._h, _devptr(bytes_ptr), ctypes.c_uint64(n), _devptr(points_ptr), ctypes.byref(bad), _stream(stream))
        if rc != 0:
            e = PlkError(rc, last_error())
            e.bad_index = bad.value if bad.value != 2**64 - 1 else None
            raise e

    def g1_encode_dev(self, points_ptr, n, bytes_ptr, stream=None):
        _check(lib().plk_g1_encode_dev(self._h, _devptr(points_ptr), ctypes.c_uint64(n), _devptr(bytes_ptr), _stream(stream)))

    # ---- witness files on the GPU (wtnsio.hip): field elements to and from their 32 little-endian file bytes
    @staticmethod
    def _raise_with_bad_index(rc, bad):
        e = PlkError(rc, last_error())
        e.bad_index = bad.value if bad.value != 2**64 - 1 else None
        raise e

    def fr_decode_dev(self, bytes_ptr, n, fr_ptr, stream=None):
        """n x 32 little-endian canonical bytes -> n Montgomery Fr on the device; raises PlkError (`.bad_index` = the lowest element
        >= r; zero is stored there) if an element is refused"""
        bad = ctypes.c_uint64(0)
        rc = lib().plk_fr_decode_dev(self._h, _devptr(bytes_ptr), ctypes.c_uint64(n), _devptr(fr_ptr), ctypes.byref(bad), _stream(stream))
        if rc != 0:
            self._raise_with_bad_index(rc, bad)

    def fr_encode_dev(self, fr_ptr, n, bytes_ptr, stream=None):
        _check(lib().plk_fr_encode_dev(self._h, _devptr(fr_ptr), ctypes.c_uint64(n), _devptr(bytes_ptr), _stream(stream)))

    def wtns_decode(self, data, out_ptr, cap, stream=None):
        """.wtns file bytes -> Montgomery Fr at `out_ptr` (room for `cap` elements; None: only count).  Returns (n, bad): the elements in
        the file and None; a malformed container or an element >= r raises PlkError, the latter with `.bad_index` = the lowest such element."""
        buf = np.frombuffer(data, dtype=np.uint8)                     # bytes, bytearray, memoryview, uint8 array: no copy
        n, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib().plk_wtns_decode(self._h, _np(buf), ctypes.c_uint64(buf.size), _devptr(out_ptr) if out_ptr is not None else None,
                                   ctypes.c_uint64(cap), ctypes.byref(n), ctypes.byref(bad), _stream(stream))
        if rc != 0:
            self._raise_with_bad_index(rc, bad)
        return n.value, None

    def srs_lagrange_from_powers(self, log_n):
        """Crs::<Lagrange>::from_powers on the device: G1 iNTT of the first 2^log_n resident points -> the Lagrange-form key"""
        _check(lib().plk_srs_lagrange_from_powers(self._h, ctypes.c_uint32(log_n)))

    # ---- structure checks of the resident key(s) (keycheck.hip; the reference has no counterpart: Crs::read checks the curve equation only)
    @staticmethod
    def _seed(seed):
        if seed is None:
            return None
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("seed must be 32 bytes, got %d" % len(seed))
        return seed

    def srs_check(self, g2_bytes, seed=None, locate=False):
        """are the resident monomial points P_0, tau P_0, tau^2 P_0, ... for the tau of the key file's G2 section `g2_bytes` (256 bytes)?
        One random linear combination (rho from `seed`, 32 bytes; None: OS randomness), one commitment, one pairing product.  Returns
        (valid, bad_index): bad_index is None for a valid key, 0 when P_0 is infinity, and with locate=True the lowest i with
        P_{i+1} != tau P_i; otherwise None."""
        g2 = bytes(g2_bytes)
        if len(g2) != 256:
            raise ValueError("g2_bytes must be the 256 bytes of a key file's G2 section, got %d" % len(g2))
        valid, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
        _check(lib().plk_srs_check(self._h, g2, self._seed(seed), ctypes.c_uint32(2 if locate else 0), ctypes.byref(valid), ctypes.byref(bad)))
        return bool(valid.value), (bad.value if bad.value != 2**64 - 1 else None)

    def srs_check_points_dev(self, ptr, n, g2_bytes, seed=None, locate=False, stream=None):
        """srs_check for `n` points in device memory (the key's form) that are NOT installed: the same (valid, bad_index) as srs_check on
        those points made resident.  No key needs to be resident, nothing resident changes and no fixed-base table is built."""
        g2 = bytes(g2_bytes)
        if len(g2) != 256:
            raise ValueError("g2_bytes must be the 256 bytes of a key file's G2 section, got %d" % len(g2))
        valid, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
        _check(lib().plk_srs_check_points_dev(self._h, _devptr(ptr), ctypes.c_uint64(n), g2, self._seed(seed), ctypes.c_uint32(2 if locate else 0),
                                              ctypes.byref(valid), ctypes.byref(bad), _stream(stream)))
        return bool(valid.value), (bad.value if bad.value != 2**64 - 1 else None)

    def srs_lagrange_check(self, seed=None):
        """does the resident Lagrange-form key belong to the resident monomial key (same tau, same domain, same order)?"""
        valid = ctypes.c_int32(0)
        _check(lib().plk_srs_lagrange_check(self._h, self._seed(seed), ctypes.byref(valid)))
        return bool(valid.value)

    # ---- contributing a secret to the key (srs_update.hip; the reference has no counterpart)
    def srs_update(self, g2, s=None, first=0):
        """resident points P_i (global indexes first + i) <- s^(first + i) P_i, the step of an updatable SRS.  `g2`: the 256 bytes of the
        key's G2 section; `s`: 4 x uint64 Montgomery Fr, None: drawn from the OS inside the call and gone when it returns.  Returns
        (g2_new, receipt): the new G2 section and the 192 bytes S1 || S2 that srs_update_verify checks."""
        g2 = bytes(g2)
        if len(g2) != 256:
            raise ValueError("g2 must be the 256 bytes of a key file's G2 section, got %d" % len(g2))
        sv = np.ascontiguousarray(s, dtype=np.uint64).reshape(4) if s is not None else None
        g2_new, receipt = ctypes.create_string_buffer(256), ctypes.create_string_buffer(192)
        _check(lib().plk_srs_update(self._h, _np(sv) if sv is not None else None, ctypes.c_uint64(first), g2, g2_new, receipt))
        return g2_new.raw, receipt.raw

    def srs_update_last_ms(self):
        """HIP-event time of the device work of the last srs_update on the context (set_kernel_timing on)"""
        v = ctypes.c_float(0)
        _check(lib().plk_srs_update_last_ms(self._h, ctypes.byref(v)))
        return v.value

    def srs_update_verify(self, old_p01, g2_old, g2_new, receipt, seed=None):
        """is the resident key (whole prefix) the key of `old_p01` (its points 0 and 1, [2, 8] uint64; [1, 8] for a one-point key) and
        `g2_old`, updated by the s committed in `receipt`?  Returns (valid, reason): reason is one of UPDATE_REASONS, "ok" when valid."""
        p = np.zeros((2, 8), dtype=np.uint64)
        o = np.ascontiguousarray(old_p01, dtype=np.uint64).reshape(-1, 8)
        p[:min(2, o.shape[0])] = o[:2]
        g2_old, g2_new, receipt = _update_bytes(g2_old, g2_new, receipt)
        valid, reason = ctypes.c_int32(0), ctypes.c_uint32(0)
        _check(lib().plk_srs_update_verify(self._h, _np(p), g2_old, g2_new, receipt, self._seed(seed), ctypes.byref(valid), ctypes.byref(reason)))
        return bool(valid.value), UPDATE_REASONS[reason.value]

    def set_kernel_timing(self, on=True):
        _check(lib().plk_set_kernel_timing(self._h, ctypes.c_int32(1 if on else 0)))

    def msm_last_kernel_ms(self):
        v = ctypes.c_float(0)
        _check(lib().plk_msm_last_kernel_ms(self._h, ctypes.byref(v)))
        return v.value

    def msm_last_shape(self):
        """diagnostic (plk_msm_last_shape): the dispatch shape of the commitment finished last, as a dict of the struct's fields;
        `path` is one of MSM_PATHS"""
        v = MsmShape()
        _check(lib().plk_msm_last_shape(self._h, ctypes.byref(v)))
        d = {name: int(getattr(v, name)) for name, _ in MsmShape._fields_}
        d["path"] = MSM_PATHS[d["path"]]
        return d

    def msm_last_no_inf(self):
        """diagnostic (plk_msm_last_no_inf): True if the accumulation of the commitment finished last ran without the point-at-infinity
        test (the resident key's table holds no such point and the commitment took the plain kernel)"""
        v = ctypes.c_uint32(0)
        _check(lib().plk_msm_last_no_inf(self._h, ctypes.byref(v)))
        return bool(v.value)

    # ---- NTT
    def ntt(self, data, log_n, inverse=False, coset=None):
        """host array in, new host array out (natural order)."""
        a = np.ascontiguousarray(data, dtype=np.uint64).copy()
        assert a.shape == (1 << log_n, 4)
        c = np.ascontiguousarray(coset, dtype=np.uint64) if coset is not None else None
        _check(lib().plk_ntt(self._h, _np(a), ctypes.c_uint32(log_n), ctypes.c_int32(1 if inverse else 0),
                             _np(c) if c is not None else None))
        return a

    def ntt_dev(self, ptr, log_n, inverse=False, coset=None, stream=None):
        c = np.ascontiguousarray(coset, dtype=np.uint64) if coset is not None else None
        _check(lib().plk_ntt_dev(self._h, _devptr(ptr), ctypes.c_uint32(log_n), ctypes.c_int32(1 if inverse else 0),
                                 _np(c) if c is not None else None, _stream(stream)))

    def lde4(self, coeffs, log_n):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64)
        assert a.shape == (1 << log_n, 4)
        out = np.zeros((4 << log_n, 4), dtype=np.uint64)
        _check(lib().plk_lde4(self._h, _np(a), ctypes.c_uint32(log_n), _np(out)))
        return out

    def lde4_dev(self, in_ptr, log_n, out_ptr, stream=None):
        _check(lib().plk_lde4_dev(self._h, _devptr(in_ptr), ctypes.c_uint32(log_n), _devptr(out_ptr), _stream(stream)))

    def lde4_coset_major_dev(self, in_ptrs, log_n, out_ptrs, stream=None):
        """`count` polynomials -> their 4n evaluations in the prover's coset-major order (out[k*n + r] = f(7 w_4n^(4r+k)))"""
        cnt = len(in_ptrs)
        ins = (ctypes.c_void_p * cnt)(*[_devptr(p).value for p in in_ptrs])
        outs = (ctypes.c_void_p * cnt)(*[_devptr(p).value for p in out_ptrs])
        _check(lib().plk_lde4_coset_major_dev(self._h, ins, ctypes.c_uint32(cnt), ctypes.c_uint32(log_n), outs, _stream(stream)))

    def icoset4_coset_major_dev(self, ptr, log_n, stream=None):
        """4n values in coset-major order -> the 4n coefficients (natural order), in place"""
        _check(lib().plk_icoset4_coset_major_dev(self._h, _devptr(ptr), ctypes.c_uint32(log_n), _stream(stream)))

    # ---- MSM
    def msm(self, scalars, base_offset=0):
        s = np.ascontiguousarray(scalars, dtype=np.uint64)
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().plk_msm_g1(self._h, _np(s), ctypes.c_uint64(s.shape[0]), ctypes.c_uint64(base_offset), _np(out)))
        return out

    def msm_dev(self, ptr, n, base_offset=0, stream=None):
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().plk_msm_g1_dev(self._h, _devptr(ptr), ctypes.c_uint64(n), ctypes.c_uint64(base_offset), _np(out), _stream(stream)))
        return out

    def msm_batch_dev(self, ptrs, n, base_offset=0, stream=None):
        """several commitments (same length, same bases) in one pass; returns [count, 8] affine points"""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        out = np.zeros((len(ptrs), 8), dtype=np.uint64)
        _check(lib().plk_msm_g1_batch_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint64(n), ctypes.c_uint64(base_offset), _np(out), _stream(stream)))
        return out

    # ---- MSM against caller-supplied bases: no resident key, no fixed-base table (plk_msm_g1_bases*)
    def _bases_result(self, rc, bad, out):
        if rc != 0:
            self._raise_with_bad_index(rc, bad)                       # a refused base (check=True): PlkError with `.bad_index`
        return out

    def msm_bases(self, bases, scalars, check=False):
        """sum_i scalars[i] * bases[i] for host arrays: bases (n, 8) uint64 in the key's form (x ‖ y Montgomery, zeros = infinity), scalars
        (n, 4) uint64 Montgomery Fr.  check=True refuses a base that is not on the curve: PlkError with `.bad_index` = the lowest such index."""
        b = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        if b.shape[0] != s.shape[0]:
            raise ValueError("msm_bases: %d bases and %d scalars" % (b.shape[0], s.shape[0]))
        out, bad = np.zeros(8, dtype=np.uint64), ctypes.c_uint64(0)
        rc = lib().plk_msm_g1_bases(self._h, _np(b), _np(s), ctypes.c_uint64(s.shape[0]), ctypes.c_uint32(1 if check else 0), _np(out), ctypes.byref(bad))
        return self._bases_result(rc, bad, out)

    def msm_bases_dev(self, bases_ptr, scalars_ptr, n, check=False, stream=None):
        out, bad = np.zeros(8, dtype=np.uint64), ctypes.c_uint64(0)
        rc = lib().plk_msm_g1_bases_dev(self._h, _devptr(bases_ptr), _devptr(scalars_ptr), ctypes.c_uint64(n), ctypes.c_uint32(1 if check else 0),
                                        _np(out), ctypes.byref(bad), _stream(stream))
        return self._bases_result(rc, bad, out)

    def msm_bases_batch_dev(self, bases_ptr, scalar_ptrs, n, check=False, stream=None):
        """several scalar vectors (same length) against the same caller-supplied bases in one pass; returns [count, 8] affine points"""
        arr = (ctypes.c_void_p * len(scalar_ptrs))(*[_devptr(p) for p in scalar_ptrs])
        out, bad = np.zeros((len(scalar_ptrs), 8), dtype=np.uint64), ctypes.c_uint64(0)
        rc = lib().plk_msm_g1_bases_batch_dev(self._h, _devptr(bases_ptr), arr, ctypes.c_uint32(len(scalar_ptrs)), ctypes.c_uint64(n),
                                              ctypes.c_uint32(1 if check else 0), _np(out), ctypes.byref(bad), _stream(stream))
        return self._bases_result(rc, bad, out)

    def msm_partial_dev(self, ptr, n, base_offset=0, stream=None):
        out = np.zeros(12, dtype=np.uint64)
        _check(lib().plk_msm_g1_partial_dev(self._h, _devptr(ptr), ctypes.c_uint64(n), ctypes.c_uint64(base_offset), _np(out), _stream(stream)))
        return out

    def msm_enqueue_dev(self, ptr, n, base_offset=0, stream=None):
        _check(lib().plk_msm_g1_enqueue_dev(self._h, _devptr(ptr), ctypes.c_uint64(n), ctypes.c_uint64(base_offset), _stream(stream)))

    def msm_enqueue_batch_dev(self, ptrs, n, base_offset=0, stream=None):
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        _check(lib().plk_msm_g1_enqueue_batch_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint64(n), ctypes.c_uint64(base_offset), _stream(stream)))

    def msm_finish_batch(self, count):
        out = np.zeros((count, 12), dtype=np.uint64)
        _check(lib().plk_msm_g1_finish_batch(self._h, _np(out), ctypes.c_uint32(count)))
        return out

    def msm_finish_batch_sharded(self, count):
        """finish + the installed combiner (one exchange for the batch): [count, 8] affine commitments over all ranks' shards"""
        out = np.zeros((count, 8), dtype=np.uint64)
        _check(lib().plk_msm_g1_finish_batch_sharded(self._h, _np(out), ctypes.c_uint32(count)))
        return out

    def msm_finish(self):
        out = np.zeros(12, dtype=np.uint64)
        _check(lib().plk_msm_g1_finish(self._h, _np(out)))
        return out

    def g1_intt(self, points, log_n):
        p = np.ascontiguousarray(points, dtype=np.uint64)
        assert p.shape == (1 << log_n, 8)
        out = np.zeros_like(p)
        _check(lib().plk_g1_intt(self._h, _np(p), ctypes.c_uint32(log_n), _np(out)))
        return out


    # ---- tracing hook and the polynomial helpers of rounds 2, 4, 5 (tests localise a wrong proof with them)
    def prove_trace(self, which):
        """vector `which` of the last prove on this context: 0..3 wire polynomials, 4 z, 5 t (4N), 6 r, 7 / 8 opening quotients"""
        n = ctypes.c_uint64(0)
        _check(lib().plk_prove_trace(self._h, ctypes.c_uint32(which), None, ctypes.c_uint64(0), ctypes.byref(n)))
        out = np.zeros((n.value, 4), dtype=np.uint64)
        _check(lib().plk_prove_trace(self._h, ctypes.c_uint32(which), _np(out), ctypes.c_uint64(n.value), ctypes.byref(n)))
        return out

    def poly_evaluate_at_dev(self, ptr, n, z, stream=None):
        z = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().plk_poly_evaluate_at_dev(self._h, _devptr(ptr), ctypes.c_uint64(n), _np(z), _np(out), _stream(stream)))
        return out

    def poly_divide_by_linear_dev(self, ptr, n, z, out_ptr, stream=None):
        z = np.ascontiguousarray(z, dtype=np.uint64)
        _check(lib().plk_poly_divide_by_linear_dev(self._h, _devptr(ptr), ctypes.c_uint64(n), _np(z), _devptr(out_ptr), _stream(stream)))

    # ---- KZG openings on their own (kzg.hip): values on the domain as well as coefficients
    def poly_evaluate_values_at_dev(self, ptr, log_n, z, stream=None):
        """plk_poly_evaluate_values_at_dev: f(z) from the 2^log_n values f(omega^i) in device memory (barycentric; z = omega^k reads f_k)"""
        z = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().plk_poly_evaluate_values_at_dev(self._h, _devptr(ptr), ctypes.c_uint32(log_n), _np(z), _np(out), _stream(stream)))
        return out

    def poly_divide_values_by_linear_dev(self, ptr, log_n, z, out_ptr, y=None, stream=None):
        """plk_poly_divide_values_by_linear_dev: the values of (f - y) / (x - z) from the values of f; y=None: f(z).  out_ptr may be ptr."""
        z = np.ascontiguousarray(z, dtype=np.uint64)
        y = np.ascontiguousarray(y, dtype=np.uint64) if y is not None else None
        _check(lib().plk_poly_divide_values_by_linear_dev(self._h, _devptr(ptr), ctypes.c_uint32(log_n), _np(z), _np(y) if y is not None else None,
                                                          _devptr(out_ptr), _stream(stream)))

    def kzg_commit_dev(self, ptrs, n, values=False, stream=None):
        """plk_kzg_commit_dev: [count, 8] commitments of count <= 8 device vectors of n elements: coefficients against the resident key, or
        (values=True) values on the domain against the Lagrange-form key"""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        out = np.zeros((len(ptrs), 8), dtype=np.uint64)
        _check(lib().plk_kzg_commit_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint64(n), ctypes.c_uint32(1 if values else 0), _np(out), _stream(stream)))
        return out

    def kzg_open_dev(self, ptrs, n, z, v=None, values=False, stream=None):
        """plk_kzg_open_dev: opens count <= 8 polynomials at z, combined by powers of v (None allowed for one polynomial):
        ([count, 4] evaluations, the proof point [8])"""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        z = np.ascontiguousarray(z, dtype=np.uint64)
        v = np.ascontiguousarray(v, dtype=np.uint64) if v is not None else None
        evals, proof = np.zeros((len(ptrs), 4), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        _check(lib().plk_kzg_open_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint64(n), _np(z), _np(v) if v is not None else None,
                                      ctypes.c_uint32(1 if values else 0), _np(evals), _np(proof), _stream(stream)))
        return evals, proof

    def kzg_verify_many_dev(self, commitments_ptr, z_ptr, evals_ptr, proofs_ptr, n, g2_bytes, verdict_ptr, stream=None):
        """plk_kzg_verify_many_dev: n single-polynomial openings in device memory, one verdict byte each (1 / 0, 2 = malformed), each what
        kzg_verify says about that opening; ordered on `stream`, does not wait"""
        _check(lib().plk_kzg_verify_many_dev(self._h, _devptr(commitments_ptr), _devptr(z_ptr), _devptr(evals_ptr), _devptr(proofs_ptr), ctypes.c_uint64(n),
                                             bytes(g2_bytes), _devptr(verdict_ptr), _stream(stream)))

    @staticmethod
    def _kzg_multi_masks(who, count, sets):
        masks = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1)
        if 1 <= count <= 32 and masks.shape[0] != count:                 # (a count out of range is the library's to refuse; it reads no set then)
            raise ValueError("%s: %d polynomials need %d sets, got %d" % (who, count, count, masks.shape[0]))
        return masks if masks.shape[0] else np.zeros(1, dtype=np.uint32)

    def kzg_verify_multi_many_dev(self, count, npoints, sets, commitments_ptr, points_ptr, evals_ptr, gamma_ptr, u_ptr, proofs_ptr, n, g2_bytes, verdict_ptr,
                                  stream=None):
        """plk_kzg_verify_multi_many_dev: n multi-point openings of ONE shape (count polynomials, npoints points, sets: count masks on the host)
        in device memory — per opening count commitments, npoints points, count x npoints evaluations, gamma, u and the proof points W, W' —
        one verdict byte each (1 / 0, 2 = malformed), each what kzg_verify_multi says about that opening; ordered on `stream`, does not wait"""
        masks = self._kzg_multi_masks("kzg_verify_multi_many_dev", count, sets)
        _check(lib().plk_kzg_verify_multi_many_dev(self._h, ctypes.c_uint32(count), ctypes.c_uint32(npoints), _np(masks), _devptr(commitments_ptr), _devptr(points_ptr),
                                                   _devptr(evals_ptr), _devptr(gamma_ptr), _devptr(u_ptr), _devptr(proofs_ptr), ctypes.c_uint64(n), bytes(g2_bytes),
                                                   _devptr(verdict_ptr), _stream(stream)))

    def kzg_verify_multi_front_dev(self, count, npoints, sets, commitments_ptr, points_ptr, evals_ptr, gamma_ptr, u_ptr, proofs_ptr, n, scalars_ptr, state_ptr,
                                   stream=None):
        """plk_kzg_verify_multi_front_dev: the front of kzg_verify_multi_many_dev on its own.  Per opening count + 3 Montgomery scalars
        (c_0 .. c_{count-1}, -sum c_i r_i(u), -Z_T(u), u: what multiplies C_0 .. C_{count-1}, G, W, W') and a state byte: 1 = goes on to
        the group arithmetic, 2 = malformed (its scalars are zero); ordered on `stream`, does not wait"""
        masks = self._kzg_multi_masks("kzg_verify_multi_front_dev", count, sets)
        _check(lib().plk_kzg_verify_multi_front_dev(self._h, ctypes.c_uint32(count), ctypes.c_uint32(npoints), _np(masks), _devptr(commitments_ptr), _devptr(points_ptr),
                                                    _devptr(evals_ptr), _devptr(gamma_ptr), _devptr(u_ptr), _devptr(proofs_ptr), ctypes.c_uint64(n),
                                                    _devptr(scalars_ptr), _devptr(state_ptr), _stream(stream)))

    def kzg_open_all_prepare(self, log_n):
        """plk_kzg_open_all_prepare: build and keep the transform of the resident key for the 2^log_n domain (optional; kzg_open_all_dev builds it
        on first use)"""
        _check(lib().plk_kzg_open_all_prepare(self._h, ctypes.c_uint32(log_n)))

    def kzg_open_all_dev(self, poly_ptr, log_n, proofs_ptr, evals_ptr=None, values=False, stream=None):
        """plk_kzg_open_all_dev: proofs_ptr[i] <- the opening proof at omega^i of the polynomial at poly_ptr (2^log_n coefficients, or with
        values=True its values on the domain), for every i at once; evals_ptr (optional) <- f(omega^i).  Blocks."""
        _check(lib().plk_kzg_open_all_dev(self._h, _devptr(poly_ptr), ctypes.c_uint32(log_n), ctypes.c_uint32(1 if values else 0), _devptr(proofs_ptr),
                                          _devptr(evals_ptr) if evals_ptr is not None else None, _stream(stream)))

    def kzg_open_all_batch_dev(self, polys_ptr, count, log_n, proofs_ptr, evals_ptr=None, values=False, stream=None):
        """plk_kzg_open_all_batch_dev: kzg_open_all_dev for `count` polynomials of 2^log_n back to back at polys_ptr, in one pass under the one
        key: proofs_ptr[b * N + i] <- the proof at omega^i of polynomial b, evals_ptr (optional) likewise.  Blocks."""
        _check(lib().plk_kzg_open_all_batch_dev(self._h, _devptr(polys_ptr), ctypes.c_uint32(count), ctypes.c_uint32(log_n), ctypes.c_uint32(1 if values else 0),
                                                _devptr(proofs_ptr), _devptr(evals_ptr) if evals_ptr is not None else None, _stream(stream)))

    def kzg_open_all_last_ms(self):
        """plk_kzg_open_all_last_ms: [key transform, scalar NTTs, point-wise product, inverse transform, forward transform + affine] of the last
        kzg_open_all_dev, in ms (set_kernel_timing must be on)"""
        out = (ctypes.c_float * 5)()
        _check(lib().plk_kzg_open_all_last_ms(self._h, out))
        return [float(v) for v in out]

    # ---- many polynomials at several points, a proof of two points (kzg_multi.hip)
    _KZG_CHALLENGE = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64))

    def poly_quotient_multi_dev(self, ptrs, n, points, coef, out_ptr, stream=None):
        """plk_poly_quotient_multi_dev: out[k] = sum_j sum_{l > k} G_j[l] t_j^(l-k-1) with G_j = sum_i coef[i][j] f_i, for count <= 64 device
        polynomials of n coefficients, points [npoints <= 8, 4] and coef [count, npoints, 4]; out_ptr is none of the inputs.  Blocks."""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        cf = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
        if cf.shape[0] != len(ptrs) * pts.shape[0]:
            raise ValueError("poly_quotient_multi_dev: %d polynomials and %d points need %d coefficients, got %d"
                             % (len(ptrs), pts.shape[0], len(ptrs) * pts.shape[0], cf.shape[0]))
        _check(lib().plk_poly_quotient_multi_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint64(n), _np(pts), ctypes.c_uint32(pts.shape[0]), _np(cf),
                                                 _devptr(out_ptr), _stream(stream)))

    def kzg_open_multi_dev(self, ptrs, n, points, sets, gamma, challenge, stream=None):
        """plk_kzg_open_multi_dev: opens count <= 32 device polynomials of n coefficients, polynomial i at the points named by the bits of
        sets[i] (points: [npoints <= 8, 4]), with a proof of two points.  challenge: a callable W ([8] uint64) -> u ([4] uint64), called once
        after the first commitment, or a fixed scalar u.  Returns ([count, npoints, 4] evaluations, zero outside the sets; u; [2, 8] W, W').
        An exception raised by the callable is raised again here, after the call has failed with PLK_ERR_IO."""
        return self._kzg_open_multi("kzg_open_multi_dev", lib().plk_kzg_open_multi_dev, ptrs, ctypes.c_uint64(n), points, sets, gamma, challenge, stream)

    def _kzg_open_multi(self, name, fn, ptrs, size, points, sets, gamma, challenge, stream):
        """the two routes of the multi-point opening: the arrays, the callback around `challenge`, the call, the outputs"""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        masks = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1)
        if masks.shape[0] != len(ptrs):
            raise ValueError("%s: %d polynomials and %d sets" % (name, len(ptrs), masks.shape[0]))
        gamma = np.ascontiguousarray(gamma, dtype=np.uint64)
        raised = []

        def _call(_user, w, u_out):
            try:
                u = challenge(np.array([w[k] for k in range(8)], dtype=np.uint64)) if callable(challenge) else challenge
                if isinstance(u, int):                                # a plain int from the callable is the C callback's return code (non-zero: failure)
                    return u
                u = np.ascontiguousarray(u, dtype=np.uint64).reshape(4)
                for k in range(4):
                    u_out[k] = int(u[k])
                return 0
            except Exception as e:                                    # noqa: BLE001 — an exception must not cross the C frames
                raised.append(e)
                return -1

        cb = self._KZG_CHALLENGE(_call)                               # kept alive by this frame until the call has returned
        evals = np.zeros((len(ptrs), pts.shape[0], 4), dtype=np.uint64)
        u, proof = np.zeros(4, dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
        rc = fn(self._h, arr, ctypes.c_uint32(len(ptrs)), size, _np(pts), ctypes.c_uint32(pts.shape[0]), _np(masks),
                _np(gamma), cb, None, _np(evals), _np(u), _np(proof), _stream(stream))
        if raised:
            raise raised[0]
        _check(rc)
        return evals, u, proof

    def kzg_open_multi_last_ms(self):
        """plk_kzg_open_multi_last_ms: [evaluations, first quotient, its commitment, second quotient with its commitment] of the last
        kzg_open_multi_dev or kzg_open_multi_values_dev, in ms (set_kernel_timing must be on)"""
        out = (ctypes.c_float * 4)()
        _check(lib().plk_kzg_open_multi_last_ms(self._h, out))
        return [float(v) for v in out]

    # ---- the same from values on the domain, against the Lagrange-form key (kzg_multi_values.hip)
    def kzg_open_multi_values_dev(self, ptrs, log_n, points, sets, gamma, challenge, stream=None):
        """plk_kzg_open_multi_values_dev: kzg_open_multi_dev for count <= 32 device arrays of the 2^log_n values f_i(omega^k): no transform, the
        commitments against the Lagrange-form key.  The same arguments otherwise and the same return, byte for byte what kzg_open_multi_dev
        gives for the coefficients of the same polynomials: ([count, npoints, 4] evaluations, zero outside the sets; u; [2, 8] W, W')."""
        return self._kzg_open_multi("kzg_open_multi_values_dev", lib().plk_kzg_open_multi_values_dev, ptrs, ctypes.c_uint32(log_n), points, sets, gamma,
                                    challenge, stream)

    def poly_quotient_multi_values_dev(self, ptrs, log_n, points, coef, out_ptr, stream=None):
        """plk_poly_quotient_multi_values_dev: out = the 2^log_n values of sum_j D_{t_j}[sum_i coef[i][j] f_i] from the values of count <= 64
        device polynomials, points [npoints <= 8, 4] (on the domain or off it) and coef [count, npoints, 4]; out_ptr is none of the inputs.  Blocks."""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        cf = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
        if cf.shape[0] != len(ptrs) * pts.shape[0]:
            raise ValueError("poly_quotient_multi_values_dev: %d polynomials and %d points need %d coefficients, got %d"
                             % (len(ptrs), pts.shape[0], len(ptrs) * pts.shape[0], cf.shape[0]))
        _check(lib().plk_poly_quotient_multi_values_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint32(log_n), _np(pts), ctypes.c_uint32(pts.shape[0]),
                                                        _np(cf), _devptr(out_ptr), _stream(stream)))

    def poly_evaluate_values_multi_dev(self, ptrs, log_n, points, sets, stream=None):
        """plk_poly_evaluate_values_multi_dev: [count, npoints, 4] evaluations f_i(t_j) for bit j of sets[i], zero elsewhere, from the 2^log_n
        values of count <= 64 device polynomials; every polynomial is read once for all its points.  Blocks."""
        arr = (ctypes.c_void_p * len(ptrs))(*[_devptr(p) for p in ptrs])
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        masks = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1)
        if masks.shape[0] != len(ptrs):
            raise ValueError("poly_evaluate_values_multi_dev: %d polynomials and %d sets" % (len(ptrs), masks.shape[0]))
        evals = np.zeros((len(ptrs), pts.shape[0], 4), dtype=np.uint64)
        _check(lib().plk_poly_evaluate_values_multi_dev(self._h, arr, ctypes.c_uint32(len(ptrs)), ctypes.c_uint32(log_n), _np(pts), ctypes.c_uint32(pts.shape[0]),
                                                        _np(masks), _np(evals), _stream(stream)))
        return evals

    def g1_ntt_dev(self, in_ptr, log_n, out_ptr, inverse=False, stream=None):
        """plk_g1_ntt_dev: the G1 transform of 2^log_n affine points in device memory, forward (out[i] = sum_j omega^(i j) in[j]) or inverse
        (g1_intt's, bit for bit); ordered on `stream`, does not wait"""
        _check(lib().plk_g1_ntt_dev(self._h, _devptr(in_ptr), ctypes.c_uint32(log_n), ctypes.c_int32(1 if inverse else 0), _devptr(out_ptr), _stream(stream)))

    def g1_ntt_batch_dev(self, in_ptr, count, log_n, out_ptr, inverse=False, stream=None):
        """plk_g1_ntt_batch_dev: g1_ntt_dev over `count` arrays of 2^log_n affine points back to back, every stage of all of them in one launch;
        ordered on `stream`, does not wait"""
        _check(lib().plk_g1_ntt_batch_dev(self._h, _devptr(in_ptr), ctypes.c_uint32(count), ctypes.c_uint32(log_n), ctypes.c_int32(1 if inverse else 0),
                                          _devptr(out_ptr), _stream(stream)))

    def permutation_grand_product_dev(self, wires, sigmas, beta, gamma, log_n, out_ptr, stream=None):
        w = (ctypes.c_void_p * 4)(*[_devptr(p) for p in wires])
        s = (ctypes.c_void_p * 4)(*[_devptr(p) for p in sigmas])
        b, g = np.ascontiguousarray(beta, dtype=np.uint64), np.ascontiguousarray(gamma, dtype=np.uint64)
        _check(lib().plk_permutation_grand_product_dev(self._h, w, s, _np(b), _np(g), ctypes.c_uint32(log_n), _devptr(out_ptr), _stream(stream)))

    def setup_permutation_dev(self, vars_ptrs, log_n, num_vars, index_ptr=None, sigma_ptrs=None, stream=None):
        """plk_setup_permutation_dev: the setup's copy-constraint permutation from four device columns of 2^log_n uint32 variable ids
        (every id < num_vars, id 0 the dummy); index_ptr: 4 * 2^log_n uint32 (col' << 30 | row'), sigma_ptrs: four columns of 2^log_n Fr"""
        v = (ctypes.c_void_p * 4)(*[_devptr(p) for p in vars_ptrs])
        s = (ctypes.c_void_p * 4)(*[_devptr(p) for p in sigma_ptrs]) if sigma_ptrs is not None else None
        _check(lib().plk_setup_permutation_dev(self._h, v, ctypes.c_uint32(log_n), ctypes.c_uint64(num_vars),
                                               _devptr(index_ptr) if index_ptr is not None else None, s, _stream(stream)))

    def sigma_decode_dev(self, sigmas, log_n, stream=None):
        """plk_sigma_decode_dev, the inverse of setup_permutation_dev's sigma output: four device columns of 2^log_n Fr (torch tensors /
        ints) -> (index, bad_key).  index: an int32 torch tensor of 4 * 2^log_n words holding the uint32 bit patterns
        idx[col * n + row] = col' << 30 | row', 0xFFFFFFFF where the value is no cell label; bad_key: row * 4 + col of the lowest such cell,
        None when every value decodes"""
        import torch
        if len(sigmas) != 4:
            raise ValueError("sigma_decode_dev: 4 sigma columns expected, got %d" % len(sigmas))
        if not 1 <= log_n <= 26:
            raise PlkError(1, "plk_sigma_decode_dev: bad argument")
        s = (ctypes.c_void_p * 4)(*[_devptr(p) for p in sigmas])
        index = torch.empty(4 << log_n, dtype=torch.int32, device="cuda:%d" % self.device)
        bad = ctypes.c_uint64(0)
        _check(lib().plk_sigma_decode_dev(self._h, s, ctypes.c_uint32(log_n), _devptr(index), ctypes.byref(bad), _stream(stream)))
        return index, (bad.value if bad.value != 2**64 - 1 else None)

    def g1_intt_srs_dev(self, log_n, out_ptr, stream=None):
        _check(lib().plk_g1_intt_srs_dev(self._h, ctypes.c_uint32(log_n), _devptr(out_ptr), _stream(stream)))


    def pairing_check_many_dev(self, a_ptr, b_ptr, n, g2_bytes, verdict_ptr, stream=None):
        """plk_pairing_check_many_dev: n checks e(A_i, Q_0) e(B_i, Q_1) == 1 on device arrays of affine points; one verdict byte each
        (1 / 0, 2 = a point off the curve), ordered on `stream`"""
        _check(lib().plk_pairing_check_many_dev(self._h, _devptr(a_ptr), _devptr(b_ptr), ctypes.c_uint64(n), bytes(g2_bytes), _devptr(verdict_ptr), _stream(stream)))

    def verify_front_dev(self, key, blob_ptr, blob_len, off_ptr, count, points_ptr, scalars_ptr, state_ptr, stream=None):
        """plk_verify_front_dev: the verifier's front kernel on its own.  Device memory: the packed proof bytes, count + 1 uint64 offsets, and
        per proof 25 affine points, 25 scalars (plk_verify_terms's, zero unless state is 1) and a state byte (1 goes on, 0 invalid, 2 malformed);
        ordered on `stream`"""
        _check(lib().plk_verify_front_dev(self._h, key._h, _devptr(blob_ptr), ctypes.c_uint64(blob_len), _devptr(off_ptr), ctypes.c_uint64(count), _devptr(points_ptr),
                                          _devptr(scalars_ptr), _devptr(state_ptr), _stream(stream)))

    def verify_many_last_ms(self):
        """plk_verify_many_last_ms (set_kernel_timing on): host flattening (after verify_many_packed: the front kernel), upload, scalar
        multiplications, sums, pairing checks, download"""
        out = (ctypes.c_float * 6)()
        _check(lib().plk_verify_many_last_ms(self._h, out))
        return [float(x) for x in out]

# ------------------------------------------------- circuit pipeline (mirrors src/plonk.rs's API)
class Circuit:
    """CircomCircuit{r1cs, witness, wire_mapping: None, aux_offset: 1} (src/circom_circuit.rs:41-47).
    File type is chosen from the suffix exactly as the reference does (src/reader.rs:93,179)."""

    def __init__(self, r1cs_bytes, r1cs_is_json, witness_bytes=None, witness_is_json=False):
        self._h = ctypes.c_void_p()
        _check(lib().plk_circuit_load(bytes(r1cs_bytes), ctypes.c_uint64(len(r1cs_bytes)), ctypes.c_int32(1 if r1cs_is_json else 0),
                                      bytes(witness_bytes) if witness_bytes is not None else None,
                                      ctypes.c_uint64(len(witness_bytes) if witness_bytes is not None else 0),
                                      ctypes.c_int32(1 if witness_is_json else 0), ctypes.byref(self._h)))

    @classmethod
    def synthetic(cls, target_gates, seed=0x706c6f6e6b6974):
        """seeded chain circuit with exactly `target_gates` gates and one public input (bench input)"""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        _check(lib().plk_circuit_synthetic(ctypes.c_uint64(target_gates), ctypes.c_uint64(seed), ctypes.byref(self._h)))
        return self

    @classmethod
    def synthetic_ex(cls, target_gates, seed=0x706c6f6e6b6974, witness_seed=0, lc_terms=0):
        """the same generator; witness_seed != 0: same R1CS, another satisfying witness; lc_terms >= 5: dense body (long
        linear combinations folded through the d column: all 11 commitments of a proof are non-trivial; parity unpinned)"""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        _check(lib().plk_circuit_synthetic_ex(ctypes.c_uint64(target_gates), ctypes.c_uint64(seed), ctypes.c_uint64(witness_seed),
                                              ctypes.c_uint32(lc_terms), ctypes.byref(self._h)))
        return self

    def export(self, what):
        """what = "r1cs" | "wtns": bytes in the reference's binary formats"""
        code = {"r1cs": 0, "wtns": 1}[what]
        n = ctypes.c_uint64(0)
        _check(lib().plk_circuit_export(self._h, ctypes.c_int32(code), None, ctypes.c_uint64(0), ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        _check(lib().plk_circuit_export(self._h, ctypes.c_int32(code), buf, ctypes.c_uint64(n.value), ctypes.byref(n)))
        return buf.raw

    @classmethod
    def from_files(cls, r1cs_path, witness_path=None):
        w = open(witness_path, "rb").read() if witness_path else None
        return cls(open(r1cs_path, "rb").read(), r1cs_path.endswith("json"), w, bool(witness_path) and witness_path.endswith("json"))

    def domain_size(self):
        """N of the circuit's setup without building it (transpile only)"""
        n = ctypes.c_uint64(0)
        _check(lib().plk_circuit_domain_size(self._h, ctypes.byref(n)))
        return n.value

    def analyse(self):
        """plonk::analyse (src/plonk.rs:72-93) as the serde_json string of src/tests.rs:14"""
        size = 1 << 20
        while True:                                                   # ~40 bytes per constraint: grow until it fits
            buf = ctypes.create_string_buffer(size)
            rc = lib().plk_circuit_analyse(self._h, buf, ctypes.c_uint64(size))
            if rc == 0:
                return buf.value.decode()
            if size >= (1 << 31) or "too small" not in last_error():
                _check(rc)
            size <<= 3

    def close(self):
        if self._h:
            lib().plk_circuit_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SetupForProver:
    """SetupForProver (src/plonk.rs:50-176): prepare_setup_for_prover / make_verification_key / prove."""

    def __init__(self, ctx, circuit):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().plk_setup_prepare(ctx._h, circuit._h, ctypes.byref(self._h)))

    @classmethod
    def prepare_host(cls, circuit):
        """the CPU half only (transpile + columns): no context, no GPU; finish with upload(ctx)"""
        self = cls.__new__(cls)
        self.ctx = None
        self._h = ctypes.c_void_p()
        _check(lib().plk_setup_prepare_host(circuit._h, ctypes.byref(self._h)))
        return self

    def upload(self, ctx):
        _check(lib().plk_setup_upload(ctx._h, self._h))
        self.ctx = ctx
        return self

    @property
    def domain_size(self):
        return lib().plk_setup_domain_size(self._h)

    def verification_key_bytes(self, g2_bytes):
        assert len(g2_bytes) == 256
        out = ctypes.create_string_buffer(4096)
        n = ctypes.c_uint64(0)
        _check(lib().plk_setup_write_vk(self.ctx._h, self._h, bytes(g2_bytes), out, ctypes.c_uint64(len(out)), ctypes.byref(n)))
        return out.raw[:n.value]

    def prove(self, circuit, ctx=None):
        """proof.bin bytes (the context's transcript: Keccak unless Context.set_transcript gave another — src/plonk.rs:152-159).  `ctx`: another context on the same device
        (one per host thread: several proofs of this setup may be in flight at once; ctypes releases the GIL for the call)"""
        h = (ctx or self.ctx)._h
        cap = 1 << 16
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint64(0)
        rc = lib().plk_prove(h, self._h, circuit._h, out, ctypes.c_uint64(cap), ctypes.byref(n))
        if rc == 1 and n.value > cap:                                 # many public inputs: retry with the reported size
            cap = n.value
            out = ctypes.create_string_buffer(cap)
            rc = lib().plk_prove(h, self._h, circuit._h, out, ctypes.c_uint64(cap), ctypes.byref(n))
        (ctx or self.ctx)._finish_prove(rc)
        return out.raw[:n.value]

    # ---- assembled input (plk_setup_from_polynomials / plk_prove_assembled*): bellman's SetupPolynomials and the prover assembly's
    #      wire columns (src/plonk.rs:50-55,104,152-159) instead of circuit bytes
    @classmethod
    def from_polynomials(cls, ctx, n, num_inputs, selectors, next_step, sigmas, values=False):
        """a resident setup from the 6 selectors (q_a q_b q_c q_d q_m q_const), the next-step selector q_d_next and the 4 sigmas,
        each a numpy (len, 4) uint64 array of Montgomery Fr (oracle_lib.fr_vec's format); values=False: monomial coefficients
        (1 <= len <= n + 1, zero-extended), values=True: the n + 1 evaluations on <omega_N> in row order"""
        if len(selectors) != 6 or len(sigmas) != 4:
            raise ValueError("from_polynomials: 6 selectors and 4 sigmas expected, got %d and %d" % (len(selectors), len(sigmas)))
        vecs = _fr_vectors(list(selectors) + [next_step] + list(sigmas), "from_polynomials")
        length = vecs[0].shape[0]
        self = cls.__new__(cls)
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        sel = (ctypes.c_void_p * 6)(*[_np(v) for v in vecs[:6]])
        sig = (ctypes.c_void_p * 4)(*[_np(v) for v in vecs[7:]])
        _check(lib().plk_setup_from_polynomials(ctx._h if ctx is not None else None, ctypes.c_uint64(n), ctypes.c_uint64(num_inputs), sel,
                                                _np(vecs[6]), sig, ctypes.c_uint64(length), ctypes.c_uint32(1 if values else 0),
                                                ctypes.byref(self._h)))
        return self

    def _prove_into(self, call, ctx=None):
        cap = 1 << 16
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint64(0)
        rc = call(out, cap, n)
        if rc == 1 and n.value > cap:                                 # many public inputs: retry with the reported size
            cap = n.value
            out = ctypes.create_string_buffer(cap)
            rc = call(out, cap, n)
        (ctx or self.ctx)._finish_prove(rc)
        return out.raw[:n.value]

    def prove_assembled(self, columns, ctx=None):
        """proof.bin bytes from the assembled wire columns a, b, c, d: four numpy (rows, 4) uint64 Montgomery arrays (zero-extended to
        the domain; public input i is a[i])"""
        if len(columns) != 4:
            raise ValueError("prove_assembled: 4 columns expected, got %d" % len(columns))
        cols = _fr_vectors(columns, "prove_assembled", allow_empty=True)
        rows = cols[0].shape[0]
        arr = (ctypes.c_void_p * 4)(*[_np(c) for c in cols])
        h = (ctx or self.ctx)._h
        return self._prove_into(lambda out, cap, n: lib().plk_prove_assembled(h, self._h, arr, ctypes.c_uint64(rows), out,
                                                                              ctypes.c_uint64(cap), ctypes.byref(n)), ctx)

    def prove_assembled_dev(self, ptrs, rows, stream=None, ctx=None):
        """the same from columns already on the device (4 torch tensors / ints, rows x 32 bytes each), ordered after `stream`"""
        if len(ptrs) != 4:
            raise ValueError("prove_assembled_dev: 4 column pointers expected, got %d" % len(ptrs))
        arr = (ctypes.c_void_p * 4)(*[_devptr(p) for p in ptrs])
        h = (ctx or self.ctx)._h
        st = _stream(stream)
        return self._prove_into(lambda out, cap, n: lib().plk_prove_assembled_dev(h, self._h, arr, ctypes.c_uint64(rows), out,
                                                                                  ctypes.c_uint64(cap), ctypes.byref(n), st), ctx)

    # ---- which copy constraint is broken (plk_setup_check_permutation / plk_check_copies*): what to call when prove_assembled says
    #      "copy constraints".  Exact checks, no key needed; every verdict is a CopyReport (kind 0 = all is well)
    def check_permutation(self, ctx=None):
        """is the setup's sigma a permutation of the cell labels: kind COPY_NOT_A_LABEL / COPY_NOT_BIJECTIVE with the lowest offending cell"""
        rep = _CopyReportStruct()
        _check(lib().plk_setup_check_permutation((ctx or self.ctx)._h, self._h, ctypes.byref(rep)))
        return rep.report()

    def check_copies(self, columns, ctx=None):
        """the sigma checks, then every cell's value against its image's: four numpy (rows, 4) uint64 Montgomery arrays as prove_assembled
        takes them; kind COPY_BROKEN names the lowest cell (row first, then a, b, c, d) that differs from its image"""
        if len(columns) != 4:
            raise ValueError("check_copies: 4 columns expected, got %d" % len(columns))
        cols = _fr_vectors(columns, "check_copies", allow_empty=True)
        arr = (ctypes.c_void_p * 4)(*[_np(c) for c in cols])
        rep = _CopyReportStruct()
        _check(lib().plk_check_copies((ctx or self.ctx)._h, self._h, arr, ctypes.c_uint64(cols[0].shape[0]), ctypes.byref(rep)))
        return rep.report()

    def check_copies_dev(self, column_tensors, stream=None, ctx=None):
        """the same for four torch tensors on the device, (rows, 4) int64 / uint64 each, ordered on `stream`"""
        if len(column_tensors) != 4:
            raise ValueError("check_copies_dev: 4 column tensors expected, got %d" % len(column_tensors))
        rows = int(column_tensors[0].shape[0])
        for t in column_tensors:
            if int(t.shape[0]) != rows or t.element_size() * t.numel() != 32 * rows or not t.is_contiguous():
                raise ValueError("check_copies_dev: contiguous tensors of one length, 32 bytes per row, expected")
        arr = (ctypes.c_void_p * 4)(*[_devptr(t) for t in column_tensors])
        rep = _CopyReportStruct()
        _check(lib().plk_check_copies_dev((ctx or self.ctx)._h, self._h, arr, ctypes.c_uint64(rows), ctypes.byref(rep), _stream(stream)))
        return rep.report()

    def validate_witness(self, circuit, ctx=None):
        """SetupForProver::validate_witness (src/plonk.rs:127-129): the gate-level check of prove() on its own, no key needed.
        Returns (valid, bad_row): bad_row is the lowest failing row of the gate table, None for a satisfying witness."""
        valid, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
        _check(lib().plk_validate_witness((ctx or self.ctx)._h, self._h, circuit._h, ctypes.byref(valid), ctypes.byref(bad)))
        return bool(valid.value), (bad.value if bad.value != 2**64 - 1 else None)

    # ---- one setup, a stream of witnesses: the witness without its circuit (plk_prove_witness / _witness_dev / _wtns)
    def prove_witness(self, w, ctx=None):
        """proof.bin bytes for the next witness of this setup's circuit: numpy (n, 4) uint64 Montgomery Fr, n >= num_variables"""
        w = _fr_vectors([w], "prove_witness", allow_empty=True)[0]
        h = (ctx or self.ctx)._h
        return self._prove_into(lambda out, cap, n: lib().plk_prove_witness(h, self._h, _np(w), ctypes.c_uint64(w.shape[0]), out,
                                                                            ctypes.c_uint64(cap), ctypes.byref(n)), ctx)

    def prove_witness_dev(self, ptr, n, stream=None, ctx=None):
        """the same for n elements already on the device (torch tensor / int), ordered after `stream`"""
        h, st = (ctx or self.ctx)._h, _stream(stream)
        return self._prove_into(lambda out, cap, ln: lib().plk_prove_witness_dev(h, self._h, _devptr(ptr), ctypes.c_uint64(n), out,
                                                                                 ctypes.c_uint64(cap), ctypes.byref(ln), st), ctx)

    def prove_wtns(self, data, ctx=None):
        """the same from the bytes of a .wtns file, decoded and range-checked on the device; an element >= r raises PlkError with
        `.bad_index` = the lowest such element"""
        buf = np.frombuffer(data, dtype=np.uint8)
        h, bad = (ctx or self.ctx)._h, ctypes.c_uint64(0)
        try:
            return self._prove_into(lambda out, cap, n: lib().plk_prove_wtns(h, self._h, _np(buf), ctypes.c_uint64(buf.size), out,
                                                                             ctypes.c_uint64(cap), ctypes.byref(n), ctypes.byref(bad)), ctx)
        except PlkError as e:
            e.bad_index = bad.value if bad.value != 2**64 - 1 else None
            raise

    def validate_witness_dev(self, ptr, n, stream=None, ctx=None):
        """validate_witness for n elements already on the device; returns (valid, bad_row)"""
        valid, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
        _check(lib().plk_validate_witness_dev((ctx or self.ctx)._h, self._h, _devptr(ptr), ctypes.c_uint64(n), ctypes.byref(valid),
                                              ctypes.byref(bad), _stream(stream)))
        return bool(valid.value), (bad.value if bad.value != 2**64 - 1 else None)

    def timings_ms(self, ctx=None):
        arr = (ctypes.c_double * 16)()
        cnt = ctypes.c_uint32(0)
        _check(lib().plk_prove_timings((ctx or self.ctx)._h, arr, ctypes.c_uint32(16), ctypes.byref(cnt)))
        names = ["witness", "round1", "round2", "round3", "round4", "round5", "serialise"]
        return {names[i] if i < len(names) else str(i): arr[i] for i in range(cnt.value)}

    def close(self):
        if self._h:
            lib().plk_setup_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class R1cs:
    """plk_r1cs: the constraints of a circuit on the device, for checking witnesses against them (no setup, no key; the circuit's own
    witness is not needed and the circuit may be closed afterwards).  Read-only after upload: usable from several contexts of one device."""

    def __init__(self, ctx, circuit):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().plk_r1cs_upload(ctx._h, circuit._h, ctypes.byref(self._h)))

    @property
    def num_constraints(self):
        return lib().plk_r1cs_num_constraints(self._h)

    @property
    def num_variables(self):
        return lib().plk_r1cs_num_variables(self._h)

    @staticmethod
    def _verdict(rc, valid, bad):
        _check(rc)
        return bool(valid.value), (bad.value if bad.value != 2**64 - 1 else None)

    def check(self, witness, ctx=None):
        """witness: numpy (n, 4) uint64 Montgomery Fr, n >= num_variables; wire 0 counts as 1 whatever witness[0] holds.
        Returns (valid, bad): bad is the lowest failing constraint, None when every constraint holds."""
        w = _fr_vectors([witness], "R1cs.check", allow_empty=True)[0]
        valid, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
        return self._verdict(lib().plk_r1cs_check_witness((ctx or self.ctx)._h, self._h, _np(w), ctypes.c_uint64(w.shape[0]),
                                                          ctypes.byref(valid), ctypes.byref(bad)), valid, bad)

    def check_dev(self, ptr, n, stream=None, ctx=None):
        """the same for n elements already on the device (torch tensor / int), ordered after `stream`"""
        valid, bad = ctypes.c_int32(0), ctypes.c_uint64(0)
        return self._verdict(lib().plk_r1cs_check_witness_dev((ctx or self.ctx)._h, self._h, _devptr(ptr), ctypes.c_uint64(n),
                                                              ctypes.byref(valid), ctypes.byref(bad), _stream(stream)), valid, bad)

    def last_kernel_ms(self, ctx=None):
        """HIP-event times of the last check on the context (Context.set_kernel_timing on): short LCs, long LCs, verdict, all three"""
        arr = (ctypes.c_float * 4)()
        _check(lib().plk_r1cs_last_kernel_ms((ctx or self.ctx)._h, arr))
        return dict(zip(("lc_short", "lc_long", "verdict", "kernels"), [float(x) for x in arr]))

    def close(self):
        if self._h:
            lib().plk_r1cs_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def r1cs_long_lc_terms():
    """linear combinations of at least this many terms are summed by a whole wave (diagnostic, for the tests)"""
    return int(lib().plk_r1cs_long_lc_terms())


# ------------------------------------------------------------------ CPU-only helpers of the ABI
def g1_sum_jacobian(parts):
    parts = np.ascontiguousarray(parts, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(8, dtype=np.uint64)
    _check(lib().plk_g1_sum_jacobian(_np(parts), ctypes.c_uint64(parts.shape[0]), _np(out)))
    return out


def comm_unique_id():
    """ncclGetUniqueId through the library (rank 0 calls it and hands the 128 bytes to the other ranks)"""
    out = ctypes.create_string_buffer(128)
    _check(lib().plk_comm_unique_id(out))
    return out.raw


def g1_to_bytes(p):
    p = np.ascontiguousarray(p, dtype=np.uint64)
    out = ctypes.create_string_buffer(64)
    _check(lib().plk_g1_to_bytes(_np(p), out))
    return out.raw


def g1_from_bytes(b):
    out = np.zeros(8, dtype=np.uint64)
    _check(lib().plk_g1_from_bytes(bytes(b), _np(out)))
    return out


def fr_to_bytes(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    out = ctypes.create_string_buffer(32)
    _check(lib().plk_fr_to_bytes(_np(a), out))
    return out.raw


def fr_from_bytes(b):
    out = np.zeros(4, dtype=np.uint64)
    _check(lib().plk_fr_from_bytes(bytes(b), _np(out)))
    return out


def verify(vk_bytes, proof_bytes, strict_inputs=None, transcript=None):
    """plonk::verify(&vk, &proof, "keccak") (src/plonk.rs:189-210) on the bytes of vk.bin / proof.bin; pure CPU.
    strict_inputs: None = plk_verify (accepts num_inputs = 0 unless PLK_VERIFY_STRICT_INPUTS is set); True / False = plk_verify_ex with /
    without PLK_VERIFY_STRICT_INPUTS (the Solidity verifier's `num_inputs >= 1`, contrib/template.sol:697).
    transcript: a TranscriptOps — plk_verify_with under the caller's transcript instead of Keccak."""
    valid = ctypes.c_int32(0)
    if transcript is not None:
        if strict_inputs is None:
            e = os.environ.get("PLK_VERIFY_STRICT_INPUTS", "")
            strict_inputs = bool(e) and e[0] != "0"
        table = _TranscriptTable(transcript)
        _finish(lib().plk_verify_with(bytes(vk_bytes), ctypes.c_uint64(len(vk_bytes)), bytes(proof_bytes), ctypes.c_uint64(len(proof_bytes)),
                                      ctypes.c_uint32(1 if strict_inputs else 0), ctypes.byref(table.struct), ctypes.byref(valid)), table)
    elif strict_inputs is None:
        _check(lib().plk_verify(bytes(vk_bytes), ctypes.c_uint64(len(vk_bytes)), bytes(proof_bytes), ctypes.c_uint64(len(proof_bytes)), ctypes.byref(valid)))
    else:
        _check(lib().plk_verify_ex(bytes(vk_bytes), ctypes.c_uint64(len(vk_bytes)), bytes(proof_bytes), ctypes.c_uint64(len(proof_bytes)),
                                   ctypes.c_uint32(1 if strict_inputs else 0), ctypes.byref(valid)))
    return bool(valid.value)


class VerificationKey:
    """plk_vk: a verification key resident on the GPU of `ctx` with the line table of its G2 pair (plk_vk_load); verify_many checks each
    proof exactly as `verify` does.  strict_inputs: None = as plk_verify reads the environment at load time; True / False = the flag."""

    def __init__(self, ctx, vk_bytes, strict_inputs=None):
        self._h = ctypes.c_void_p()
        self.ctx = ctx
        if strict_inputs is None:
            e = os.environ.get("PLK_VERIFY_STRICT_INPUTS", "")
            strict_inputs = bool(e) and e[0] != "0"
        _check(lib().plk_vk_load(ctx._h, bytes(vk_bytes), ctypes.c_uint64(len(vk_bytes)), ctypes.c_uint32(1 if strict_inputs else 0), ctypes.byref(self._h)))
        self.first_bad = None

    def verify_many(self, proofs, ctx=None, transcript=None):
        """numpy uint8 per proof: 1 valid, 0 invalid, 2 malformed; .first_bad = lowest index that is not 1, or None.
        transcript: a TranscriptOps — plk_verify_many_with: the host front end runs it per proof, on the calling thread"""
        proofs = [bytes(p) for p in proofs]
        n = len(proofs)
        ptrs = (ctypes.c_char_p * max(n, 1))(*proofs)
        lens = (ctypes.c_uint64 * max(n, 1))(*[len(p) for p in proofs])
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        first_bad = ctypes.c_uint64(0)
        if transcript is not None:
            table = _TranscriptTable(transcript)
            _finish(lib().plk_verify_many_with((ctx or self.ctx)._h, self._h, ptrs, lens, ctypes.c_uint64(n), ctypes.byref(table.struct), _np(verdict),
                                               ctypes.byref(first_bad)), table)
        else:
            _check(lib().plk_verify_many((ctx or self.ctx)._h, self._h, ptrs, lens, ctypes.c_uint64(n), _np(verdict), ctypes.byref(first_bad)))
        self.first_bad = None if first_bad.value == 2 ** 64 - 1 else int(first_bad.value)
        return verdict[:n]

    def verify_many_packed(self, blob, offsets, ctx=None):
        """plk_verify_many_packed: proof i = blob[offsets[i]:offsets[i + 1]]; the front end runs on the GPU.  Returns and sets .first_bad as
        verify_many; offsets that decrease or reach past the blob raise PlkError (PLK_ERR_ARG)"""
        blob = bytes(blob)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("verify_many_packed: offsets must hold count + 1 entries")
        n = off.size - 1
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        first_bad = ctypes.c_uint64(0)
        _check(lib().plk_verify_many_packed((ctx or self.ctx)._h, self._h, blob, ctypes.c_uint64(len(blob)), _np(off), ctypes.c_uint64(n), _np(verdict), ctypes.byref(first_bad)))
        self.first_bad = None if first_bad.value == 2 ** 64 - 1 else int(first_bad.value)
        return verdict[:n]

    def verify_many_dev(self, blob_tensor, offsets_tensor, stream=None, ctx=None):
        """plk_verify_many_dev: blob (uint8) and offsets (int64 / uint64, count + 1 entries) are torch tensors on the key's GPU; returns a uint8
        tensor of verdicts there, ordered on `stream` (default: the context's) — nothing passes through the host and nothing waits.  A bad
        offset pair gives that proof verdict 2"""
        import torch
        if blob_tensor.dtype != torch.uint8 or offsets_tensor.element_size() != 8 or not blob_tensor.is_contiguous() or not offsets_tensor.is_contiguous():
            raise ValueError("verify_many_dev: blob must be a contiguous uint8 tensor and offsets a contiguous 64-bit integer tensor")
        dev = (ctx or self.ctx).device
        for t in (blob_tensor, offsets_tensor):                       # a host pointer must not reach the kernel
            if not t.is_cuda or t.device.index != dev:
                raise ValueError("verify_many_dev: blob and offsets must be tensors on cuda:%d, the device of the key's context" % dev)
        n = offsets_tensor.numel() - 1
        if n < 0:
            raise ValueError("verify_many_dev: offsets must hold count + 1 entries")
        if stream is not None and hasattr(stream, "cuda_stream"):
            with torch.cuda.stream(stream):                           # the verdict tensor belongs to the stream that fills it
                verdict = torch.empty(n, dtype=torch.uint8, device=blob_tensor.device)
        else:
            verdict = torch.empty(n, dtype=torch.uint8, device=blob_tensor.device)
        _check(lib().plk_verify_many_dev((ctx or self.ctx)._h, self._h, _devptr(blob_tensor), ctypes.c_uint64(blob_tensor.numel()), _devptr(offsets_tensor),
                                         ctypes.c_uint64(n), _devptr(verdict), _stream(stream)))
        return verdict

    def close(self):
        if self._h:
            lib().plk_vk_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VerificationKeySet:
    """plk_vkset: several verification keys resident on the GPU of `ctx` as one image (plk_vkset_create); the verify_many* calls take a key
    index per proof and answer for each proof exactly as `verify` does under that key.  `keys`: VerificationKey objects (which keep their
    strict_inputs flag and may be closed afterwards) or vk bytes (loaded as VerificationKey(ctx, bytes) would)."""

    def __init__(self, ctx, keys):
        self._h = ctypes.c_void_p()
        self.ctx = ctx
        self.first_bad = None
        keys = list(keys)
        own = []
        try:
            loaded = []
            for k in keys:
                if not isinstance(k, VerificationKey):
                    k = VerificationKey(ctx, k)
                    own.append(k)
                loaded.append(k)
            arr = (ctypes.c_void_p * max(len(loaded), 1))(*[k._h.value for k in loaded])
            _check(lib().plk_vkset_create(ctx._h, arr, ctypes.c_uint32(len(loaded)), ctypes.byref(self._h)))
        finally:
            for k in own:
                k.close()

    @property
    def keys(self):
        return int(lib().plk_vkset_keys(self._h))

    @property
    def tables(self):
        """distinct G2 pairs among the keys (1: the single-key pairing kernel serves the whole set)"""
        return int(lib().plk_vkset_tables(self._h))

    @staticmethod
    def _key_of(key_of, n, who):
        k = np.asarray(key_of)
        if k.ndim != 1 or k.size != n or (k.size and (k.dtype.kind not in "iu" or k.min() < 0 or k.max() > 0xffffffff)):
            raise ValueError("%s: key_of must hold one index in [0, 2^32) per proof" % who)
        return np.ascontiguousarray(k, dtype=np.uint32)

    def verify_many(self, proofs, key_of, ctx=None):
        """plk_verify_mixed: numpy uint8 per proof (1 valid, 0 invalid, 2 malformed) under key key_of[i]; .first_bad as VerificationKey.
        An index that is not a key of the set raises PlkError (PLK_ERR_ARG)"""
        proofs = [bytes(p) for p in proofs]
        n = len(proofs)
        keys = self._key_of(key_of, n, "verify_many")
        ptrs = (ctypes.c_char_p * max(n, 1))(*proofs)
        lens = (ctypes.c_uint64 * max(n, 1))(*[len(p) for p in proofs])
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        first_bad = ctypes.c_uint64(0)
        _check(lib().plk_verify_mixed((ctx or self.ctx)._h, self._h, ptrs, lens, _np(keys), ctypes.c_uint64(n), _np(verdict), ctypes.byref(first_bad)))
        self.first_bad = None if first_bad.value == 2 ** 64 - 1 else int(first_bad.value)
        return verdict[:n]

    def verify_many_packed(self, blob, offsets, key_of, ctx=None):
        """plk_verify_mixed_packed: proof i = blob[offsets[i]:offsets[i + 1]] under key key_of[i]; the front end runs on the GPU"""
        blob = bytes(blob)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("verify_many_packed: offsets must hold count + 1 entries")
        n = off.size - 1
        keys = self._key_of(key_of, n, "verify_many_packed")
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        first_bad = ctypes.c_uint64(0)
        _check(lib().plk_verify_mixed_packed((ctx or self.ctx)._h, self._h, blob, ctypes.c_uint64(len(blob)), _np(off), _np(keys), ctypes.c_uint64(n), _np(verdict),
                                             ctypes.byref(first_bad)))
        self.first_bad = None if first_bad.value == 2 ** 64 - 1 else int(first_bad.value)
        return verdict[:n]

    def verify_many_dev(self, blob_tensor, offsets_tensor, key_of_tensor, stream=None, ctx=None):
        """plk_verify_mixed_dev: blob (uint8), offsets (64-bit integers, count + 1 entries) and key indices (32-bit integers, count entries)
        are torch tensors on the set's GPU; returns a uint8 tensor of verdicts there, ordered on `stream` — nothing passes through the host
        and nothing waits.  A key index out of range, like a bad offset pair, gives that proof verdict 2"""
        import torch
        if (blob_tensor.dtype != torch.uint8 or offsets_tensor.element_size() != 8 or key_of_tensor.element_size() != 4 or key_of_tensor.is_floating_point()
                or offsets_tensor.is_floating_point() or not blob_tensor.is_contiguous() or not offsets_tensor.is_contiguous() or not key_of_tensor.is_contiguous()):
            raise ValueError("verify_many_dev: blob must be a contiguous uint8 tensor, offsets a contiguous 64-bit and key_of a contiguous 32-bit integer tensor")
        dev = (ctx or self.ctx).device
        for t in (blob_tensor, offsets_tensor, key_of_tensor):          # a host pointer must not reach the kernel
            if not t.is_cuda or t.device.index != dev:
                raise ValueError("verify_many_dev: blob, offsets and key_of must be tensors on cuda:%d, the device of the set's context" % dev)
        n = offsets_tensor.numel() - 1
        if n < 0 or key_of_tensor.numel() != n:
            raise ValueError("verify_many_dev: offsets must hold count + 1 entries and key_of count")
        if stream is not None and hasattr(stream, "cuda_stream"):
            with torch.cuda.stream(stream):                           # the verdict tensor belongs to the stream that fills it
                verdict = torch.empty(n, dtype=torch.uint8, device=blob_tensor.device)
        else:
            verdict = torch.empty(n, dtype=torch.uint8, device=blob_tensor.device)
        _check(lib().plk_verify_mixed_dev((ctx or self.ctx)._h, self._h, _devptr(blob_tensor), ctypes.c_uint64(blob_tensor.numel()), _devptr(offsets_tensor),
                                          _devptr(key_of_tensor), ctypes.c_uint64(n), _devptr(verdict), _stream(stream)))
        return verdict

    def close(self):
        if self._h:
            lib().plk_vkset_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_terms(vk_bytes, proof_bytes, strict_inputs=False, transcript=None):
    """plk_verify_terms: (points [25, 8] uint64 Montgomery affine, scalars [25, 4] uint64 Montgomery, early).  pg = sum of terms 0..22,
    px = terms 23 + 24; early False: already invalid without group arithmetic.  Pure CPU.
    transcript: a TranscriptOps — plk_verify_terms_with under the caller's transcript."""
    pts = np.zeros((25, 8), dtype=np.uint64)
    sc = np.zeros((25, 4), dtype=np.uint64)
    early = ctypes.c_int32(0)
    if transcript is not None:
        table = _TranscriptTable(transcript)
        _finish(lib().plk_verify_terms_with(bytes(vk_bytes), ctypes.c_uint64(len(vk_bytes)), bytes(proof_bytes), ctypes.c_uint64(len(proof_bytes)),
                                            ctypes.c_uint32(1 if strict_inputs else 0), ctypes.byref(table.struct), _np(pts), _np(sc),
                                            ctypes.byref(early)), table)
    else:
        _check(lib().plk_verify_terms(bytes(vk_bytes), ctypes.c_uint64(len(vk_bytes)), bytes(proof_bytes), ctypes.c_uint64(len(proof_bytes)),
                                      ctypes.c_uint32(1 if strict_inputs else 0), _np(pts), _np(sc), ctypes.byref(early)))
    return pts, sc, bool(early.value)


def pairing_check(a, g2_a, b, g2_b):
    """e(a, g2_a) * e(b, g2_b) == 1 ; G1 as 8 x u64 Montgomery affine, G2 as the 128-byte file encoding"""
    out = ctypes.c_int32(0)
    a = np.ascontiguousarray(a, dtype=np.uint64); b = np.ascontiguousarray(b, dtype=np.uint64)
    _check(lib().plk_pairing_check(_np(a), bytes(g2_a), _np(b), bytes(g2_b), ctypes.byref(out)))
    return bool(out.value)


def kzg_verify(commitments, z, evals, proof, g2_bytes, v=None):
    """plk_kzg_verify (pure CPU): is `proof` an opening of the commitments ([count, 8]) at z to evals ([count, 4]), combined by powers of v
    (None allowed for one commitment)?  g2_bytes: the 256 bytes of the key file's G2 section.  Malformed input raises PlkError."""
    c = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
    e = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
    if c.shape[0] != e.shape[0]:
        raise ValueError("kzg_verify: %d commitments and %d evaluations" % (c.shape[0], e.shape[0]))
    g2_bytes = bytes(g2_bytes)
    if len(g2_bytes) != 256:
        raise ValueError("g2_bytes must be the 256 bytes of a key file's G2 section, got %d" % len(g2_bytes))
    z = np.ascontiguousarray(z, dtype=np.uint64)
    v = np.ascontiguousarray(v, dtype=np.uint64) if v is not None else None
    p = np.ascontiguousarray(proof, dtype=np.uint64)
    out = ctypes.c_int32(0)
    _check(lib().plk_kzg_verify(_np(c), ctypes.c_uint32(c.shape[0]), _np(z), _np(e), _np(v) if v is not None else None, _np(p), g2_bytes, ctypes.byref(out)))
    return bool(out.value)


def kzg_verify_multi(commitments, points, sets, evals, gamma, u, proof, g2_bytes):
    """plk_kzg_verify_multi (pure CPU): is proof ([2, 8]: W, W') an opening of the commitments ([count, 8]), commitment i at the points
    ([npoints, 4]) named by the bits of sets[i], to evals ([count, npoints, 4]; entries outside a set are not read), under the batching
    challenge gamma and the evaluation challenge u?  g2_bytes: the 256 bytes of the key file's G2 section.  Malformed input raises PlkError."""
    c = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
    masks = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1)
    e = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
    if masks.shape[0] != c.shape[0] or e.shape[0] != c.shape[0] * pts.shape[0]:
        raise ValueError("kzg_verify_multi: %d commitments and %d points need %d sets and %d evaluations, got %d and %d"
                         % (c.shape[0], pts.shape[0], c.shape[0], c.shape[0] * pts.shape[0], masks.shape[0], e.shape[0]))
    g2_bytes = bytes(g2_bytes)
    if len(g2_bytes) != 256:
        raise ValueError("g2_bytes must be the 256 bytes of a key file's G2 section, got %d" % len(g2_bytes))
    gamma, u = np.ascontiguousarray(gamma, dtype=np.uint64), np.ascontiguousarray(u, dtype=np.uint64)
    p = np.ascontiguousarray(proof, dtype=np.uint64).reshape(2, 8)
    out = ctypes.c_int32(0)
    _check(lib().plk_kzg_verify_multi(_np(c), ctypes.c_uint32(c.shape[0]), _np(pts), ctypes.c_uint32(pts.shape[0]), _np(masks), _np(e), _np(gamma), _np(u), _np(p),
                                      g2_bytes, ctypes.byref(out)))
    return bool(out.value)


UPDATE_REASONS = ("ok", "bad_g2", "q0_changed", "p0_changed", "bad_s1", "bad_s2", "receipt_split", "p1_mismatch", "q1_mismatch",
                  "key_structure")                                  # PLK_UPDATE_*


def _update_bytes(g2_old, g2_new, receipt):
    g2_old, g2_new, receipt = bytes(g2_old), bytes(g2_new), bytes(receipt)
    if len(g2_old) != 256 or len(g2_new) != 256 or len(receipt) != 192:
        raise ValueError("a G2 section is 256 bytes and a receipt 192, got %d, %d and %d" % (len(g2_old), len(g2_new), len(receipt)))
    return g2_old, g2_new, receipt


def srs_update_receipt(s, g2_old):
    """the host half of Context.srs_update for a given s (4 x uint64 Montgomery Fr): (g2_new, receipt).  Pure CPU."""
    g2_old = bytes(g2_old)
    if len(g2_old) != 256:
        raise ValueError("g2_old must be the 256 bytes of a key file's G2 section, got %d" % len(g2_old))
    sv = np.ascontiguousarray(s, dtype=np.uint64).reshape(4) if s is not None else None
    g2_new, receipt = ctypes.create_string_buffer(256), ctypes.create_string_buffer(192)
    _check(lib().plk_srs_update_receipt(_np(sv) if sv is not None else None, g2_old, g2_new, receipt))
    return g2_new.raw, receipt.raw


def srs_update_check_receipt(old_p01, new_p01, g2_old, g2_new, receipt):
    """the host half of Context.srs_update_verify: every rule but the key's own structure check, given points 0 and 1 of the old and
    of the new key ([2, 8] uint64 each; [1, 8] for a one-point key).  Returns (valid, reason).  Pure CPU."""
    o = np.ascontiguousarray(old_p01, dtype=np.uint64).reshape(-1, 8)
    n = np.ascontiguousarray(new_p01, dtype=np.uint64).reshape(-1, 8)
    points = min(2, o.shape[0], n.shape[0])
    g2_old, g2_new, receipt = _update_bytes(g2_old, g2_new, receipt)
    valid, reason = ctypes.c_int32(0), ctypes.c_uint32(0)
    _check(lib().plk_srs_update_check_receipt(_np(o), _np(n), ctypes.c_uint32(points), g2_old, g2_new, receipt, ctypes.byref(valid), ctypes.byref(reason)))
    return bool(valid.value), UPDATE_REASONS[reason.value]


def crs42_g2_bytes():
    out = ctypes.create_string_buffer(256)
    lib().plk_crs42_g2_bytes(out)
    return out.raw


def keccak256(data):
    out = ctypes.create_string_buffer(32)
    lib().plk_keccak256(bytes(data), ctypes.c_uint64(len(data)), out)
    return out.raw


class _TranscriptStruct(ctypes.Structure):
    _fields_ = [("state0", ctypes.c_uint8 * 32), ("state1", ctypes.c_uint8 * 32), ("counter", ctypes.c_uint32)]


class Transcript:
    """RollingKeccakTranscript (src/plonk.rs:10; contrib/template.sol:267-307)."""

    def __init__(self):
        self._t = _TranscriptStruct()
        lib().plk_transcript_init(ctypes.byref(self._t))

    def absorb_fr(self, a):
        lib().plk_transcript_absorb_fr(ctypes.byref(self._t), _np(np.ascontiguousarray(a, dtype=np.uint64)))

    def absorb_g1(self, p):
        lib().plk_transcript_absorb_g1(ctypes.byref(self._t), _np(np.ascontiguousarray(p, dtype=np.uint64)))

    def challenge(self):
        out = np.zeros(4, dtype=np.uint64)
        lib().plk_transcript_challenge(ctypes.byref(self._t), _np(out))
        return out
