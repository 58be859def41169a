"""ctypes binding of csrc/libcsmp.so -- the C ABI declared in include/csmp.h.

This is the Python twin of the `ccall` stubs in julia/CompressedSensingAMD.jl.  There is NO CPU
fallback: if the shared library is missing, or no MI355X is visible, every compute entry point
raises `CsmpError` loudly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libcsmp.so")

OK, EINVAL, EDIM, ERANGE, EHIP, ESTATE, ENOMEM, ERCCL, EIO = 0, -1, -2, -3, -4, -5, -6, -7, -8
F32, F64 = 0, 1
HOST, DEVICE, HOST_STREAMED = 0, 1, 2
ALGO_MP, ALGO_OMP, ALGO_GOMP, ALGO_FR, ALGO_SP, ALGO_OMPR = 0, 1, 2, 3, 4, 5
STOP_EPS, STOP_STAG, STOP_FULL = 1, 2, 4
# csmp_set_option keys (include/csmp.h)
OPT_BATCH_CERT, OPT_BATCH_GRAM, OPT_BATCH_WINDOW, OPT_PIPELINE, OPT_SOLVES_IN_FLIGHT, OPT_SCREENED_SWEEP, OPT_BATCH_SCREEN = 1, 2, 3, 4, 9, 10, 11
OPTIONS = {"batch_cert": OPT_BATCH_CERT, "batch_gram": OPT_BATCH_GRAM, "batch_window": OPT_BATCH_WINDOW, "pipeline": OPT_PIPELINE,
           "solves_in_flight": OPT_SOLVES_IN_FLIGHT, "screened_sweep": OPT_SCREENED_SWEEP, "batch_screen": OPT_BATCH_SCREEN}

i64 = C.c_int64
vp = C.c_void_p

# name -> (restype, argtypes): every symbol include/csmp.h declares
SIGNATURES = {
    "csmp_version": (C.c_int, []),
    "csmp_create": (C.c_int, [C.POINTER(vp), C.c_int]),
    "csmp_destroy": (C.c_int, [vp]),
    "csmp_last_error": (C.c_char_p, [vp]),
    "csmp_set_stream": (C.c_int, [vp, vp]),
    "csmp_sync": (C.c_int, [vp]),
    "csmp_device_info": (C.c_int, [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(i64)]),
    "csmp_set_dictionary": (C.c_int, [vp, vp, i64, i64, i64, C.c_int, C.c_int]),
    "csmp_dictionary_file_write": (C.c_int, [C.c_char_p, vp, i64, i64, i64, C.c_int]),
    "csmp_dictionary_file_info": (C.c_int, [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int)]),
    "csmp_set_dictionary_file": (C.c_int, [vp, C.c_char_p, C.c_int]),
    "csmp_clone": (C.c_int, [vp, C.POINTER(vp)]),
    "csmp_shard_config": (C.c_int, [vp, i64]),
    "csmp_shard_record_bytes": (i64, [vp]),
    "csmp_shard_sweep": (C.c_int, [vp, C.c_double, C.c_int, vp]),
    "csmp_shard_append": (C.c_int, [vp, vp, C.c_int]),
    "csmp_shard_range": (C.c_int, [i64, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]),
    "csmp_comm_id": (C.c_int, [vp]),
    "csmp_comm_init": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "csmp_comm_free": (C.c_int, [vp]),
    "csmp_omp_sharded": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, C.c_double, C.c_int, vp, vp, vp, C.c_int]),
    "csmp_pack_block_device": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp]),
    "csmp_unpack_gathered_device": (C.c_int, [vp, vp, i64, i64, C.c_int, vp, vp, vp]),
    "csmp_pack_results": (C.c_int, [vp, vp, vp, i64, i64, vp]),
    "csmp_unpack_results": (C.c_int, [vp, i64, i64, vp, vp, vp]),
    "csmp_mp": (C.c_int, [vp, vp, C.c_int, i64, vp, vp, i64, vp, vp, C.POINTER(i64)]),
    "csmp_omp": (C.c_int, [vp, vp, C.c_int, i64, C.c_double, vp, vp, C.POINTER(i64), vp]),
    "csmp_gomp": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_double, vp, vp, C.POINTER(i64), vp]),
    "csmp_sp": (C.c_int, [vp, vp, C.c_int, i64, C.c_double, i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]),
    "csmp_fr": (C.c_int, [vp, vp, C.c_int, i64, C.c_double, C.c_double, vp, vp, C.POINTER(i64), vp]),
    "csmp_fr_scores": (C.c_int, [vp, vp]),
    "csmp_srr": (C.c_int, [vp, vp, C.c_int, i64, C.c_double, i64, C.c_int, i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]),
    "csmp_srr_from": (C.c_int, [vp, vp, C.c_int, i64, C.c_double, i64, vp, i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]),
    "csmp_rmp_delta": (C.c_int, [vp, vp, C.c_int, C.c_double, i64, i64, vp, vp, C.POINTER(i64)]),
    "csmp_rmp_k": (C.c_int, [vp, vp, C.c_int, i64, i64, vp, vp, C.POINTER(i64)]),
    "csmp_foba": (C.c_int, [vp, vp, C.c_int, C.c_double, i64, vp, vp, C.POINTER(i64)]),
    "csmp_br": (C.c_int, [vp, vp, C.c_int, C.c_double, C.c_double, i64, C.c_int, vp, vp, C.POINTER(i64)]),
    "csmp_fr_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, C.c_double, C.c_double, vp, vp, vp, C.c_int]),
    "csmp_mp_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, vp, vp, vp, C.c_int]),
    "csmp_somp": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, C.c_double, C.c_int, vp, vp, i64, C.POINTER(i64), vp, vp, C.POINTER(i64),
                            C.c_int]),
    "csmp_ompr": (C.c_int, [vp, vp, C.c_int, i64, C.c_double, i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]),
    "csmp_omp_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, C.c_double, vp, vp, vp, C.c_int]),
    "csmp_gomp_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, i64, C.c_double, vp, vp, vp, C.c_int]),
    "csmp_sp_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, i64, C.c_double, i64, vp, vp, vp, vp]),
    "csmp_omp_batch_mfma": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, C.c_double, vp, vp, vp, C.c_int]),
    "csmp_batch_stats": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                   C.POINTER(C.c_double)]),
    "csmp_screened_stats": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), C.c_int]),
    "csmp_set_option": (C.c_int, [vp, C.c_int, i64]),
    "csmp_get_option": (C.c_int, [vp, C.c_int, C.POINTER(i64)]),
    "csmp_solver_begin": (C.c_int, [vp, C.c_int, vp, C.c_int, i64, vp, vp, i64]),
    "csmp_solver_step": (C.c_int, [vp, i64]),
    "csmp_solver_acquire": (C.c_int, [vp, i64]),
    "csmp_solver_remove": (C.c_int, [vp, i64]),
    "csmp_solver_state": (C.c_int, [vp, vp, vp, C.POINTER(i64), C.POINTER(C.c_double), vp, C.POINTER(C.c_int)]),
    "csmp_ista": (C.c_int, [vp, vp, C.c_int, vp, i64, vp, vp, i64, i64, C.c_double, C.c_int, vp, C.c_int, C.POINTER(C.c_double)]),
    "csmp_ista_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, i64, vp, i64, i64, C.c_double, C.c_int, vp, i64, C.c_int,
                                  C.POINTER(C.c_double)]),
    "csmp_ista_joint": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, vp, i64, i64, C.c_double, C.c_int, vp, i64, C.c_int,
                                  C.POINTER(i64), C.POINTER(C.c_double)]),
    "csmp_ard_weights": (C.c_int, [vp, vp, vp, C.c_double, i64, vp, C.c_int]),
    "csmp_ista_reweighted": (C.c_int, [vp, vp, C.c_int, C.c_double, C.c_int, C.c_double, i64, i64, C.c_double, i64, C.c_double, C.c_int, vp, C.c_int, vp,
                                       C.POINTER(i64), C.POINTER(C.c_double)]),
    "csmp_bp": (C.c_int, [vp, vp, C.c_int, vp, i64, C.c_double, i64, C.c_double, i64, vp, C.c_int, C.POINTER(i64), C.POINTER(C.c_double),
                          C.POINTER(C.c_int)]),
    "csmp_bp_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, C.c_double, i64, C.c_double, i64, vp, i64, C.c_int, C.POINTER(i64),
                                C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "csmp_bp_joint": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, C.c_double, i64, C.c_double, i64, vp, i64, C.c_int, C.POINTER(i64),
                                C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "csmp_bp_reweighted": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_double, i64, i64, C.c_double, C.c_double, i64, C.c_double, i64, vp, C.c_int, vp,
                                     C.POINTER(i64), C.POINTER(C.c_double)]),
    "csmp_bpd": (C.c_int, [vp, vp, C.c_int, C.c_double, vp, i64, C.c_double, i64, C.c_double, i64, vp, C.c_int, C.POINTER(i64), C.POINTER(C.c_double),
                           C.POINTER(C.c_int)]),
    "csmp_bpd_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, vp, i64, C.c_double, i64, C.c_double, i64, vp, i64, C.c_int,
                                 C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "csmp_bpd_reweighted": (C.c_int, [vp, vp, C.c_int, C.c_double, C.c_int, C.c_double, i64, i64, C.c_double, C.c_double, i64, C.c_double, i64, vp, C.c_int,
                                      vp, C.POINTER(i64), C.POINTER(C.c_double)]),
    "csmp_sbl": (C.c_int, [vp, vp, C.c_int, C.c_double, i64, C.c_double, vp, vp, vp, C.c_int, C.POINTER(i64), C.POINTER(C.c_int)]),
    "csmp_fsbl": (C.c_int, [vp, vp, C.c_int, C.c_double, i64, C.c_double, vp, vp, vp, C.c_int, vp, i64, C.POINTER(i64), C.POINTER(C.c_int)]),
    "csmp_rmps": (C.c_int, [vp, vp, C.c_int, C.c_double, i64, i64, i64, C.c_double, vp, vp, vp, C.c_int, vp, i64, C.POINTER(i64),
                            C.POINTER(C.c_int)]),
    "csmp_fsbl_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, i64, C.c_double, vp, i64, vp, i64, vp, i64, C.c_int, vp, i64,
                                  C.POINTER(i64), C.POINTER(C.c_int)]),
    "csmp_rmps_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, i64, i64, i64, C.c_double, vp, i64, vp, i64, vp, i64, C.c_int, vp,
                                  i64, C.POINTER(i64), C.POINTER(C.c_int)]),
    "csmp_ompr_batch": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, i64, C.POINTER(C.c_double), i64, i64, vp, vp, vp, C.POINTER(i64),
                                  C.POINTER(C.c_int)]),
    "csmp_colnorms": (C.c_int, [vp, vp, C.c_int]),
    "csmp_cumbabel": (C.c_int, [vp, i64, C.c_int, vp, vp]),
    "csmp_sweep": (C.c_int, [vp, vp, vp, i64, vp, vp]),
    "csmp_lstsq": (C.c_int, [vp, vp, i64, vp, C.c_int, vp]),
}


# measurement and test hooks: include/csmp_internal.h (not part of the drop-in boundary)
INTERNAL_SIGNATURES = {
    "csmp_profile_enable": (C.c_int, [vp, C.c_int]),
    "csmp_profile_read": (C.c_int, [vp, C.POINTER(i64), C.POINTER(C.c_double), C.c_int]),
    "csmp_bench_sweep": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "csmp_bench_ard_forms": (C.c_int, [vp, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "csmp_bp_rowgram": (C.c_int, [vp, vp, C.c_int]),
    "csmp_sbl_rowgram": (C.c_int, [vp, vp, vp, C.c_int]),
    "csmp_sbl_forms": (C.c_int, [vp, vp, i64, vp, vp, vp, C.c_int]),
    "csmp_bench_sbl": (C.c_int, [vp, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "csmp_fsbl_score": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "csmp_fsbl_sqc": (C.c_int, [vp, vp, vp, vp, i64, C.c_double]),
    "csmp_bench_fsbl": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "csmp_profile_overhead": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
    "csmp_live_resources": (C.c_int, [C.POINTER(i64)] * 6),
    "csmp_profile_window": (C.c_int, [vp, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "csmp_sweep_config": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "csmp_sweep_group": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "csmp_sweep_group_wide": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "csmp_tune": (C.c_int, [vp, C.c_int, i64]),
    "csmp_batch_layout": (C.c_int, [vp, C.POINTER(i64), C.POINTER(C.c_int)]),
    "csmp_batch_screen_kernel": (C.c_char_p, [vp]),
}
TUNE = {"sweep_grid": 2, "sweep_unit": 3, "tick_grid": 4, "batch_budget_mib": 5, "diag_split": 6, "swap_refuse": 7, "rebuild_direct": 8, "sweep_dyn": 9, "tick_order": 10, "claim_pools": 11, "pipelines": 12, "pair_lds_kib": 13, "pair_split": 14, "sweep_lds_kib": 15, "sweep_short": 16, "phase_rows": 17, "fail_alloc": 18, "screen_static": 19, "group_max": 20, "group_wide": 21, "rowgram_scalar": 22, "pass_c": 23, "group_split": 24, "sbl_scalar": 25, "fsbl_scalar": 26}  # CSMP_TUNE_* (include/csmp_internal.h)

COMM_ID_BYTES = 128  # CSMP_COMM_ID_BYTES
BABEL_KMAX = 1024  # CSMP_BABEL_KMAX
ARD_KMAX = 1024  # CSMP_ARD_KMAX
REWEIGHT_CANDES, REWEIGHT_ARD = 0, 1  # CSMP_REWEIGHT_*
BP_CONVERGED, BP_FACTORED = 1, 2  # CSMP_BP_*
BPD_CONVERGED, BPD_FACTORED = 1, 2  # CSMP_BPD_*
BPD_RHO = 100.0  # the bindings' default penalty of bpd
SBL_CONVERGED = 1  # CSMP_SBL_*
FSBL_CONVERGED = RMPS_CONVERGED = 1  # CSMP_FSBL_*, CSMP_RMPS_*
OMPR_SOLVED_ALONE = 1  # CSMP_OMPR_SOLVED_ALONE
FSBL_MODES = {"all": 1, "add": 2, "rmp_delete": 3, "update": 4}  # csmp_fsbl_score's modes


def live_resources():
    """what the library holds right now, process-wide (csmp_internal.h): all zero when no context exists"""
    v = [i64(0) for _ in range(6)]
    rc = lib().csmp_live_resources(*[C.byref(x) for x in v])
    if rc != OK:
        raise CsmpError(rc, "csmp_live_resources")
    return dict(zip(("device_bytes", "device_blocks", "pinned_bytes", "registered_ranges", "events", "streams"), (int(x.value) for x in v)))


def comm_id():
    """rank 0: a fresh RCCL communicator id (bytes) to hand to every rank's Context.comm_init."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().csmp_comm_id(C.cast(buf, vp))
    if rc != 0:
        raise CsmpError(rc, lib().csmp_last_error(None).decode())
    return buf.raw


def write_dictionary_file(path, A):
    """A (numpy, M x N, float32 / float64) -> a dictionary file (include/csmp.h: 64-byte header + the columns padded to 16 bytes).
    Host only: no GPU is touched."""
    A = np.asarray(A)
    if A.ndim != 2 or A.dtype not in (np.float32, np.float64):
        raise ValueError("A must be a float32 or float64 matrix")
    if not A.flags.f_contiguous:
        A = np.asfortranarray(A)
    M, N = A.shape
    rc = lib().csmp_dictionary_file_write(os.fsencode(path), ptr(A), i64(M), i64(N), i64(M), dtype_code(A.dtype))
    if rc != 0:
        raise CsmpError(rc, f"cannot write {path}")


def dictionary_file_info(path):
    """(M, N, numpy dtype) of a dictionary file."""
    M, N, dt = i64(0), i64(0), C.c_int(0)
    rc = lib().csmp_dictionary_file_info(os.fsencode(path), C.byref(M), C.byref(N), C.byref(dt))
    if rc != 0:
        raise CsmpError(rc, f"{path} is not a dictionary file")
    return int(M.value), int(N.value), (np.float32 if dt.value == dtype_code(np.dtype(np.float32)) else np.float64)


class CsmpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcsmp error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libcsmp.so (built by `make -C csrc` / __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CsmpError(ESTATE, f"{LIB_PATH} is missing -- build it with `make -C {os.path.dirname(LIB_PATH)}`; "
                                    "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(INTERNAL_SIGNATURES.items()):
            f = getattr(L, name)  # AttributeError if the ABI and the header disagree
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.float32:
        return F32
    if dt == np.float64:
        return F64
    raise TypeError(f"unsupported element type {dt}: the dictionary and b must be float32 or float64")


def _scheme(scheme):
    return {"candes": REWEIGHT_CANDES, "ard": REWEIGHT_ARD}.get(scheme, scheme)


def ista_batch_weights(w, N, nsig):
    """The weights of an ista batch as csmp_ista_batch takes them: (Float64 array in Fortran order, nw, ldw).  A scalar and an
    N-vector are shared by all signals (ldw = 0); an nsig-vector is one lambda per signal (nw = 1, ldw = 1); an N x nsig matrix one
    weight vector per signal.  With nsig == N a vector is the shared N-vector.  ValueError: any other shape."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim == 0 or w.shape == (1,):
        return np.ascontiguousarray(w.reshape(1)), 1, 0
    if w.shape == (N,):
        return np.ascontiguousarray(w), N, 0
    if w.shape == (nsig,):
        return np.ascontiguousarray(w), 1, 1
    if w.shape == (N, nsig):
        return np.asfortranarray(w), N, max(N, 1)
    raise ValueError(f"size(w) = {w.shape}: the weights are a scalar, {nsig} (one per signal), {N} (one per atom) or {(N, nsig)} numbers")


class Context:
    """One GPU + one HIP stream + the resident dictionary (csmp_ctx)."""
    last_status = OK  # status of the most recent call

    def __init__(self, device=0):
        self._h = vp()
        L = lib()
        rc = L.csmp_create(C.byref(self._h), int(device))
        if rc != OK:
            msg = L.csmp_last_error(None).decode()
            self._h = None
            raise CsmpError(rc, msg)
        self.M = self.N = 0
        self.dtype = None
        self._keep = None  # keeps a borrowed device tensor alive

    def close(self):
        if getattr(self, "_h", None):
            lib().csmp_destroy(self._h)
            self._h = None
        self._parent = None

    def clone(self):
        """A second context on the same GPU borrowing this one's resident dictionary (csmp_clone): what every
        step-level functor works on, so that two of them never share solver state."""
        c = Context.__new__(Context)
        c._h = vp()
        c.M, c.N, c.dtype, c._keep = self.M, self.N, self.dtype, self._keep
        c._parent = self  # the borrowed dictionary must outlive the clone
        rc = lib().csmp_clone(self._h, C.byref(c._h))
        if rc != OK:
            c._h = None
            self.check(rc)
        return c

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        self.last_status = rc
        if rc < OK:
            raise CsmpError(rc, lib().csmp_last_error(self._h).decode())

    def call(self, name, *args):
        self.check(getattr(lib(), name)(self._h, *args))

    # ---- dictionary
    def set_dictionary(self, A, streamed=False):
        """A: numpy array (host; copied once to HBM) or a torch CUDA tensor holding the
        column-major dictionary as a (N, M) row-major tensor, i.e. `A_torch[j]` is atom j.
        streamed=True (numpy only): A stays in host memory, mapped into the device; every sweep crosses the host link
        (CSMP_HOST_STREAMED: for a dictionary larger than HBM).  The array is kept alive by this object."""
        if isinstance(A, np.ndarray):
            if A.ndim != 2:
                raise ValueError("A must be a matrix")
            if not A.flags.f_contiguous:
                A = np.asfortranarray(A)
            M, N = A.shape
            self.call("csmp_set_dictionary", ptr(A), i64(M), i64(N), i64(M), dtype_code(A.dtype), HOST_STREAMED if streamed else HOST)
            self.dtype = A.dtype
            self._keep = A if streamed else None
        else:  # torch tensor on the GPU, shape (N, M): rows are atoms
            import torch
            if not (isinstance(A, torch.Tensor) and A.is_cuda and A.dim() == 2 and A.is_contiguous()):
                raise ValueError("device dictionary must be a contiguous 2-D CUDA tensor of shape (N atoms, M rows)")
            N, M = A.shape
            dt = np.float32 if A.dtype == torch.float32 else np.float64 if A.dtype == torch.float64 else None
            if dt is None:
                raise TypeError("device dictionary must be float32 or float64")
            self.call("csmp_set_dictionary", vp(A.data_ptr()), i64(M), i64(N), i64(M), dtype_code(dt), DEVICE)
            self.dtype = np.dtype(dt)
            self._keep = A
        self.M, self.N = int(M), int(N)

    def set_dictionary_file(self, path, streamed=False):
        """A dictionary file (write_dictionary_file) read to where it will live: HBM, or mapped host memory (streamed=True)."""
        M, N, dt = dictionary_file_info(path)
        self.call("csmp_set_dictionary_file", os.fsencode(path), HOST_STREAMED if streamed else DEVICE)
        self.dtype = np.dtype(dt)
        self._keep = None
        self.M, self.N = M, N

    def sync(self):
        self.call("csmp_sync")

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int(0)
        mem = i64(0)
        self.call("csmp_device_info", name, 256, C.byref(cus), C.byref(mem))
        return name.value.decode(), cus.value, mem.value

    def _b(self, b):
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(np.float64)
        if b.shape != (self.M,):
            raise CsmpError(EDIM, f"length(b) = {b.shape} but size(A, 1) = {self.M}")
        return b

    # ---- drivers
    def omp(self, b, k, eps):
        b = self._b(b)
        cap = max(int(k), 1)
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        order = np.zeros(cap, np.int64)
        nnz = i64(0)
        self.call("csmp_omp", ptr(b), dtype_code(b.dtype), i64(int(k)), C.c_double(eps), ptr(idx), ptr(val),
                  C.byref(nnz), ptr(order))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), order[:n].copy()

    def gomp(self, b, l, k, eps):
        b = self._b(b)
        cap = max(int(k) + int(l), 1)
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        order = np.zeros(cap, np.int64)
        nnz = i64(0)
        self.call("csmp_gomp", ptr(b), dtype_code(b.dtype), i64(int(l)), i64(int(k)), C.c_double(eps), ptr(idx),
                  ptr(val), C.byref(nnz), ptr(order))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), order[:n].copy()

    def mp(self, b, k, idx0=None, val0=None):
        b = self._b(b)
        idx0 = np.zeros(0, np.int64) if idx0 is None else np.ascontiguousarray(idx0, dtype=np.int64)
        val0 = np.zeros(0, np.float64) if val0 is None else np.ascontiguousarray(val0, dtype=np.float64)
        cap = max(int(k) + len(idx0), 1)
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        nnz = i64(0)
        self.call("csmp_mp", ptr(b), dtype_code(b.dtype), i64(int(k)), ptr(idx0), ptr(val0), i64(len(idx0)),
                  ptr(idx), ptr(val), C.byref(nnz))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy()

    def sp(self, b, k, delta, maxiter=-1):
        b = self._b(b)
        cap = max(2 * int(k), 1)
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        nnz = i64(0)
        iters = i64(0)
        self.call("csmp_sp", ptr(b), dtype_code(b.dtype), i64(int(k)), C.c_double(delta), i64(int(maxiter)),
                  ptr(idx), ptr(val), C.byref(nnz), C.byref(iters))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), iters.value

    def ompr(self, b, k, delta, maxiter=-1):
        b = self._b(b)
        idx = np.zeros(max(int(k), 1), np.int64)
        val = np.zeros(max(int(k), 1), np.float64)
        nnz = i64(0)
        iters = i64(0)
        self.call("csmp_ompr", ptr(b), dtype_code(b.dtype), i64(int(k)), C.c_double(delta), i64(int(maxiter)),
                  ptr(idx), ptr(val), C.byref(nnz), C.byref(iters))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), iters.value

    def _ompr_batch_call(self, B, code, ldB, nsig, b_loc, k, delta, maxiter):
        """csmp_ompr_batch: the outputs live on the host whatever b_loc is -> (idx k x nsig, val, nnz, info)"""
        d = np.ascontiguousarray(np.atleast_1d(np.asarray(delta, dtype=np.float64)))
        if d.ndim != 1:
            raise CsmpError(EDIM, "delta has to be a scalar or one value per signal")
        kk = max(int(k), 1)
        idx = np.zeros((kk, max(nsig, 1)), np.int64, order="F")
        val = np.zeros((kk, max(nsig, 1)), np.float64, order="F")
        nnz, it, fl = np.zeros(max(nsig, 1), np.int64), np.zeros(max(nsig, 1), np.int64), np.zeros(max(nsig, 1), np.int32)
        self.call("csmp_ompr_batch", B, code, i64(ldB), i64(nsig), b_loc, i64(int(k)), d.ctypes.data_as(C.POINTER(C.c_double)), i64(len(d)),
                  i64(-1 if maxiter is None else int(maxiter)), ptr(idx), ptr(val), ptr(nnz), it.ctypes.data_as(C.POINTER(i64)),
                  fl.ctypes.data_as(C.POINTER(C.c_int)))
        info = {"iterations": it[:nsig], "solved_alone": (fl[:nsig] & OMPR_SOLVED_ALONE) != 0}
        return idx[:, :nsig], val[:, :nsig], nnz[:nsig], info

    def ompr_batch(self, B, k, delta, maxiter=None):
        """csmp_ompr_batch on the host matrix B (M x nsig): ompr for every column, the update!s of a group's signals in lockstep on shared
        launches -> (idx k x nsig, val, nnz, info = iterations int64[nsig], solved_alone bool[nsig]).  Column s is ompr(B[:, s], k,
        delta_s, maxiter)'s bit for bit.  delta: a scalar or one value per signal; maxiter=None: size(A, 1)."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        return self._ompr_batch_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), B.shape[1], HOST, k, delta, maxiter)

    def ompr_batch_device(self, B, k, delta, maxiter=None):
        """as ompr_batch, on a torch CUDA matrix whose COLUMNS are the signals: B (M, nsig) float32 / float64 with stride (1, ldB >= M).
        The results come back as ompr_batch's host arrays; the work is done when the call returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        if (self.M > 1 and B.stride(0) != 1) or ldB < self.M:
            raise CsmpError(EDIM, "B must be column-major: unit row stride, a column stride of at least its row count")
        return self._ompr_batch_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, k, delta, maxiter)

    def fr(self, b, k, max_eps=0.0, min_delta=0.0):
        b = self._b(b)
        cap = max(int(k), 1)
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        order = np.zeros(cap, np.int64)
        nnz = i64(0)
        self.call("csmp_fr", ptr(b), dtype_code(b.dtype), i64(int(k)), C.c_double(max_eps), C.c_double(min_delta),
                  ptr(idx), ptr(val), C.byref(nnz), ptr(order))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), order[:n].copy()

    def srr(self, b, k, delta=1e-12, maxiter=-1, initialization=1, l=1, init=None):
        b = self._b(b)
        cap = int(k) + int(l) + 1
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        nnz = i64(0)
        iters = i64(0)
        if int(initialization) == 3 and init is not None:  # (without a draw: csmp_srr refuses initialization 3 itself)
            init = np.ascontiguousarray(init, np.int64)
            if init.size != int(k):
                raise ValueError("srr: initialization = 3 needs k initial atoms")
            self.call("csmp_srr_from", ptr(b), dtype_code(b.dtype), i64(int(k)), C.c_double(delta), i64(int(maxiter)),
                      ptr(init), i64(int(l)), ptr(idx), ptr(val), C.byref(nnz), C.byref(iters))
            n = nnz.value
            return idx[:n].copy(), val[:n].copy(), iters.value
        self.call("csmp_srr", ptr(b), dtype_code(b.dtype), i64(int(k)), C.c_double(delta), i64(int(maxiter)),
                  int(initialization), i64(int(l)), ptr(idx), ptr(val), C.byref(nnz), C.byref(iters))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), iters.value

    def _stepwise_cap(self, kmax):
        lim = min(self.M, self.N, 4095)
        return lim if kmax is None or kmax <= 0 else min(int(kmax), lim)

    def rmp(self, b, delta_or_k, maxiter=1, kmax=None):
        """rmp(A,b,δ,maxiter) for a float second argument, rmp(A,b,k) for an int."""
        b = self._b(b)
        cap = self._stepwise_cap(kmax)
        idx = np.zeros(cap + 1, np.int64)
        val = np.zeros(cap + 1, np.float64)
        nnz = i64(0)
        if isinstance(delta_or_k, (int, np.integer)):
            self.call("csmp_rmp_k", ptr(b), dtype_code(b.dtype), i64(int(delta_or_k)), i64(cap), ptr(idx), ptr(val), C.byref(nnz))
        else:
            self.call("csmp_rmp_delta", ptr(b), dtype_code(b.dtype), C.c_double(float(delta_or_k)), i64(int(maxiter)), i64(cap),
                      ptr(idx), ptr(val), C.byref(nnz))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy()

    def foba(self, b, delta, kmax=None):
        b = self._b(b)
        cap = self._stepwise_cap(kmax)
        idx = np.zeros(cap + 1, np.int64)
        val = np.zeros(cap + 1, np.float64)
        nnz = i64(0)
        self.call("csmp_foba", ptr(b), dtype_code(b.dtype), C.c_double(float(delta)), i64(cap), ptr(idx), ptr(val), C.byref(nnz))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy()

    def br(self, b, max_eps=float("inf"), max_delta=float("inf"), k=0, lace=False):
        b = self._b(b)
        idx = np.zeros(self.N + 1, np.int64)
        val = np.zeros(self.N + 1, np.float64)
        nnz = i64(0)
        self.call("csmp_br", ptr(b), dtype_code(b.dtype), C.c_double(float(max_eps)), C.c_double(float(max_delta)),
                  i64(int(k)), int(bool(lace)), ptr(idx), ptr(val), C.byref(nnz))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy()

    def fr_scores(self):
        d2 = np.zeros(self.N, np.float64)
        self.call("csmp_fr_scores", ptr(d2))
        return d2

    def _batch_host(self, name, B, k, args, locs=True):
        """The batch entry `name` on the host matrix B (M x nsig, column-major) -> (idx k x nsig, val, nnz) numpy arrays, + iters for
        csmp_sp_batch (locs False: no b_loc / out_loc arguments).  args: those between nsig (b_loc) and the outputs."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        M, nsig = B.shape
        if M != self.M:
            raise CsmpError(EDIM, f"size(B, 1) = {M} but size(A, 1) = {self.M}")
        out = (np.zeros((int(k), nsig), np.int64, order="F"), np.zeros((int(k), nsig), np.float64, order="F"), np.zeros(nsig, np.int64))
        if locs:
            self.call(name, ptr(B), dtype_code(B.dtype), i64(M), i64(nsig), HOST, *args, *map(ptr, out), HOST)
            return out
        out += (np.zeros(nsig, np.int64),)
        self.call(name, ptr(B), dtype_code(B.dtype), i64(M), i64(nsig), *args, *map(ptr, out))
        return out

    def _batch_device(self, name, B, k, args, idx, val, nnz):
        """The batch entry `name` on torch CUDA tensors: B (nsig, M) rows = signals; outputs idx (nsig, k) int64, val (nsig, k) float64,
        nnz (nsig,) int64.  args: those between b_loc and the outputs."""
        import torch
        nsig, M = B.shape
        assert B.is_cuda and B.is_contiguous() and M == self.M
        assert idx.dtype == torch.int64 and val.dtype == torch.float64 and nnz.dtype == torch.int64
        assert idx.is_contiguous() and val.is_contiguous() and idx.shape == (nsig, int(k)) and val.shape == (nsig, int(k))
        code = F32 if B.dtype == torch.float32 else F64
        self.call(name, vp(B.data_ptr()), code, i64(M), i64(nsig), DEVICE, *args, vp(idx.data_ptr()), vp(val.data_ptr()),
                  vp(nnz.data_ptr()), DEVICE)

    def omp_batch(self, B, k, eps):
        """Host matrix B (M x nsig, column-major) -> (idx k x nsig, val, nnz) numpy arrays."""
        return self._batch_host("csmp_omp_batch", B, k, (i64(int(k)), C.c_double(eps)))

    def omp_batch_device(self, B, k, eps, idx, val, nnz):
        """torch CUDA tensors: B (nsig, M) rows = signals; outputs idx (nsig, k) int64,
        val (nsig, k) float64, nnz (nsig,) int64.  Only enqueues work; call sync()."""
        self._batch_device("csmp_omp_batch", B, k, (i64(int(k)), C.c_double(eps)), idx, val, nnz)

    def mp_batch(self, B, k):
        """mp for every column of the host matrix B (M x nsig, column-major) -> (idx k x nsig, val, nnz); nnz[s] <= k: atoms repeat."""
        return self._batch_host("csmp_mp_batch", B, k, (i64(int(k)),))

    def mp_batch_device(self, B, k, idx, val, nnz):
        """torch CUDA tensors as in omp_batch_device.  Only enqueues work; call sync()."""
        self._batch_device("csmp_mp_batch", B, k, (i64(int(k)),), idx, val, nnz)

    def _somp_call(self, B, code, ldB, nsig, b_loc, k, eps, p):
        """csmp_somp with the outputs on the host -> (idx, val n x nsig, info)"""
        kk = max(int(k), 1)
        idx, order = np.zeros(kk, np.int64), np.zeros(kk, np.int64)
        val = np.zeros((kk, max(nsig, 1)), np.float64, order="F")
        resnorm = np.zeros(max(nsig, 1), np.float64)
        nnz, passes = i64(0), i64(0)
        self.call("csmp_somp", B, code, i64(ldB), i64(nsig), b_loc, i64(int(k)), C.c_double(eps), int(p), ptr(idx), ptr(val), i64(kk),
                  C.byref(nnz), ptr(order), ptr(resnorm), C.byref(passes), HOST)
        n = nnz.value
        info = {"order": order[:n].copy(), "resnorm": resnorm[:nsig].copy(), "steps": n, "passes": passes.value}
        return idx[:n].copy(), np.asfortranarray(val[:n, :nsig]), info

    def somp(self, B, k, eps, p=1):
        """csmp_somp on the host matrix B (M x nsig): simultaneous OMP, ONE support for all columns -> (idx n ascending, val n x nsig
        whose row i belongs to atom idx[i], info = order (the atoms as they were picked), resnorm float64[nsig], steps, passes)."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        return self._somp_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), B.shape[1], HOST, k, eps, p)

    def somp_device(self, B, k, eps, p=1):
        """as somp, on a torch CUDA matrix whose COLUMNS are the signals: B (M, nsig) float32 / float64 with stride (1, ldB >= M).
        The results come back as somp's host arrays; the work is done when the call returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        if (self.M > 1 and B.stride(0) != 1) or ldB < self.M:
            raise CsmpError(EDIM, "B must be column-major: unit row stride, a column stride of at least its row count")
        return self._somp_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, k, eps, p)

    def gomp_batch(self, B, l, k, eps):
        """Host matrix B (M x nsig, column-major) -> (idx k x nsig, val, nnz): gomp for every column, two solves in flight."""
        return self._batch_host("csmp_gomp_batch", B, k, (i64(int(l)), i64(int(k)), C.c_double(eps)))

    def gomp_batch_device(self, B, l, k, eps, idx, val, nnz):
        """torch CUDA tensors as in omp_batch_device."""
        self._batch_device("csmp_gomp_batch", B, k, (i64(int(l)), i64(int(k)), C.c_double(eps)), idx, val, nnz)

    def sp_batch(self, B, k, delta=1e-12, maxiter=-1):
        """Host matrix B (M x nsig, column-major) -> (idx k x nsig, val, nnz, iters): sp for every column, several solves in flight."""
        return self._batch_host("csmp_sp_batch", B, k, (i64(int(k)), C.c_double(delta), i64(int(maxiter))), locs=False)

    def fr_batch(self, B, k, max_eps=0.0, min_delta=0.0):
        """fr for every column of the host matrix B (M x nsig, column-major) -> (idx k x nsig, val, nnz)."""
        return self._batch_host("csmp_fr_batch", B, k, (i64(int(k)), C.c_double(max_eps), C.c_double(min_delta)))

    def fr_batch_device(self, B, k, max_eps, min_delta, idx, val, nnz):
        """torch CUDA tensors as in omp_batch_device.  Only enqueues work; call sync()."""
        self._batch_device("csmp_fr_batch", B, k, (i64(int(k)), C.c_double(max_eps), C.c_double(min_delta)), idx, val, nnz)

    def omp_batch_mfma(self, B, k, eps):
        """Batched (MFMA-screened) variant of omp_batch: same inputs and outputs."""
        return self._batch_host("csmp_omp_batch_mfma", B, k, (i64(int(k)), C.c_double(eps)))

    def omp_batch_mfma_device(self, B, k, eps, idx, val, nnz):
        """torch CUDA tensors as in omp_batch_device; synchronises once at the end."""
        self._batch_device("csmp_omp_batch_mfma", B, k, (i64(int(k)), C.c_double(eps)), idx, val, nnz)

    def batch_screen_kernel(self):
        return lib().csmp_batch_screen_kernel(self._h).decode()

    # ---- signals sharded over GPUs with the collective inside the library (csmp_comm_*, csmp_omp_sharded)
    def comm_init(self, comm_id, rank, world):
        """ncclCommInitRank on this context's GPU; comm_id: the COMM_ID_BYTES bytes rank 0 got from comm_id()."""
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        self.call("csmp_comm_init", C.cast(buf, vp), int(rank), int(world))

    def comm_free(self):
        self.call("csmp_comm_free")

    def pack_block_device(self, idx, val, nnz, rows):
        """torch CUDA tensors idx / val (nloc, k), nnz (nloc,) -> (rows, 2k+1) float64 tensor on the device (rows >= nloc, surplus zero)."""
        import torch
        nloc, k = idx.shape
        out = torch.empty((int(rows), 2 * k + 1), dtype=torch.float64, device=idx.device)
        self.call("csmp_pack_block_device", vp(idx.data_ptr() if nloc else 0), vp(val.data_ptr() if nloc else 0), vp(nnz.data_ptr() if nloc else 0),
                  i64(k), i64(nloc), i64(int(rows)), vp(out.data_ptr()))
        return out

    def unpack_gathered_device(self, gathered, k, nsig, world):
        """(world * rows, 2k+1) float64 CUDA tensor of every rank's packed block -> idx (nsig, k) int64, val (nsig, k), nnz (nsig,) on the device."""
        import torch
        dev = gathered.device
        idx = torch.empty((int(nsig), int(k)), dtype=torch.int64, device=dev)
        val = torch.empty((int(nsig), int(k)), dtype=torch.float64, device=dev)
        nnz = torch.empty(int(nsig), dtype=torch.int64, device=dev)
        self.call("csmp_unpack_gathered_device", vp(gathered.data_ptr()), i64(int(k)), i64(int(nsig)), int(world), vp(idx.data_ptr()),
                  vp(val.data_ptr()), vp(nnz.data_ptr()))
        return idx, val, nnz

    def omp_sharded(self, B_local, nsig, k, eps, method="exact"):
        """This rank's block B_local (M x nloc, host) of `nsig` signals in all -> (idx k x nsig, val, nnz) of ALL signals."""
        B = np.asfortranarray(B_local)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B, 1) = {B.shape[0]} but size(A, 1) = {self.M}")
        idx = np.zeros((int(k), int(nsig)), np.int64, order="F")
        val = np.zeros((int(k), int(nsig)), np.float64, order="F")
        nnz = np.zeros(int(nsig), np.int64)
        self.call("csmp_omp_sharded", ptr(B), dtype_code(B.dtype), i64(self.M), i64(int(nsig)), HOST, i64(int(k)), C.c_double(eps),
                  {"exact": 0, "mfma": 1}[method], ptr(idx), ptr(val), ptr(nnz), HOST)
        return idx, val, nnz

    def omp_sharded_device(self, B_local, nsig, k, eps, idx, val, nnz, method="exact"):
        """torch CUDA tensors: B_local (nloc, M) rows = this rank's signals; idx / val (nsig, k), nnz (nsig): all signals."""
        import torch
        nloc, M = B_local.shape
        assert B_local.is_cuda and B_local.is_contiguous() and M == self.M
        assert idx.dtype == torch.int64 and val.dtype == torch.float64 and nnz.dtype == torch.int64
        assert idx.is_contiguous() and val.is_contiguous() and idx.shape == (int(nsig), int(k)) and val.shape == (int(nsig), int(k))
        code = F32 if B_local.dtype == torch.float32 else F64
        self.call("csmp_omp_sharded", vp(B_local.data_ptr() if nloc else 0), code, i64(M), i64(int(nsig)), DEVICE, i64(int(k)), C.c_double(eps),
                  {"exact": 0, "mfma": 1}[method], vp(idx.data_ptr()), vp(val.data_ptr()), vp(nnz.data_ptr()), DEVICE)

    def batch_layout(self):
        n, st = i64(0), C.c_int(0)
        self.call("csmp_batch_layout", C.byref(n), C.byref(st))
        return {"screen_signals": n.value, "streams": st.value}

    def batch_stats(self):
        v = [i64(0) for _ in range(5)]
        ms = C.c_double(0)
        self.call("csmp_batch_stats", *[C.byref(x) for x in v], C.byref(ms))
        return {"signals": v[0].value, "resolved_exactly": v[1].value, "uncertain": v[2].value, "illcond": v[3].value,
                "screen_launches": v[4].value, "screen_ms": ms.value}

    def screened_stats(self, reset=False):
        """Screened solves (option screened_sweep) made by this context, and how many were repeated with the exact sweep."""
        a, b = i64(0), i64(0)
        self.call("csmp_screened_stats", C.byref(a), C.byref(b), int(bool(reset)))
        return {"solves": a.value, "fallbacks": b.value}

    # ---- step level
    def solver_begin(self, algo, b, kcap, idx0=None, val0=None):
        b = self._b(b)
        idx0 = np.zeros(0, np.int64) if idx0 is None else np.ascontiguousarray(idx0, dtype=np.int64)
        val0 = np.zeros(0, np.float64) if val0 is None else np.ascontiguousarray(val0, dtype=np.float64)
        self.call("csmp_solver_begin", int(algo), ptr(b), dtype_code(b.dtype), i64(int(kcap)), ptr(idx0), ptr(val0),
                  i64(len(idx0)))

    def solver_step(self, l=1):
        self.call("csmp_solver_step", i64(int(l)))

    def solver_acquire(self, k):
        """sp_acquisition!(P, x, k) (SP) / oblivious_acquisition!(P, x, k) (OMPR, OMP, GOMP)"""
        self.call("csmp_solver_acquire", i64(int(k)))

    def solver_remove(self, atom):
        self.call("csmp_solver_remove", i64(int(atom)))

    def solver_state(self, cap):
        idx = np.zeros(cap, np.int64)
        val = np.zeros(cap, np.float64)
        order = np.zeros(cap, np.int64)
        nnz = i64(0)
        res = C.c_double(0)
        stop = C.c_int(0)
        self.call("csmp_solver_state", ptr(idx), ptr(val), C.byref(nnz), C.byref(res), ptr(order), C.byref(stop))
        n = nnz.value
        return idx[:n].copy(), val[:n].copy(), res.value, order[:n].copy(), stop.value

    # ---- one signal, columns sharded (csmp_shard_*): torch CUDA byte tensors for the records
    def set_option(self, key, value):
        """csmp_set_option: key is an OPT_* constant or its lower-case name ("batch_cert", "batch_gram", ...)."""
        self.call("csmp_set_option", int(OPTIONS.get(key, key)), int(value))

    def get_option(self, key):
        v = i64(0)
        self.call("csmp_get_option", int(OPTIONS.get(key, key)), C.byref(v))
        return int(v.value)

    def set_stream(self, hip_stream):
        """Borrow a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); 0 / None: the library's own."""
        self.call("csmp_set_stream", vp(hip_stream or 0))

    def shard_config(self, col_offset):
        self.call("csmp_shard_config", i64(int(col_offset)))

    def shard_record_bytes(self):
        return int(lib().csmp_shard_record_bytes(self._h))

    def shard_sweep(self, eps, check_eps, rec):
        assert rec.is_cuda and rec.is_contiguous() and rec.numel() * rec.element_size() >= self.shard_record_bytes()
        self.call("csmp_shard_sweep", C.c_double(eps), int(bool(check_eps)), vp(rec.data_ptr()))

    def shard_append(self, recs, nrec):
        assert recs.is_cuda and recs.is_contiguous() and recs.numel() * recs.element_size() >= nrec * self.shard_record_bytes()
        self.call("csmp_shard_append", vp(recs.data_ptr()), int(nrec))

    # ---- l1-regularised least squares
    def _ista_args(self, w, idx0, val0):
        w = np.ascontiguousarray(np.atleast_1d(w), dtype=np.float64)
        if w.ndim != 1:
            raise CsmpError(EDIM, "the weights must be a scalar or a vector")
        idx0 = np.zeros(0, np.int64) if idx0 is None else np.ascontiguousarray(idx0, dtype=np.int64)
        val0 = np.zeros(0, np.float64) if val0 is None else np.ascontiguousarray(val0, dtype=np.float64)
        if idx0.shape != val0.shape or idx0.ndim != 1:
            raise CsmpError(EDIM, "warm start: idx0 and val0 must be vectors of one length")
        return w, idx0, val0

    def ista(self, b, w, idx0=None, val0=None, maxiter=1024, stepsize=1e-2, accel=False):
        """csmp_ista on a host signal: (dense x, Float64[N]; ||b - A x||).  w: one weight or N of them; idx0 / val0: the warm start."""
        b = self._b(b)
        w, idx0, val0 = self._ista_args(w, idx0, val0)
        x = np.zeros(self.N, np.float64)
        rn = C.c_double(0)
        self.call("csmp_ista", ptr(b), dtype_code(b.dtype), ptr(w), i64(len(w)), ptr(idx0), ptr(val0), i64(len(idx0)), i64(int(maxiter)),
                  C.c_double(stepsize), int(bool(accel)), ptr(x), HOST, C.byref(rn))
        return x, rn.value

    def ista_device(self, b, w, x, idx0=None, val0=None, maxiter=1024, stepsize=1e-2, accel=False):
        """torch CUDA tensors: b (M,) float32 / float64, x (N,) float64 receives the dense result.  Returns ||b - A x||; the work is done
        when the call returns."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        if not (x.is_cuda and x.is_contiguous() and x.shape == (self.N,) and x.dtype == torch.float64):
            raise CsmpError(EDIM, "x must be a contiguous CUDA float64 vector of length size(A, 2)")
        w, idx0, val0 = self._ista_args(w, idx0, val0)
        rn = C.c_double(0)
        self.call("csmp_ista", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, ptr(w), i64(len(w)), ptr(idx0), ptr(val0),
                  i64(len(idx0)), i64(int(maxiter)), C.c_double(stepsize), int(bool(accel)), vp(x.data_ptr()), DEVICE, C.byref(rn))
        return rn.value

    def _ista_batch_call(self, B, code, ldB, nsig, b_loc, w, X0, ldX0, X, ldX, x_loc, maxiter, stepsize, accel):
        try:
            w, nw, ldw = ista_batch_weights(w, self.N, nsig)
        except ValueError as e:
            raise CsmpError(EDIM, str(e)) from None
        rn = np.zeros(max(nsig, 1), np.float64)
        self.call("csmp_ista_batch", B, code, i64(ldB), i64(nsig), b_loc, ptr(w), i64(nw), i64(ldw), X0, i64(ldX0), i64(int(maxiter)),
                  C.c_double(stepsize), int(bool(accel)), X, i64(ldX), x_loc, rn.ctypes.data_as(C.POINTER(C.c_double)))
        return rn[:nsig]

    def ista_batch(self, B, w, X0=None, maxiter=1024, stepsize=1e-2, accel=False):
        """csmp_ista_batch on the host matrix B (M x nsig): ista (accel: fista) for every column, the signals of a group on shared
        launches -- (X, Float64 N x nsig in Fortran order; resnorm float64[nsig]).  Column s and resnorm[s] are ista(B[:, s], w_s, ...)'s
        bit for bit.  w: a scalar, an nsig-vector (one lambda per signal), an N-vector (shared by all signals) or an N x nsig matrix (a
        weight vector per signal); with nsig == N a vector is the shared N-vector.  X0: None, or the dense N x nsig warm starts."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        nsig = B.shape[1]
        ld = max(self.N, 1)
        X = np.zeros((ld, nsig), np.float64, order="F")
        if X0 is not None:
            X0 = np.asarray(X0, dtype=np.float64)
            if X0.shape != (self.N, nsig):
                raise CsmpError(EDIM, f"size(X0) = {X0.shape} but the warm starts are size(A, 2) x nsig = {(self.N, nsig)}")
            X[:self.N] = X0  # (continued in place: X0 == X)
        rn = self._ista_batch_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), nsig, HOST, w, None if X0 is None else ptr(X), ld, ptr(X), ld, HOST,
                                   maxiter, stepsize, accel)
        return X[:self.N], rn

    def ista_batch_device(self, B, w, X, X0=None, maxiter=1024, stepsize=1e-2, accel=False):
        """torch CUDA tensors whose COLUMNS are the signals and the results, with bp_batch_device's stride rules: B (M, nsig) float32 /
        float64 with stride (1, ldB >= M), X and (optionally) X0 (N, nsig) float64 with stride (1, ld >= N); X0 may be X itself (a run
        continued in place) and must not overlap it otherwise.  w: as ista_batch, on the host.  Returns resnorm; the work is done when
        the call returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        if (self.M > 1 and B.stride(0) != 1) or ldB < self.M:
            raise CsmpError(EDIM, "B must be column-major: unit row stride, a column stride of at least its row count")
        lds = []
        for name, T in (("X", X), ("X0", X0)):
            if T is None:
                lds.append(max(self.N, 1))
                continue
            if not (T.is_cuda and T.dim() == 2 and T.shape == (self.N, nsig) and T.dtype == torch.float64):
                raise CsmpError(EDIM, f"{name} must be a CUDA float64 matrix of size(A, 2) rows and B's columns")
            ld = T.stride(1) if nsig > 1 else max(self.N, 1)
            if (self.N > 1 and T.stride(0) != 1) or ld < self.N:
                raise CsmpError(EDIM, f"{name} must be column-major: unit row stride, a column stride of at least its row count")
            lds.append(ld)
        return self._ista_batch_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, w,
                                     None if X0 is None else vp(X0.data_ptr()), lds[1], vp(X.data_ptr()), lds[0], DEVICE, maxiter, stepsize, accel)

    def _ista_joint_call(self, B, code, ldB, nsig, b_loc, w, X0, ldX0, X, ldX, x_loc, maxiter, stepsize, accel):
        w = np.atleast_1d(np.asarray(w, dtype=np.float64))
        if w.ndim != 1:
            raise CsmpError(EDIM, "the weights must be a scalar or a vector (one weight per row of X)")
        w = np.ascontiguousarray(w)
        rn = np.zeros(max(nsig, 1), np.float64)
        rows = i64(0)
        self.call("csmp_ista_joint", B, code, i64(ldB), i64(nsig), b_loc, ptr(w), i64(len(w)), X0, i64(ldX0), i64(int(maxiter)),
                  C.c_double(stepsize), int(bool(accel)), X, i64(ldX), x_loc, C.byref(rows), rn.ctypes.data_as(C.POINTER(C.c_double)))
        return {"rows": int(rows.value), "resnorm": rn[:nsig]}

    def ista_joint(self, B, w, X0=None, maxiter=1024, stepsize=1e-2, accel=False):
        """csmp_ista_joint on the host matrix B (M x nsig): ista (accel: fista) on ||B - A X||_F^2 + sum_j w_j ||X[j, :]||_2, ONE row
        support for all columns -- (X, Float64 N x nsig in Fortran order; info = rows (the non-zero rows of X), resnorm float64[nsig]).
        w: a scalar or an N-vector (one weight per row).  X0: None, or the dense N x nsig warm start.  One column is ista."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        nsig = B.shape[1]
        ld = max(self.N, 1)
        X = np.zeros((ld, nsig), np.float64, order="F")
        if X0 is not None:
            X0 = np.asarray(X0, dtype=np.float64)
            if X0.shape != (self.N, nsig):
                raise CsmpError(EDIM, f"size(X0) = {X0.shape} but the warm start is size(A, 2) x nsig = {(self.N, nsig)}")
            X[:self.N] = X0  # (continued in place: X0 == X)
        info = self._ista_joint_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), nsig, HOST, w, None if X0 is None else ptr(X), ld, ptr(X), ld,
                                     HOST, maxiter, stepsize, accel)
        return X[:self.N], info

    def ista_joint_device(self, B, w, X, X0=None, maxiter=1024, stepsize=1e-2, accel=False):
        """torch CUDA tensors whose COLUMNS are the signals and the results, with ista_batch_device's stride rules: B (M, nsig) float32 /
        float64 with stride (1, ldB >= M), X and (optionally) X0 (N, nsig) float64 with stride (1, ld >= N); X0 may be X itself (a run
        continued in place) and must not overlap it otherwise.  w: as ista_joint, on the host.  Returns info; the work is done when the
        call returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        if (self.M > 1 and B.stride(0) != 1) or ldB < self.M:
            raise CsmpError(EDIM, "B must be column-major: unit row stride, a column stride of at least its row count")
        lds = []
        for name, T in (("X", X), ("X0", X0)):
            if T is None:
                lds.append(max(self.N, 1))
                continue
            if not (T.is_cuda and T.dim() == 2 and T.shape == (self.N, nsig) and T.dtype == torch.float64):
                raise CsmpError(EDIM, f"{name} must be a CUDA float64 matrix of size(A, 2) rows and B's columns")
            ld = T.stride(1) if nsig > 1 else max(self.N, 1)
            if (self.N > 1 and T.stride(0) != 1) or ld < self.N:
                raise CsmpError(EDIM, f"{name} must be column-major: unit row stride, a column stride of at least its row count")
            lds.append(ld)
        return self._ista_joint_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, w,
                                     None if X0 is None else vp(X0.data_ptr()), lds[1], vp(X.data_ptr()), lds[0], DEVICE, maxiter, stepsize, accel)

    # ---- reweighted l1
    def ard_weights(self, x, w=None, eps=1e-2, iter=8):
        """csmp_ard_weights on host vectors: the N weights after `iter` iterations of ard_weights! from w (None: ones)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        w = np.ones(self.N) if w is None else np.ascontiguousarray(w, dtype=np.float64)
        if x.shape != (self.N,) or w.shape != (self.N,):
            raise CsmpError(EDIM, "length(x) and length(w) have to be size(A, 2)")
        out = np.zeros(max(self.N, 1), np.float64)
        self.call("csmp_ard_weights", ptr(x), ptr(w), C.c_double(eps), i64(int(iter)), ptr(out), HOST)
        return out[:self.N]

    def ard_weights_device(self, x, w, out, eps=1e-2, iter=8):
        """torch CUDA float64 vectors of length N: x, the weights w to start from, out (may be w) receives the result."""
        import torch
        for v in (x, w, out):
            if not (v.is_cuda and v.is_contiguous() and v.shape == (self.N,) and v.dtype == torch.float64):
                raise CsmpError(EDIM, "x, w and out must be contiguous CUDA float64 vectors of length size(A, 2)")
        self.call("csmp_ard_weights", vp(x.data_ptr()), vp(w.data_ptr()), C.c_double(eps), i64(int(iter)), vp(out.data_ptr()), DEVICE)

    def ista_reweighted(self, b, lam, scheme, eps=1e-2, ard_iter=8, outer_maxiter=8, min_decrease=1e-8, maxiter=1024, stepsize=1e-2, accel=False,
                        return_weights=False):
        """csmp_ista_reweighted on a host signal: (dense x, ||b - A x||, solves done[, the last weights]).  scheme: "candes" / "ard"."""
        b = self._b(b)
        x = np.zeros(max(self.N, 1), np.float64)
        w = np.zeros(max(self.N, 1), np.float64) if return_weights else None
        rn, done = C.c_double(0), i64(0)
        self.call("csmp_ista_reweighted", ptr(b), dtype_code(b.dtype), C.c_double(lam), _scheme(scheme), C.c_double(eps), i64(int(ard_iter)),
                  i64(int(outer_maxiter)), C.c_double(min_decrease), i64(int(maxiter)), C.c_double(stepsize), int(bool(accel)), ptr(x), HOST, ptr(w),
                  C.byref(done), C.byref(rn))
        res = (x[:self.N], rn.value, int(done.value))
        return res + (w[:self.N],) if return_weights else res

    def ista_reweighted_device(self, b, lam, scheme, x, w=None, eps=1e-2, ard_iter=8, outer_maxiter=8, min_decrease=1e-8, maxiter=1024,
                               stepsize=1e-2, accel=False):
        """torch CUDA tensors: b (M,) float32 / float64; x and (optionally) w (N,) float64 receive the result and the last weights.
        Returns (||b - A x||, solves done); the work is done when the call returns."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        for v in (x,) if w is None else (x, w):
            if not (v.is_cuda and v.is_contiguous() and v.shape == (self.N,) and v.dtype == torch.float64):
                raise CsmpError(EDIM, "x and w must be contiguous CUDA float64 vectors of length size(A, 2)")
        rn, done = C.c_double(0), i64(0)
        self.call("csmp_ista_reweighted", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, C.c_double(lam), _scheme(scheme),
                  C.c_double(eps), i64(int(ard_iter)), i64(int(outer_maxiter)), C.c_double(min_decrease), i64(int(maxiter)), C.c_double(stepsize),
                  int(bool(accel)), vp(x.data_ptr()), DEVICE, vp(w.data_ptr() if w is not None else 0), C.byref(done), C.byref(rn))
        return rn.value, int(done.value)

    # ---- basis pursuit
    def _bp_info(self, it, rn, flags):
        return {"iterations": int(it.value), "converged": bool(flags.value & BP_CONVERGED), "factored": bool(flags.value & BP_FACTORED),
                "resnorm": rn.value}

    def bp(self, b, w=1.0, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
        """csmp_bp on a host signal: (dense z, Float64[N]; info = iterations, converged, factored, resnorm).  w: one weight or N of them.
        The first call on a dictionary forms and factorises A Aᵀ: M² + (2M)² doubles of device memory (128 MiB + 512 MiB at M = 4096), kept
        until the dictionary changes."""
        b = self._b(b)
        w, _, _ = self._ista_args(w, None, None)
        x = np.zeros(max(self.N, 1), np.float64)
        rn, it, flags = C.c_double(0), i64(0), C.c_int(0)
        self.call("csmp_bp", ptr(b), dtype_code(b.dtype), ptr(w), i64(len(w)), C.c_double(rho), i64(int(maxiter)), C.c_double(tol),
                  i64(int(check_every)), ptr(x), HOST, C.byref(it), C.byref(rn), C.byref(flags))
        return x[:self.N], self._bp_info(it, rn, flags)

    def bp_device(self, b, w, x, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
        """torch CUDA tensors: b (M,) float32 / float64, x (N,) float64 receives the dense result.  Returns info; the work is done when the
        call returns."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        if not (x.is_cuda and x.is_contiguous() and x.shape == (self.N,) and x.dtype == torch.float64):
            raise CsmpError(EDIM, "x must be a contiguous CUDA float64 vector of length size(A, 2)")
        w, _, _ = self._ista_args(w, None, None)
        rn, it, flags = C.c_double(0), i64(0), C.c_int(0)
        self.call("csmp_bp", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, ptr(w), i64(len(w)), C.c_double(rho), i64(int(maxiter)),
                  C.c_double(tol), i64(int(check_every)), vp(x.data_ptr()), DEVICE, C.byref(it), C.byref(rn), C.byref(flags))
        return self._bp_info(it, rn, flags)

    def _bp_batch_call(self, B, code, ldB, nsig, b_loc, w, X, ldX, x_loc, rho, maxiter, tol, check_every):
        w, _, _ = self._ista_args(w, None, None)
        it, rn, flags = np.zeros(max(nsig, 1), np.int64), np.zeros(max(nsig, 1), np.float64), np.zeros(max(nsig, 1), np.int32)
        self.call("csmp_bp_batch", B, code, i64(ldB), i64(nsig), b_loc, ptr(w), i64(len(w)), C.c_double(rho), i64(int(maxiter)), C.c_double(tol),
                  i64(int(check_every)), X, i64(ldX), x_loc, it.ctypes.data_as(C.POINTER(i64)), rn.ctypes.data_as(C.POINTER(C.c_double)),
                  flags.ctypes.data_as(C.POINTER(C.c_int)))
        it, rn, flags = it[:nsig], rn[:nsig], flags[:nsig]
        return {"iterations": it, "converged": (flags & BP_CONVERGED) != 0, "resnorm": rn, "factored": bool(nsig > 0 and flags[0] & BP_FACTORED)}

    def bp_batch(self, B, w=1.0, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
        """csmp_bp_batch on the host matrix B (M x nsig): bp for every column, the signals of a group in lockstep on shared launches --
        (X, Float64 N x nsig in Fortran order; info = iterations int64[nsig], converged bool[nsig], resnorm float64[nsig], factored).
        Column s and its info are bp(B[:, s], ...)'s bit for bit.  w: one weight or N of them, shared by all signals."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        nsig = B.shape[1]
        X = np.zeros((max(self.N, 1), nsig), np.float64, order="F")
        info = self._bp_batch_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), nsig, HOST, w, ptr(X), max(self.N, 1), HOST, rho, maxiter, tol,
                                   check_every)
        return X[:self.N], info

    def bp_batch_device(self, B, w, X, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
        """torch CUDA tensors whose COLUMNS are the signals and the results: B.T and X.T are row-contiguous views, B (M, nsig) float32 /
        float64 with stride (1, ldB >= M), X (N, nsig) float64 with stride (1, ldX >= N) -- slices of taller column-major buffers
        qualify.  Returns info; the work is done when the call returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        if not (X.is_cuda and X.dim() == 2 and X.shape == (self.N, nsig) and X.dtype == torch.float64):
            raise CsmpError(EDIM, "X must be a CUDA float64 matrix of size(A, 2) rows and B's columns")
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        ldX = X.stride(1) if nsig > 1 else max(self.N, 1)
        if (self.M > 1 and B.stride(0) != 1) or (self.N > 1 and X.stride(0) != 1) or ldB < self.M or ldX < self.N:
            raise CsmpError(EDIM, "B and X must be column-major: unit row stride, column strides of at least their row counts")
        return self._bp_batch_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, w, vp(X.data_ptr()), ldX, DEVICE,
                                   rho, maxiter, tol, check_every)

    def _bp_joint_call(self, B, code, ldB, nsig, b_loc, w, X, ldX, x_loc, rho, maxiter, tol, check_every):
        w, _, _ = self._ista_args(w, None, None)
        rn = np.zeros(max(nsig, 1), np.float64)
        it, rows, flags = i64(0), i64(0), C.c_int(0)
        self.call("csmp_bp_joint", B, code, i64(ldB), i64(nsig), b_loc, ptr(w), i64(len(w)), C.c_double(rho), i64(int(maxiter)), C.c_double(tol),
                  i64(int(check_every)), X, i64(ldX), x_loc, C.byref(it), C.byref(rows), rn.ctypes.data_as(C.POINTER(C.c_double)), C.byref(flags))
        return {"iterations": int(it.value), "converged": bool(flags.value & BP_CONVERGED), "factored": bool(flags.value & BP_FACTORED),
                "rows": int(rows.value), "resnorm": rn[:nsig]}

    def bp_joint(self, B, w=1.0, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
        """csmp_bp_joint on the host matrix B (M x nsig): min sum_j w_j ||X[j, :]||_2 subject to A X = B, ONE row support for all columns
        and ONE stopping rule -- (X, Float64 N x nsig in Fortran order; info = iterations, converged, factored, rows (the non-zero rows of
        X), resnorm float64[nsig]).  w: one weight or N of them (one per row).  One column is bp."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        nsig = B.shape[1]
        X = np.zeros((max(self.N, 1), nsig), np.float64, order="F")
        info = self._bp_joint_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), nsig, HOST, w, ptr(X), max(self.N, 1), HOST, rho, maxiter, tol,
                                   check_every)
        return X[:self.N], info

    def bp_joint_device(self, B, w, X, rho=1.0, maxiter=16384, tol=1e-8, check_every=32):
        """torch CUDA tensors whose COLUMNS are the signals and the results, with bp_batch_device's stride rules: B (M, nsig) float32 /
        float64 with stride (1, ldB >= M), X (N, nsig) float64 with stride (1, ldX >= N).  Returns info; the work is done when the call
        returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        if not (X.is_cuda and X.dim() == 2 and X.shape == (self.N, nsig) and X.dtype == torch.float64):
            raise CsmpError(EDIM, "X must be a CUDA float64 matrix of size(A, 2) rows and B's columns")
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        ldX = X.stride(1) if nsig > 1 else max(self.N, 1)
        if (self.M > 1 and B.stride(0) != 1) or (self.N > 1 and X.stride(0) != 1) or ldB < self.M or ldX < self.N:
            raise CsmpError(EDIM, "B and X must be column-major: unit row stride, column strides of at least their row counts")
        return self._bp_joint_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, w, vp(X.data_ptr()), ldX, DEVICE,
                                   rho, maxiter, tol, check_every)

    def bp_reweighted(self, b, scheme, eps=1e-2, ard_iter=8, outer_maxiter=8, min_decrease=1e-8, rho=1.0, maxiter=16384, tol=1e-8, check_every=32,
                      return_weights=False):
        """csmp_bp_reweighted on a host signal: (dense z, ||b - A z||, solves done[, the last weights]).  scheme: "candes" / "ard"."""
        b = self._b(b)
        x = np.zeros(max(self.N, 1), np.float64)
        w = np.zeros(max(self.N, 1), np.float64) if return_weights else None
        rn, done = C.c_double(0), i64(0)
        self.call("csmp_bp_reweighted", ptr(b), dtype_code(b.dtype), _scheme(scheme), C.c_double(eps), i64(int(ard_iter)), i64(int(outer_maxiter)),
                  C.c_double(min_decrease), C.c_double(rho), i64(int(maxiter)), C.c_double(tol), i64(int(check_every)), ptr(x), HOST, ptr(w),
                  C.byref(done), C.byref(rn))
        res = (x[:self.N], rn.value, int(done.value))
        return res + (w[:self.N],) if return_weights else res

    def bp_reweighted_device(self, b, scheme, x, w=None, eps=1e-2, ard_iter=8, outer_maxiter=8, min_decrease=1e-8, rho=1.0, maxiter=16384,
                             tol=1e-8, check_every=32):
        """torch CUDA tensors: b (M,) float32 / float64; x and (optionally) w (N,) float64 receive the result and the last weights.
        Returns (||b - A z||, solves done)."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        for v in (x,) if w is None else (x, w):
            if not (v.is_cuda and v.is_contiguous() and v.shape == (self.N,) and v.dtype == torch.float64):
                raise CsmpError(EDIM, "x and w must be contiguous CUDA float64 vectors of length size(A, 2)")
        rn, done = C.c_double(0), i64(0)
        self.call("csmp_bp_reweighted", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, _scheme(scheme), C.c_double(eps),
                  i64(int(ard_iter)), i64(int(outer_maxiter)), C.c_double(min_decrease), C.c_double(rho), i64(int(maxiter)), C.c_double(tol),
                  i64(int(check_every)), vp(x.data_ptr()), DEVICE, vp(w.data_ptr() if w is not None else 0), C.byref(done), C.byref(rn))
        return rn.value, int(done.value)

    def bp_rowgram(self, device=False):
        """csmp_bp_rowgram (csmp_internal.h): G = A Aᵀ as k_rowgram forms it, Float64 (M, M) -- a numpy array, or (device=True) a torch
        CUDA tensor"""
        if device:
            import torch
            out = torch.empty((self.M, self.M), dtype=torch.float64, device="cuda")
            self.call("csmp_bp_rowgram", vp(out.data_ptr()), DEVICE)
            return out
        out = np.zeros((self.M, self.M), np.float64)
        self.call("csmp_bp_rowgram", ptr(out), HOST)
        return out

    # ---- basis pursuit denoising
    def _bpd_info(self, it, rn, flags):
        return {"iterations": int(it.value), "converged": bool(flags.value & BPD_CONVERGED), "factored": bool(flags.value & BPD_FACTORED),
                "resnorm": rn.value}

    def bpd(self, b, delta, w=1.0, rho=BPD_RHO, maxiter=16384, tol=1e-8, check_every=32):
        """csmp_bpd on a host signal: (dense z, Float64[N]; info = iterations, converged, factored, resnorm).  w: one weight or N of them.
        The first call on a dictionary forms A Aᵀ and factorises I + A Aᵀ: (2M)² doubles of device memory (512 MiB at M = 4096) are kept until
        the dictionary changes, apart from bp's factor."""
        b = self._b(b)
        w, _, _ = self._ista_args(w, None, None)
        x = np.zeros(max(self.N, 1), np.float64)
        rn, it, flags = C.c_double(0), i64(0), C.c_int(0)
        self.call("csmp_bpd", ptr(b), dtype_code(b.dtype), C.c_double(delta), ptr(w), i64(len(w)), C.c_double(rho), i64(int(maxiter)),
                  C.c_double(tol), i64(int(check_every)), ptr(x), HOST, C.byref(it), C.byref(rn), C.byref(flags))
        return x[:self.N], self._bpd_info(it, rn, flags)

    def bpd_device(self, b, delta, w, x, rho=BPD_RHO, maxiter=16384, tol=1e-8, check_every=32):
        """torch CUDA tensors: b (M,) float32 / float64, x (N,) float64 receives the dense result.  Returns info; the work is done when the
        call returns."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        if not (x.is_cuda and x.is_contiguous() and x.shape == (self.N,) and x.dtype == torch.float64):
            raise CsmpError(EDIM, "x must be a contiguous CUDA float64 vector of length size(A, 2)")
        w, _, _ = self._ista_args(w, None, None)
        rn, it, flags = C.c_double(0), i64(0), C.c_int(0)
        self.call("csmp_bpd", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, C.c_double(delta), ptr(w), i64(len(w)), C.c_double(rho),
                  i64(int(maxiter)), C.c_double(tol), i64(int(check_every)), vp(x.data_ptr()), DEVICE, C.byref(it), C.byref(rn), C.byref(flags))
        return self._bpd_info(it, rn, flags)

    def _bpd_batch_call(self, B, code, ldB, nsig, b_loc, delta, w, X, ldX, x_loc, rho, maxiter, tol, check_every):
        w, _, _ = self._ista_args(w, None, None)
        delta = np.ascontiguousarray(np.atleast_1d(np.asarray(delta, dtype=np.float64)))
        if delta.ndim != 1 or len(delta) not in (1, nsig):
            raise CsmpError(EDIM, f"length(delta) = {delta.shape} but B has {nsig} columns: one radius, or one per signal")
        it, rn, flags = np.zeros(max(nsig, 1), np.int64), np.zeros(max(nsig, 1), np.float64), np.zeros(max(nsig, 1), np.int32)
        self.call("csmp_bpd_batch", B, code, i64(ldB), i64(nsig), b_loc, ptr(delta), i64(len(delta)), ptr(w), i64(len(w)), C.c_double(rho),
                  i64(int(maxiter)), C.c_double(tol), i64(int(check_every)), X, i64(ldX), x_loc, it.ctypes.data_as(C.POINTER(i64)),
                  rn.ctypes.data_as(C.POINTER(C.c_double)), flags.ctypes.data_as(C.POINTER(C.c_int)))
        it, rn, flags = it[:nsig], rn[:nsig], flags[:nsig]
        return {"iterations": it, "converged": (flags & BPD_CONVERGED) != 0, "resnorm": rn, "factored": bool(nsig > 0 and flags[0] & BPD_FACTORED)}

    def bpd_batch(self, B, delta, w=1.0, rho=BPD_RHO, maxiter=16384, tol=1e-8, check_every=32):
        """csmp_bpd_batch on the host matrix B (M x nsig): bpd for every column, the signals of a group in lockstep on shared launches --
        (X, Float64 N x nsig in Fortran order; info = iterations int64[nsig], converged bool[nsig], resnorm float64[nsig], factored).
        Column s and its info are bpd(B[:, s], delta[s], ...)'s bit for bit.  delta: one radius or nsig of them; w: one weight or N of
        them, shared by all signals."""
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        nsig = B.shape[1]
        X = np.zeros((max(self.N, 1), nsig), np.float64, order="F")
        info = self._bpd_batch_call(ptr(B), dtype_code(B.dtype), max(self.M, 1), nsig, HOST, delta, w, ptr(X), max(self.N, 1), HOST, rho, maxiter,
                                    tol, check_every)
        return X[:self.N], info

    def bpd_batch_device(self, B, delta, w, X, rho=BPD_RHO, maxiter=16384, tol=1e-8, check_every=32):
        """torch CUDA tensors whose COLUMNS are the signals and the results, as bp_batch_device's: B (M, nsig) float32 / float64 with
        stride (1, ldB >= M), X (N, nsig) float64 with stride (1, ldX >= N).  delta: host values, one or nsig.  Returns info; the work
        is done when the call returns."""
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        if not (X.is_cuda and X.dim() == 2 and X.shape == (self.N, nsig) and X.dtype == torch.float64):
            raise CsmpError(EDIM, "X must be a CUDA float64 matrix of size(A, 2) rows and B's columns")
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        ldX = X.stride(1) if nsig > 1 else max(self.N, 1)
        if (self.M > 1 and B.stride(0) != 1) or (self.N > 1 and X.stride(0) != 1) or ldB < self.M or ldX < self.N:
            raise CsmpError(EDIM, "B and X must be column-major: unit row stride, column strides of at least their row counts")
        return self._bpd_batch_call(vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE, delta, w, vp(X.data_ptr()), ldX,
                                    DEVICE, rho, maxiter, tol, check_every)

    def bpd_reweighted(self, b, delta, scheme, eps=None, ard_iter=8, outer_maxiter=8, min_decrease=1e-4, rho=BPD_RHO, maxiter=16384, tol=1e-8,
                       check_every=32, return_weights=False):
        """csmp_bpd_reweighted on a host signal: (dense z, ||b - A z||, solves done[, the last weights]).  scheme: "candes" / "ard";
        eps=None: delta for "candes", delta² for "ard" (the reference's defaults)."""
        b = self._b(b)
        if eps is None:
            eps = delta if _scheme(scheme) == REWEIGHT_CANDES else delta * delta
        x = np.zeros(max(self.N, 1), np.float64)
        w = np.zeros(max(self.N, 1), np.float64) if return_weights else None
        rn, done = C.c_double(0), i64(0)
        self.call("csmp_bpd_reweighted", ptr(b), dtype_code(b.dtype), C.c_double(delta), _scheme(scheme), C.c_double(eps), i64(int(ard_iter)),
                  i64(int(outer_maxiter)), C.c_double(min_decrease), C.c_double(rho), i64(int(maxiter)), C.c_double(tol), i64(int(check_every)),
                  ptr(x), HOST, ptr(w), C.byref(done), C.byref(rn))
        res = (x[:self.N], rn.value, int(done.value))
        return res + (w[:self.N],) if return_weights else res

    def bpd_reweighted_device(self, b, delta, scheme, x, w=None, eps=None, ard_iter=8, outer_maxiter=8, min_decrease=1e-4, rho=BPD_RHO,
                              maxiter=16384, tol=1e-8, check_every=32):
        """torch CUDA tensors: b (M,) float32 / float64; x and (optionally) w (N,) float64 receive the result and the last weights.
        Returns (||b - A z||, solves done)."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        for v in (x,) if w is None else (x, w):
            if not (v.is_cuda and v.is_contiguous() and v.shape == (self.N,) and v.dtype == torch.float64):
                raise CsmpError(EDIM, "x and w must be contiguous CUDA float64 vectors of length size(A, 2)")
        if eps is None:
            eps = delta if _scheme(scheme) == REWEIGHT_CANDES else delta * delta
        rn, done = C.c_double(0), i64(0)
        self.call("csmp_bpd_reweighted", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, C.c_double(delta), _scheme(scheme),
                  C.c_double(eps), i64(int(ard_iter)), i64(int(outer_maxiter)), C.c_double(min_decrease), C.c_double(rho), i64(int(maxiter)),
                  C.c_double(tol), i64(int(check_every)), vp(x.data_ptr()), DEVICE, vp(w.data_ptr() if w is not None else 0), C.byref(done),
                  C.byref(rn))
        return rn.value, int(done.value)

    # ---- sparse Bayesian learning
    def sbl(self, b, sigma2, maxiter=None, min_change=1e-6, gamma=None, return_gamma=False):
        """csmp_sbl on a host signal: (dense x, Float64[N]; info = iterations, converged[; the last gamma]).  maxiter=None: 128 N, the
        reference's default.  gamma: the N variances to start from (None: ones).  The first call on a dictionary allocates the factor's
        (2M)² doubles, two M x M matrices and four N-vectors of device memory, kept until the dictionary changes."""
        b = self._b(b)
        if gamma is not None:
            gamma = np.ascontiguousarray(gamma, dtype=np.float64)
            if gamma.shape != (self.N,):
                raise CsmpError(EDIM, "length(gamma) has to be size(A, 2)")
        x = np.zeros(max(self.N, 1), np.float64)
        g = np.zeros(max(self.N, 1), np.float64) if return_gamma else None
        it, flags = i64(0), C.c_int(0)
        self.call("csmp_sbl", ptr(b), dtype_code(b.dtype), C.c_double(sigma2), i64(128 * self.N if maxiter is None else int(maxiter)),
                  C.c_double(min_change), ptr(gamma), ptr(x), ptr(g), HOST, C.byref(it), C.byref(flags))
        info = {"iterations": int(it.value), "converged": bool(flags.value & SBL_CONVERGED)}
        return (x[:self.N], info, g[:self.N]) if return_gamma else (x[:self.N], info)

    def sbl_device(self, b, sigma2, x, gamma_in=None, gamma_out=None, maxiter=None, min_change=1e-6):
        """torch CUDA tensors: b (M,) float32 / float64; x (N,) float64 receives the dense result; gamma_in (None: ones) and gamma_out
        (None: not wanted; may be gamma_in) are (N,) float64.  Returns info; the work is done when the call returns."""
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA vector of length size(A, 1), float32 or float64")
        for v in (x, gamma_in, gamma_out):
            if v is not None and not (v.is_cuda and v.is_contiguous() and v.shape == (self.N,) and v.dtype == torch.float64):
                raise CsmpError(EDIM, "x and gamma must be contiguous CUDA float64 vectors of length size(A, 2)")
        it, flags = i64(0), C.c_int(0)
        self.call("csmp_sbl", vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64, C.c_double(sigma2),
                  i64(128 * self.N if maxiter is None else int(maxiter)), C.c_double(min_change),
                  vp(gamma_in.data_ptr() if gamma_in is not None else 0), vp(x.data_ptr()),
                  vp(gamma_out.data_ptr() if gamma_out is not None else 0), DEVICE, C.byref(it), C.byref(flags))
        return {"iterations": int(it.value), "converged": bool(flags.value & SBL_CONVERGED)}

    def sbl_rowgram(self, gamma, device=False):
        """csmp_sbl_rowgram (csmp_internal.h): A diag(gamma) Aᵀ as the weighted k_rowgram forms it, Float64 (M, M) -- from and to numpy
        arrays, or (device=True) torch CUDA tensors"""
        if device:
            import torch
            out = torch.empty((self.M, self.M), dtype=torch.float64, device="cuda")
            self.call("csmp_sbl_rowgram", vp(gamma.data_ptr()), vp(out.data_ptr()), DEVICE)
            return out
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        if gamma.shape != (self.N,):
            raise CsmpError(EDIM, "length(gamma) has to be size(A, 2)")
        out = np.zeros((self.M, self.M), np.float64)
        self.call("csmp_sbl_rowgram", ptr(gamma), ptr(out), HOST)
        return out

    def sbl_forms(self, W, t, device=False):
        """csmp_sbl_forms (csmp_internal.h): (s, q), Float64[N] each, from the upper triangular directions W -- Fortran-ordered (ldw, M)
        with ldw a multiple of 64 -- and t (M,).  numpy arrays, or (device=True) torch CUDA tensors (W as its transpose: (M, ldw)
        C-contiguous)."""
        if device:
            import torch
            s = torch.empty(max(self.N, 1), dtype=torch.float64, device="cuda")
            q = torch.empty(max(self.N, 1), dtype=torch.float64, device="cuda")
            self.call("csmp_sbl_forms", vp(W.data_ptr()), i64(W.shape[1]), vp(t.data_ptr()), vp(s.data_ptr()), vp(q.data_ptr()), DEVICE)
            return s[:self.N], q[:self.N]
        W = np.asfortranarray(W, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.M or t.shape != (self.M,):
            raise CsmpError(EDIM, "W has to be (ldw, size(A, 1)) and t of length size(A, 1)")
        s, q = np.zeros(max(self.N, 1), np.float64), np.zeros(max(self.N, 1), np.float64)
        self.call("csmp_sbl_forms", ptr(W), i64(W.shape[0]), ptr(t), ptr(s), ptr(q), HOST)
        return s[:self.N], q[:self.N]

    def bench_sbl(self, sigma2, reps=5):
        """csmp_bench_sbl (csmp_internal.h): average ms of the three stages of one update on the last sbl call's gamma and b"""
        g, f, n = C.c_double(0), C.c_double(0), C.c_double(0)
        self.call("csmp_bench_sbl", C.c_double(sigma2), int(reps), C.byref(g), C.byref(f), C.byref(n))
        return {"gram_ms": g.value, "factor_ms": f.value, "forms_ms": n.value}

    # ---- greedy sparse Bayesian learning
    def _greedy(self, name, b, sigma2, caps, min_increase, alpha_in, x, alpha_out, loc, history_cap):
        """csmp_fsbl / csmp_rmps: caps are the call's iteration caps in the prototype's order; returns info"""
        cap = max(int(history_cap), 0)
        hist = np.zeros((max(cap, 1), 2), np.int64)
        it, flags = i64(0), C.c_int(0)
        self.call(name, b[0], b[1], C.c_double(sigma2), *[i64(int(c)) for c in caps], C.c_double(min_increase), alpha_in, x, alpha_out, loc,
                  ptr(hist), i64(cap), C.byref(it), C.byref(flags))
        return {"iterations": int(it.value), "converged": bool(flags.value & FSBL_CONVERGED)}, hist

    def _greedy_host(self, name, b, sigma2, caps, min_increase, alpha, history_cap):
        b = self._b(b)
        if alpha is not None:
            alpha = np.ascontiguousarray(alpha, dtype=np.float64)
            if alpha.shape != (self.N,):
                raise CsmpError(EDIM, "length(alpha) has to be size(A, 2)")
        x = np.zeros(max(self.N, 1), np.float64)
        a = np.zeros(max(self.N, 1), np.float64)
        info, hist = self._greedy(name, (ptr(b), dtype_code(b.dtype)), sigma2, caps, min_increase, ptr(alpha), ptr(x), ptr(a), HOST, history_cap)
        info["alpha"] = a[:self.N]
        return x[:self.N], info, hist

    def fsbl(self, b, sigma2, maxiter=None, min_increase=1e-6, alpha=None, history_cap=None):
        """csmp_fsbl on a host signal: (x, Float64[N], exactly 0 off the active set; info = iterations (passes), converged, alpha, history:
        the (action, index) pairs of the applied steps, 1 add, 2 delete, 3 re-estimate).  maxiter=None: 2 N, the reference's default.
        alpha: the N prior precisions to start from (+inf: inactive; None: all inactive).  history_cap=None: room for every pass.  The
        first call on a dictionary allocates M² doubles and five N-vectors of device memory, kept until the dictionary changes."""
        maxiter = 2 * self.N if maxiter is None else int(maxiter)
        cap = max(maxiter, 0) if history_cap is None else int(history_cap)
        x, info, hist = self._greedy_host("csmp_fsbl", b, sigma2, (maxiter,), min_increase, alpha, cap)
        return x, self._history(info, hist, cap, None)

    def rmps(self, b, sigma2, maxiter=None, maxiter_acquisition=None, maxiter_deletion=None, min_increase=1e-6, alpha=None, history_cap=None):
        """csmp_rmps on a host signal: as fsbl; the three caps default to M, the reference's; iterations counts the applied steps.
        history_cap=None: the whole history (a run longer than 4 N steps is run again with the room it needs)."""
        caps = tuple(self.M if c is None else int(c) for c in (maxiter, maxiter_acquisition, maxiter_deletion))
        cap = 4 * self.N if history_cap is None else int(history_cap)
        x, info, hist = self._greedy_host("csmp_rmps", b, sigma2, caps, min_increase, alpha, cap)
        if history_cap is None and info["iterations"] > cap:
            cap = info["iterations"]
            x, info, hist = self._greedy_host("csmp_rmps", b, sigma2, caps, min_increase, alpha, cap)
        return x, self._history(info, hist, cap, info["iterations"])

    @staticmethod
    def _history(info, hist, cap, applied):
        """the recorded pairs: the applied steps where known (rmps), else the rows an action was written to (fsbl: at most one a pass)"""
        n = min(cap, applied) if applied is not None else int(np.count_nonzero(hist[:max(cap, 0), 0]))
        info["history"] = [(int(a), int(i)) for a, i in hist[:n]]
        return info

    def fsbl_device(self, b, sigma2, x, alpha_in=None, alpha_out=None, maxiter=None, min_increase=1e-6, history_cap=0):
        """torch CUDA tensors: b (M,) float32 / float64; x (N,) float64 receives the result; alpha_in (None: all +inf) and alpha_out
        (None: not wanted; may be alpha_in) are (N,) float64.  Returns info; the work is done when the call returns."""
        args = self._greedy_device(b, x, alpha_in, alpha_out)
        maxiter = 2 * self.N if maxiter is None else int(maxiter)
        info, hist = self._greedy("csmp_fsbl", args[0], sigma2, (maxiter,), min_increase, *args[1:], DEVICE, history_cap)
        return self._history(info, hist, int(history_cap), None)

    def rmps_device(self, b, sigma2, x, alpha_in=None, alpha_out=None, maxiter=None, maxiter_acquisition=None, maxiter_deletion=None,
                    min_increase=1e-6, history_cap=0):
        """as fsbl_device, for csmp_rmps"""
        args = self._greedy_device(b, x, alpha_in, alpha_out)
        caps = tuple(self.M if c is None else int(c) for c in (maxiter, maxiter_acquisition, maxiter_deletion))
        info, hist = self._greedy("csmp_rmps", args[0], sigma2, caps, min_increase, *args[1:], DEVICE, history_cap)
        return self._history(info, hist, int(history_cap), info["iterations"])

    def _greedy_device(self, b, x, alpha_in, alpha_out):
        import torch
        if not (b.is_cuda and b.is_contiguous() and b.shape == (self.M,) and b.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "b must be a contiguous CUDA float32 / float64 vector of length size(A, 1)")
        for v in (x, alpha_in, alpha_out):
            if v is not None and not (v.is_cuda and v.is_contiguous() and v.shape == (self.N,) and v.dtype == torch.float64):
                raise CsmpError(EDIM, "x and alpha must be contiguous CUDA float64 vectors of length size(A, 2)")
        return ((vp(b.data_ptr()), F32 if b.dtype == torch.float32 else F64), vp(alpha_in.data_ptr() if alpha_in is not None else 0),
                vp(x.data_ptr()), vp(alpha_out.data_ptr() if alpha_out is not None else 0))

    # ---- greedy sparse Bayesian learning for many signals
    def _greedy_batch(self, name, B, code, ldB, nsig, b_loc, sigma2, caps, min_increase, alpha_in, ld_in, X, ldX, alpha_out, ld_out, x_loc,
                      history_cap, applied):
        """csmp_fsbl_batch / csmp_rmps_batch: caps are the call's iteration caps in the prototype's order; returns info without alpha"""
        s2 = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma2, dtype=np.float64)))
        if s2.ndim != 1:
            raise CsmpError(EDIM, "sigma2 has to be a scalar or one value per signal")
        cap = max(int(history_cap), 0)
        hist = np.zeros((max(nsig, 1), max(cap, 1), 2), np.int64)
        it, fl = np.zeros(max(nsig, 1), np.int64), np.zeros(max(nsig, 1), np.int32)
        self.call(name, B, code, i64(ldB), i64(nsig), b_loc, ptr(s2), i64(len(s2)), *[i64(int(c)) for c in caps], C.c_double(min_increase),
                  alpha_in, i64(ld_in), X, i64(ldX), alpha_out, i64(ld_out), x_loc, ptr(hist) if cap > 0 else None, i64(cap),
                  it.ctypes.data_as(C.POINTER(i64)), fl.ctypes.data_as(C.POINTER(C.c_int)))
        info = {"iterations": it[:nsig], "converged": (fl[:nsig] & FSBL_CONVERGED) != 0, "history": []}
        for s in range(nsig):
            one = self._history({}, hist[s], cap, int(it[s]) if applied else None)
            info["history"].append(one["history"])
        return info

    def _greedy_batch_host(self, name, B, sigma2, caps, min_increase, alpha, history_cap, applied):
        B = np.asfortranarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(np.float64)
        if B.ndim != 2 or B.shape[0] != self.M:
            raise CsmpError(EDIM, f"size(B) = {B.shape} but size(A, 1) = {self.M}")
        nsig = B.shape[1]
        ld = max(self.N, 1)
        X = np.zeros((ld, nsig), np.float64, order="F")
        a = np.zeros((ld, nsig), np.float64, order="F")
        if alpha is not None:
            alpha = np.asarray(alpha, dtype=np.float64)
            if alpha.shape != (self.N, nsig):
                raise CsmpError(EDIM, f"size(alpha) = {alpha.shape} but the warm starts are size(A, 2) x nsig = {(self.N, nsig)}")
            a[:self.N] = alpha  # (alpha_out is alpha_in)
        info = self._greedy_batch(name, ptr(B), dtype_code(B.dtype), max(self.M, 1), nsig, HOST, sigma2, caps, min_increase,
                                  None if alpha is None else ptr(a), ld, ptr(X), ld, ptr(a), ld, HOST, history_cap, applied)
        info["alpha"] = a[:self.N]
        return X[:self.N], info

    def fsbl_batch(self, B, sigma2, maxiter=None, min_increase=1e-6, alpha=None, history_cap=None):
        """csmp_fsbl_batch on the host matrix B (M x nsig): fsbl for every column, the signals of a group in lockstep on shared launches --
        (X, Float64 N x nsig in Fortran order; info = iterations int64[nsig], converged bool[nsig], alpha N x nsig, history: a list of
        (action, index) pairs per signal).  Column s and signal s's info are fsbl(B[:, s], sigma2_s, ...)'s bit for bit.  sigma2: a scalar or
        one value per signal.  alpha: None, or the N x nsig prior precisions to start from (+inf: inactive).  The defaults are fsbl's."""
        maxiter = 2 * self.N if maxiter is None else int(maxiter)
        cap = max(maxiter, 0) if history_cap is None else int(history_cap)
        return self._greedy_batch_host("csmp_fsbl_batch", B, sigma2, (maxiter,), min_increase, alpha, cap, False)

    def rmps_batch(self, B, sigma2, maxiter=None, maxiter_acquisition=None, maxiter_deletion=None, min_increase=1e-6, alpha=None,
                   history_cap=None):
        """csmp_rmps_batch on the host matrix B: as fsbl_batch, for rmps; the three caps default to M; iterations counts the applied steps.
        history_cap=None: the whole histories (a batch with a run longer than 4 N steps is run again with the room it needs)."""
        caps = tuple(self.M if c is None else int(c) for c in (maxiter, maxiter_acquisition, maxiter_deletion))
        cap = 4 * self.N if history_cap is None else int(history_cap)
        X, info = self._greedy_batch_host("csmp_rmps_batch", B, sigma2, caps, min_increase, alpha, cap, True)
        if history_cap is None and len(info["iterations"]) and int(info["iterations"].max()) > cap:
            cap = int(info["iterations"].max())
            X, info = self._greedy_batch_host("csmp_rmps_batch", B, sigma2, caps, min_increase, alpha, cap, True)
        return X, info

    def _greedy_batch_device(self, B, X, alpha_in, alpha_out):
        import torch
        if not (B.is_cuda and B.dim() == 2 and B.shape[0] == self.M and B.dtype in (torch.float32, torch.float64)):
            raise CsmpError(EDIM, "B must be a CUDA matrix of size(A, 1) rows, float32 or float64")
        nsig = B.shape[1]
        ldB = B.stride(1) if nsig > 1 else max(self.M, 1)
        if (self.M > 1 and B.stride(0) != 1) or ldB < self.M:
            raise CsmpError(EDIM, "B must be column-major: unit row stride, a column stride of at least its row count")
        lds = []
        for name, T in (("X", X), ("alpha_in", alpha_in), ("alpha_out", alpha_out)):
            if T is None:
                lds.append(max(self.N, 1))
                continue
            if not (T.is_cuda and T.dim() == 2 and T.shape == (self.N, nsig) and T.dtype == torch.float64):
                raise CsmpError(EDIM, f"{name} must be a CUDA float64 matrix of size(A, 2) rows and B's columns")
            ld = T.stride(1) if nsig > 1 else max(self.N, 1)
            if (self.N > 1 and T.stride(0) != 1) or ld < self.N:
                raise CsmpError(EDIM, f"{name} must be column-major: unit row stride, a column stride of at least its row count")
            lds.append(ld)
        p = [None if T is None else vp(T.data_ptr()) for T in (alpha_in, X, alpha_out)]
        return (vp(B.data_ptr()), F32 if B.dtype == torch.float32 else F64, ldB, nsig, DEVICE), (p[0], lds[1], p[1], lds[0], p[2], lds[2], DEVICE)

    def fsbl_batch_device(self, B, sigma2, X, alpha_in=None, alpha_out=None, maxiter=None, min_increase=1e-6, history_cap=0):
        """torch CUDA tensors whose COLUMNS are the signals and the results, with bp_batch_device's stride rules: B (M, nsig) float32 /
        float64 with stride (1, ldB >= M); X receives the results, alpha_in (None: all +inf) and alpha_out (None: not wanted; may be
        alpha_in) are (N, nsig) float64 with stride (1, ld >= N).  sigma2: on the host.  Returns info without alpha; the work is done when
        the call returns."""
        b, x = self._greedy_batch_device(B, X, alpha_in, alpha_out)
        maxiter = 2 * self.N if maxiter is None else int(maxiter)
        return self._greedy_batch("csmp_fsbl_batch", *b, sigma2, (maxiter,), min_increase, *x, history_cap, False)

    def rmps_batch_device(self, B, sigma2, X, alpha_in=None, alpha_out=None, maxiter=None, maxiter_acquisition=None, maxiter_deletion=None,
                          min_increase=1e-6, history_cap=0):
        """as fsbl_batch_device, for csmp_rmps_batch"""
        b, x = self._greedy_batch_device(B, X, alpha_in, alpha_out)
        caps = tuple(self.M if c is None else int(c) for c in (maxiter, maxiter_acquisition, maxiter_deletion))
        return self._greedy_batch("csmp_rmps_batch", *b, sigma2, caps, min_increase, *x, history_cap, True)

    def fsbl_score(self, alpha, S, Q, mode):
        """csmp_fsbl_score (csmp_internal.h): (values Float64[N], pick, value, action) of one N-pass on a state of the caller's; mode: a key
        of FSBL_MODES"""
        arrs = [np.ascontiguousarray(v, dtype=np.float64) for v in (alpha, S, Q)]
        if any(v.shape != (self.N,) for v in arrs):
            raise CsmpError(EDIM, "alpha, S and Q have to be of length size(A, 2)")
        vals = np.zeros(max(self.N, 1), np.float64)
        pick, value, action = i64(0), C.c_double(0), C.c_int(0)
        self.call("csmp_fsbl_score", ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), int(FSBL_MODES[mode]), ptr(vals), C.byref(pick), C.byref(value),
                  C.byref(action))
        return vals[:self.N], int(pick.value), value.value, int(action.value)

    def fsbl_sqc(self, Cinv, S, Q, i, gamma):
        """csmp_fsbl_sqc (csmp_internal.h): (C⁻¹, S, Q) after the rank-one step sqc(i, gamma) on a state of the caller's"""
        Cinv = np.array(Cinv, dtype=np.float64, order="F")
        S, Q = np.array(S, dtype=np.float64), np.array(Q, dtype=np.float64)
        if Cinv.shape != (self.M, self.M) or S.shape != (self.N,) or Q.shape != (self.N,):
            raise CsmpError(EDIM, "Cinv has to be (size(A, 1), size(A, 1)), S and Q of length size(A, 2)")
        self.call("csmp_fsbl_sqc", ptr(Cinv), ptr(S), ptr(Q), i64(int(i)), C.c_double(gamma))
        return Cinv, S, Q

    def bench_fsbl(self, reps=5):
        """csmp_bench_fsbl (csmp_internal.h): average ms of the four parts of one greedy step on the state the last fsbl / rmps call left"""
        v = [C.c_double(0) for _ in range(4)]
        self.call("csmp_bench_fsbl", int(reps), *[C.byref(u) for u in v])
        return dict(zip(("score_ms", "colgemv_ms", "rank1_ms", "sweep_ms"), (u.value for u in v)))

    # ---- dictionary analysis
    def colnorms(self, device=False):
        """csmp_colnorms: ||a_j|| of every column, Float64[N] -- a numpy array, or (device=True) a torch CUDA tensor."""
        if device:
            import torch
            out = torch.empty(max(self.N, 1), dtype=torch.float64, device="cuda")
            self.call("csmp_colnorms", vp(out.data_ptr()), DEVICE)
            return out[:self.N]
        out = np.zeros(max(self.N, 1), np.float64)
        self.call("csmp_colnorms", ptr(out), HOST)
        return out[:self.N]

    def cumbabel(self, k, normalize=False):
        """csmp_cumbabel: (mu, pair) -- mu[m-1] = mu_1(m) for m = 1..k, and the 0-based columns (i, j), i < j, that attain mu_1(1)."""
        k = int(k)
        mu = np.zeros(max(k, 1), np.float64)
        pair = np.full(2, -1, np.int64)
        self.call("csmp_cumbabel", i64(k), int(normalize), ptr(mu), ptr(pair))
        return mu[:k], (int(pair[0]), int(pair[1]))

    # ---- primitives
    def sweep(self, r, topk=1, want_abs=True):
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (self.M,):
            raise CsmpError(EDIM, "length(r) != size(A, 1)")
        out = np.zeros(self.N, np.float64) if want_abs else None
        ti = np.zeros(max(int(topk), 1), np.int64)
        tv = np.zeros(max(int(topk), 1), np.float64)
        self.call("csmp_sweep", ptr(r), ptr(out), i64(int(topk)), ptr(ti), ptr(tv))
        return out, ti[:int(topk)], tv[:int(topk)]

    def lstsq(self, cols, b):
        b = self._b(b)
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        coef = np.zeros(len(cols), np.float64)
        self.call("csmp_lstsq", ptr(cols), i64(len(cols)), ptr(b), dtype_code(b.dtype), ptr(coef))
        return coef

    # ---- measurement
    def profile_enable(self, on=True):
        """on=True: time every sweep launch with HIP events; on=n>1: every n-th; False: off."""
        self.call("csmp_profile_enable", int(on))

    def profile_read(self, reset=True):
        n = i64(0)
        ms = C.c_double(0)
        self.call("csmp_profile_read", C.byref(n), C.byref(ms), int(bool(reset)))
        return n.value, ms.value

    def profile_window(self):
        """the timed launches of this context and its twin as one window (csmp_internal.h); call before profile_read"""
        n, w, d, st = i64(0), C.c_double(0), C.c_double(0), C.c_int(0)
        self.call("csmp_profile_window", C.byref(n), C.byref(w), C.byref(d), C.byref(st))
        return {"launches": int(n.value), "window_ms": w.value, "mean_launch_ms": d.value, "streams": st.value}

    def profile_overhead(self, reps=64):
        """average reading (ms) of an empty HIP-event pair on this context's stream"""
        ms = C.c_double(0)
        self.call("csmp_profile_overhead", int(reps), C.byref(ms))
        return ms.value

    def bench_sweep(self, variant=0, reps=20):
        ms = C.c_double(0)
        self.call("csmp_bench_sweep", int(variant), int(reps), C.byref(ms))
        return ms.value

    def bench_ard_forms(self, variant, reps, eps=1e-2):
        """csmp_bench_ard_forms (csmp_internal.h): (average ms of the N-pass, max |w fused - w split|) on the last ard_weights call's directions"""
        ms, diff = C.c_double(0), C.c_double(0)
        self.call("csmp_bench_ard_forms", int(variant), int(reps), C.c_double(eps), C.byref(ms), C.byref(diff))
        return ms.value, diff.value

    def sweep_config(self):
        """what configure_sweep chose for the resident dictionary (csmp_internal.h)"""
        unit, ph, wg, twg, lds, dyn, cpu = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), i64(0), C.c_int(0), C.c_int(0)
        self.call("csmp_sweep_config", C.byref(unit), C.byref(ph), C.byref(wg), C.byref(twg), C.byref(lds), C.byref(dyn), C.byref(cpu))
        grp = C.c_int(0)
        self.call("csmp_sweep_group", C.byref(grp))
        wide = C.c_int(0)
        self.call("csmp_sweep_group_wide", C.byref(wide))
        return {"unit_loads": unit.value, "phases": ph.value, "workgroups": wg.value, "tick_workgroups": twg.value,
                "lds_bytes": int(lds.value), "dynamic": dyn.value, "columns_per_unit": cpu.value, "group_max": grp.value, "group_wide": wide.value}

    def tune(self, key, value):
        """measurement override (csmp_internal.h): key in TUNE"""
        self.call("csmp_tune", int(TUNE[key]), i64(int(value)))


# ---- signal sharding: the wire layout of the ONE exchange (host memory, no ctx)
def shard_range(nsig, rank, world):
    lo, hi = i64(0), i64(0)
    rc = lib().csmp_shard_range(i64(int(nsig)), int(rank), int(world), C.byref(lo), C.byref(hi))
    if rc != OK:
        raise CsmpError(rc, "csmp_shard_range: bad arguments")
    return lo.value, hi.value


def pack_results(idx, val, nnz):
    """idx, val: (nsig, k) C-contiguous int64 / float64; nnz: (nsig,) int64 -> (nsig, 2k+1) float64 rows."""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    val = np.ascontiguousarray(val, dtype=np.float64)
    nnz = np.ascontiguousarray(nnz, dtype=np.int64)
    nsig, k = idx.shape
    out = np.empty((nsig, 2 * k + 1), np.float64)
    rc = lib().csmp_pack_results(ptr(idx), ptr(val), ptr(nnz), i64(k), i64(nsig), ptr(out))
    if rc != OK:
        raise CsmpError(rc, "csmp_pack_results: bad arguments")
    return out


def unpack_results(packed, k):
    packed = np.ascontiguousarray(packed, dtype=np.float64)
    nsig = packed.shape[0]
    idx = np.empty((nsig, k), np.int64)
    val = np.empty((nsig, k), np.float64)
    nnz = np.empty(nsig, np.int64)
    rc = lib().csmp_unpack_results(ptr(packed), i64(int(k)), i64(nsig), ptr(idx), ptr(val), ptr(nnz))
    if rc != OK:
        raise CsmpError(rc, "csmp_unpack_results: bad arguments")
    return idx, val, nnz
