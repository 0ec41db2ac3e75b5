"""ctypes binding of libdfa_hip.so (include/dfa_hip.h).  There is no CPU fallback: if the shared library is
missing or a call fails, an exception is raised (ValueError for shape/dtype errors, RuntimeError otherwise,
mirroring how the reference surfaces torch shape errors and its own ValueErrors)."""
from __future__ import annotations

import collections
import ctypes as C
import os
import threading

import torch

from ._params import tensors_signature

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdfa_hip.so")

DFA_OK = 0
E_BAD_SHAPE, E_BAD_DTYPE, E_NULL_PTR, E_NOT_PREPARED, E_HIP, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6, -7
DTYPE_F32, DTYPE_BF16 = 0, 1
PREC_F32, PREC_BF16, PREC_BF16X3 = 0, 1, 2
MODEL_CNN2D, MODEL_CNN1D, MODEL_CAE = 0, 1, 2
EMB_OCSVM, EMB_GMM, EMB_MAX_P, EMB_MAX_K = 0, 1, 256, 64
NORM_CMN, NORM_CVMN, UTT_NORM_HELD_FRAMES, UTT_NORM_MAX_PACKED = 1, 2, 1024, 65536
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32, "bf16": PREC_BF16, "bfloat16": PREC_BF16,
              "bf16x3": PREC_BF16X3}

_lib = None
_lock = threading.Lock()

# (name, restype, argtypes): every symbol include/dfa_hip.h declares
SYMBOLS = [
    ("dfa_version", C.c_int, []),
    ("dfa_ctx_create", C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("dfa_ctx_destroy", C.c_int, [C.c_void_p]),
    ("dfa_ctx_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("dfa_ctx_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ("dfa_ctx_get_option", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    ("dfa_last_error", C.c_char_p, [C.c_void_p]),
    ("dfa_error_name", C.c_char_p, [C.c_int]),
    ("dfa_cnn2d_set_params", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn2d_prepare", C.c_int, [C.c_void_p, C.c_int]),
    ("dfa_cnn2d_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cnn2d_train_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn2d_train_plan", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]),
    ("dfa_cnn2d_forward_train", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                          C.c_int64, C.c_int64, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_float,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cnn2d_backward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    ("dfa_bce_smooth_fwd_bwd", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    ("dfa_augment_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                    C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64]),
    ("dfa_cnn2d_set_train_augment", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_float, C.c_uint64, C.c_uint64]),
    ("dfa_cnn1d_set_train_augment", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_float, C.c_uint64, C.c_uint64]),
    ("dfa_ctx_set_bn_sync", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("dfa_adamw_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float]),
    ("dfa_cnn1d_set_params", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn1d_prepare", C.c_int, [C.c_void_p]),
    ("dfa_cnn1d_set_kernels", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn1d_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cnn1d_train_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn1d_forward_train", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                          C.c_int64, C.c_int64, C.c_float, C.c_uint64, C.c_uint64, C.c_float, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cnn1d_backward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    ("dfa_cnn1d_train_ragged_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn1d_train_plan", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]),
    ("dfa_cnn1d_forward_train_ragged", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                                 C.c_int64, C.c_int64, C.c_void_p, C.c_float, C.c_uint64, C.c_uint64, C.c_float,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cnn1d_backward_ragged", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                            C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    ("dfa_cae_set_params", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    ("dfa_cae_prepare", C.c_int, [C.c_void_p, C.c_int]),
    ("dfa_cae_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_size_t]),
    ("dfa_cae_train_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dfa_cae_train_plan", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int]),
    ("dfa_cae_forward_train", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                        C.c_int64, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t]),
    ("dfa_cae_backward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                   C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    ("dfa_mse_fwd_bwd", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                  C.c_int64, C.c_void_p, C.c_void_p]),
    ("dfa_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dfa_ragged_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn2d_forward_ragged", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                           C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_size_t]),
    ("dfa_cnn1d_forward_ragged", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                           C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cae_ragged_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dfa_cae_score_ragged", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_dlq_set_params", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
    ("dfa_dlq_prepare", C.c_int, [C.c_void_p]),
    ("dfa_dlq_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("dfa_dlq_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_dlq_train_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("dfa_dlq_forward_train", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_float, C.c_uint64, C.c_uint64, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t]),
    ("dfa_dlq_backward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                   C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    ("dfa_dlq_gather_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("dfa_dlq_gather_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]),
    ("dfa_utt_norm_workspace_bytes", C.c_size_t, [C.c_int]),
    ("dfa_utt_norm", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                               C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_utt_norm_packed", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_size_t]),
    ("dfa_bce_pos_weight_fwd_bwd", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    ("dfa_clip_grad_norm", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]),
    ("dfa_emb_ocsvm_bind", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]),
    ("dfa_emb_gmm_bind", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    ("dfa_emb_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dfa_emb_ocsvm_score", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_emb_gmm_score", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("dfa_cnn1d_ragged_segments", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.c_int]),
    ("dfa_cnn1d_ragged_lds_bytes", C.c_size_t, [C.c_int, C.c_int]),
    ("dfa_cnn1d_ragged_segments_k", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.c_int]),
    ("dfa_cnn1d_ragged_lds_bytes_k", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("dfa_cnn1d_fused_max_t", C.c_int, [C.c_int, C.c_int]),
    ("dfa_dominant_kernel", C.c_char_p, [C.c_int, C.c_int]),
    ("dfa_ctx_timing_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("dfa_ctx_timing_reset", C.c_int, [C.c_void_p]),
    ("dfa_ctx_timing_read", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("dfa_ctx_last_conv123_form", C.c_int, [C.c_void_p]),
    ("dfa_ctx_last_conv123_phase", C.c_int, [C.c_void_p]),
    ("dfa_ctx_last_conv123_cls", C.c_int, [C.c_void_p]),
    ("dfa_cnn2d_forward_plan", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                         C.POINTER(C.c_longlong), C.c_int]),
    ("dfa_ctx_debug_read", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]),
    ("dfa_ctx_clock_read", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int)]),
]


def load():
    """dlopen libdfa_hip.so once and declare prototypes.  Raises RuntimeError when it has not been built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or `make -C deep-fake-audio-classifier_amd/csrc`).  dfa_amd has no CPU fallback.")
            lib = C.CDLL(LIB_PATH)
            for name, res, args in SYMBOLS:
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            _lib = lib
    return _lib


CNN2D_PLAN_FIELDS = ("H1", "H2", "a1_off", "a2_off", "emb_off", "slabs", "tab_off", "tab_words", "total", "path", "form", "phase",
                     "grid", "lds", "seg12", "seg3", "chunk3", "nseg3", "split3")
CNN2D_PLAN_OPTIONS = ("time_split", "fuse_conv1", "block3_m16", "fuse_blocks123", "persist123", "carry_a1", "phase123")
CNN2D_PATH_CONV1, CNN2D_PATH_CONV12, CNN2D_PATH_CONV123 = 0, 1, 2


def cnn2d_forward_plan(ctx_handle, B, T, F, precision, ragged=False, options=None, num_cus=0):
    """dfa_cnn2d_forward_plan as a tuple in the order of CNN2D_PLAN_FIELDS: for the context's options and CU count, or, with
    ctx_handle None, for `options` (seven values in the order of CNN2D_PLAN_OPTIONS; None = the defaults) and `num_cus`."""
    out = (C.c_longlong * len(CNN2D_PLAN_FIELDS))()
    opts = None if options is None else (C.c_int * len(CNN2D_PLAN_OPTIONS))(*options)
    n = load().dfa_cnn2d_forward_plan(ctx_handle, B, T, F, precision, int(ragged), opts, num_cus, out, len(out))
    if n != len(out):
        raise ValueError(f"dfa_cnn2d_forward_plan([{B}, {T}, {F}]) returned {n}, not {len(out)} fields")
    return tuple(out)


class CaeTrainPlan:
    """dfa_cae_train_plan as named fields (the order of include/dfa_hip.h): H, W, Hd, Wd, the byte offsets e, z, zd, d, dd, dzd, de,
    dz (tuples; z[0] = dz[0] = -1), zp, xf, raw, stats, sums, wq, dwq, rec, partial, partial_bytes, total, elem, and per BatchNorm
    layer C, mean, var, invstd."""
    _GROUPS = (("H", 5), ("W", 5), ("Hd", 4), ("Wd", 4), ("e", 4), ("z", 4), ("zd", 3), ("d", 3), ("dd", 3), ("dzd", 3), ("de", 4),
               ("dz", 4), ("zp", 0), ("xf", 0), ("raw", 0), ("stats", 0), ("sums", 0), ("wq", 0), ("dwq", 0), ("rec", 0), ("partial", 0),
               ("partial_bytes", 0), ("total", 0), ("elem", 0), ("C", 7), ("mean", 7), ("var", 7), ("invstd", 7))
    NFIELDS = sum(max(n, 1) for _, n in _GROUPS)

    def __init__(self, fields):
        self.fields = tuple(fields)
        i = 0
        for name, n in self._GROUPS:
            setattr(self, name, self.fields[i] if n == 0 else self.fields[i:i + n])
            i += max(n, 1)


def cae_train_plan(ctx_handle, B, T, F, precision):
    """The workspace layout of a ConvAutoencoder training step (dfa_cae_train_plan); a refused shape or precision raises as the
    step itself would (the message needs a context)."""
    out = (C.c_longlong * CaeTrainPlan.NFIELDS)()
    n = load().dfa_cae_train_plan(ctx_handle, B, T, F, precision, out, len(out))
    if n < 0:
        check(ctx_handle, n)
    if n != len(out):
        raise ValueError(f"dfa_cae_train_plan([{B}, {T}, {F}]) returned {n}, not {len(out)} fields")
    return CaeTrainPlan(out)


CNN2D_TRAIN_PLAN_FIELDS = ("H1", "H2", "elem", "a1", "z2", "a2", "z3", "emb", "demb", "msum", "dz3", "da2", "dz2", "da1", "raw", "stats",
                           "sums", "partial", "partial_bytes", "total")
Cnn2dTrainPlan = collections.namedtuple("Cnn2dTrainPlan", CNN2D_TRAIN_PLAN_FIELDS)


def cnn2d_train_plan(ctx_handle, B, T, F, precision):
    """The workspace layout of a CNN2D training step (dfa_cnn2d_train_plan) as named fields in the order of include/dfa_hip.h; a
    refused shape or precision raises as the step itself would (the message needs a context)."""
    out = (C.c_longlong * len(CNN2D_TRAIN_PLAN_FIELDS))()
    n = load().dfa_cnn2d_train_plan(ctx_handle, B, T, F, precision, out, len(out))
    if n < 0:
        check(ctx_handle, n)
    if n != len(out):
        raise ValueError(f"dfa_cnn2d_train_plan([{B}, {T}, {F}]) returned {n}, not {len(out)} fields")
    return Cnn2dTrainPlan(*out)


class Cnn1dTrainPlan:
    """dfa_cnn1d_train_plan as named fields (the order of include/dfa_hip.h): the byte offsets z, h, dz, dh (tuples, one per layer),
    pooled, dpooled, stats, sums, partial, partial_bytes, lengths (-1: a uniform batch), total."""
    _GROUPS = (("z", 3), ("h", 2), ("pooled", 0), ("dpooled", 0), ("dz", 3), ("dh", 2), ("stats", 0), ("sums", 0), ("partial", 0),
               ("partial_bytes", 0), ("lengths", 0), ("total", 0))
    NFIELDS = sum(max(n, 1) for _, n in _GROUPS)

    def __init__(self, fields):
        self.fields = tuple(fields)
        i = 0
        for name, n in self._GROUPS:
            setattr(self, name, self.fields[i] if n == 0 else self.fields[i:i + n])
            i += max(n, 1)


def cnn1d_train_plan(ctx_handle, B, T, F, ragged=False):
    """The workspace layout of a CNN1D training step (dfa_cnn1d_train_plan), of a ragged batch padded to T frames with
    ragged=True; a refused shape raises as the step itself would (the message needs a context)."""
    out = (C.c_longlong * Cnn1dTrainPlan.NFIELDS)()
    n = load().dfa_cnn1d_train_plan(ctx_handle, B, T, F, int(ragged), out, len(out))
    if n < 0:
        check(ctx_handle, n)
    if n != len(out):
        raise ValueError(f"dfa_cnn1d_train_plan([{B}, {T}, {F}]) returned {n}, not {len(out)} fields")
    return Cnn1dTrainPlan(out)


def check(ctx_handle, code):
    if code == DFA_OK:
        return
    lib = load()
    msg = lib.dfa_last_error(ctx_handle).decode() if ctx_handle else ""
    text = f"{lib.dfa_error_name(code).decode()}: {msg}"
    if code in (E_BAD_SHAPE, E_BAD_DTYPE, E_UNSUPPORTED):
        raise ValueError(text)
    raise RuntimeError(text)


class Context:
    """One dfa_ctx per (process, device).  Holds the activation workspace (a torch uint8 tensor: storage only)."""
    _by_device: dict = {}

    def __init__(self, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError(f"dfa_amd runs on an AMD GPU (torch device 'cuda'), got device '{device}'. "
                               "There is no CPU path.")
        self.device = device
        self.index = device.index if device.index is not None else torch.cuda.current_device()
        self.lib = load()
        h = C.c_void_p()
        code = self.lib.dfa_ctx_create(self.index, None, C.byref(h))
        if code != DFA_OK:
            raise RuntimeError(f"dfa_ctx_create(device={self.index}) failed: {self.lib.dfa_error_name(code).decode()}")
        self.handle = h
        self._ws = None
        # A dfa_ctx has ONE weight slot per model class (cnn2d / cnn1d / cae).  _owner remembers which nn.Module bound a
        # slot last, so a model whose own cache looks valid still re-binds after ANOTHER model of its class used the slot
        # (two live CNN2D instances used alternately).  _train_gen counts train-mode forwards per slot: a backward whose
        # forward is no longer the slot's latest would read another forward's saved activations and raises instead.
        self._owner = {}
        self._train_gen = {}

    @classmethod
    def get(cls, device) -> "Context":
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in cls._by_device:
            cls._by_device[idx] = Context(torch.device("cuda", idx))
        return cls._by_device[idx]

    def owner_changed(self, kind: str, model) -> bool:
        """Claim the ctx's `kind` weight slot for `model`; True when another model held it (caches must be rebuilt)."""
        token = model.__dict__.get("_ctx_token")
        if token is None:
            token = model.__dict__["_ctx_token"] = object()
        changed = self._owner.get(kind) is not token
        self._owner[kind] = token
        return changed

    def next_train_gen(self, kind: str) -> int:
        g = self._train_gen.get(kind, 0) + 1
        self._train_gen[kind] = g
        return g

    def check_train_gen(self, kind: str, gen: int, model=None):
        if model is not None and self._owner.get(kind) is not model.__dict__.get("_ctx_token"):
            raise RuntimeError(
                f"backward of a {kind} train-mode forward after ANOTHER {kind} model used this device's weight slot: "
                "run backward before calling a second model of the same class")
        if self._train_gen.get(kind) != gen:
            raise RuntimeError(
                f"backward of a {kind} train-mode forward that is no longer the latest one on this device: the saved "
                "activations live in one workspace per model class and were overwritten by a later train-mode forward. "
                "Call backward before the next forward (losses of two forwards cannot be summed on this path).")

    def use_current_stream(self):
        s = torch.cuda.current_stream(self.index).cuda_stream
        check(self.handle, self.lib.dfa_ctx_set_stream(self.handle, C.c_void_p(s)))

    def workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=torch.device("cuda", self.index))
        return self._ws

    def set_option(self, name: str, value: int):
        check(self.handle, self.lib.dfa_ctx_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        value = C.c_int(0)
        check(self.handle, self.lib.dfa_ctx_get_option(self.handle, name.encode(), C.byref(value)))
        return value.value

    # ---- timing -----------------------------------------------------------------------------------------------
    def timing(self, enable):
        """False/0 = off, True/1 = every slot, other int = bit mask of slots (1 << slot)."""
        check(self.handle, self.lib.dfa_ctx_timing_enable(self.handle, int(enable)))

    def timing_reset(self):
        check(self.handle, self.lib.dfa_ctx_timing_reset(self.handle))

    def timing_read(self, slot: int):
        ms, n = C.c_float(), C.c_int()
        check(self.handle, self.lib.dfa_ctx_timing_read(self.handle, slot, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_conv123_form(self) -> int:
        """Blocks 1-3 of the last CNN2D eval forward: 0 = separate kernels, 1 = one workgroup per unit, 2 = persistent,
        3 = persistent with carried a1 columns (dfa_ctx_last_conv123_form)."""
        return int(self.lib.dfa_ctx_last_conv123_form(self.handle))

    def last_conv123_phase(self) -> int:
        """1 if the last CNN2D eval forward ran the de-phased build of the carry form (option "phase123"), else 0."""
        return int(self.lib.dfa_ctx_last_conv123_phase(self.handle))

    def last_conv123_cls(self) -> int:
        """1 if the last CNN2D eval forward computed the logits inside the blocks 1-3 kernel (option "cls123"), else 0."""
        return int(self.lib.dfa_ctx_last_conv123_cls(self.handle))

    def clock_read(self):
        """(median, min, max GHz, workgroups) of the last bf16 CNN2D block-3 launch run with set_option("clock_probe", 1)."""
        med, lo, hi, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        check(self.handle, self.lib.dfa_ctx_clock_read(self.handle, C.byref(med), C.byref(lo), C.byref(hi), C.byref(n)))
        return med.value, lo.value, hi.value, n.value


class BnSync:
    """Synchronised BatchNorm for data-parallel training (dfa_ctx_set_bn_sync): while armed on the device's context, every
    BatchNorm layer's per-channel sums are added over the ranks of `process_group` between their reduction and their use, so
    N ranks x B utterances behave like one rank x N*B.  Built once per trainer (sync buffer and callback); the hook is global
    to the context and must stay the same across a forward / backward pair (the library refuses a backward whose forward found
    it otherwise), so its owner arms it around exactly that pair."""
    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)

    def __init__(self, device, process_group=None):
        import torch.distributed as dist
        self.ctx = Context.get(device)
        buf = self.buf = torch.zeros(1024, dtype=torch.float32, device=self.ctx.device)

        def hook(_user, _buf, count):
            try:       # in place, ordered after the work already on the current (= the context's) stream
                dist.all_reduce(buf[:count], op=dist.ReduceOp.SUM, group=process_group)
                return 0
            except Exception:   # noqa: BLE001 -- reported through the C ABI's error path
                return -1
        self._fn = self.FN(hook)                        # keeps the callback alive as long as the hook object
        self._armed = (C.cast(self._fn, C.c_void_p), None, dist.get_world_size(process_group), C.c_void_p(buf.data_ptr()),
                       buf.numel())

    def arm(self):
        check(self.ctx.handle, self.ctx.lib.dfa_ctx_set_bn_sync(self.ctx.handle, *self._armed))

    def disarm(self):
        check(self.ctx.handle, self.ctx.lib.dfa_ctx_set_bn_sync(self.ctx.handle, None, None, 1, None, 0))


def x_dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return DTYPE_F32
    if t.dtype == torch.bfloat16:
        return DTYPE_BF16
    raise ValueError(f"dfa_amd kernels take float32 or bfloat16 input, got {t.dtype}")


def ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- the eval bridge: what every model's eval-mode forward does around its one ABI call --------------------------------------------
def ensure_prepared(model, ctx: Context, slot: str, set_params: str, dims, prepare: str, precision=None, before=None):
    """Bind model._abi_tensors() to the context's `slot` (`set_params`(ctx, pointers, n, *dims)) and fold them for the eval
    forward (`prepare`(ctx[, precision code])), unless that is what the slot already holds: model._prepared remembers the
    signature (device, precision where the model has one, tensor addresses and versions) of the last preparation.
    before: (name, args) of a sticky setter of the slot that goes in front of every `set_params` (the CNN1D's kernel sizes)."""
    ts = model._abi_tensors()
    for t in ts:
        if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{type(model).__name__} parameters must be contiguous float32 tensors on the GPU "
                               "(call model.to('cuda')); dfa_amd has no CPU path")
    sig = (ctx.index, tensors_signature(ts)) if precision is None else (ctx.index, precision, tensors_signature(ts))
    stale = ctx.owner_changed(slot, model)      # another model of this class used the ctx's weight slot
    if sig == model._prepared and not stale:
        return
    arr = ptr_array([t.detach() for t in ts])
    if before is not None:
        check(ctx.handle, getattr(ctx.lib, before[0])(ctx.handle, *before[1]))
    check(ctx.handle, getattr(ctx.lib, set_params)(ctx.handle, arr, len(ts), *dims))
    check(ctx.handle, getattr(ctx.lib, prepare)(ctx.handle, *(() if precision is None else (PRECISIONS[precision],))))
    model._prepared = sig


def require_gpu(model, x):
    if x.device.type != "cuda":
        raise RuntimeError(f"dfa_amd.{type(model).__name__} runs on the GPU only: move the input with .to('cuda')")


class launch:
    """`with launch(model, x) as ctx`: the context of x's device, ready for one eval-mode ABI call on `model` -- x's device
    current, the context on torch's current stream, the model's weights prepared.  (A class, not a contextlib generator: this
    runs once per forward, and the generator's frame costs about a microsecond of it.)"""
    __slots__ = ("model", "ctx", "guard")

    def __init__(self, model, x):
        require_gpu(model, x)
        self.model, self.ctx = model, Context.get(x.device)
        self.guard = torch.cuda.device(self.ctx.index)

    def __enter__(self):
        self.guard.__enter__()
        try:
            self.ctx.use_current_stream()
            self.model._ensure_prepared(self.ctx)
        except BaseException:
            self.guard.__exit__(None, None, None)
            raise
        return self.ctx

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


def stored_layout(x, in_place: bool, time_last: bool):
    """A float32 batch in the stored channel-major layout [B][C][T_pad] (time fastest, rows of T_pad = T rounded up to 4 frames:
    16-byte rows): x itself when the caller's test `in_place` found it to be one already, else a zero-padded copy on x's device.
    time_last: x is [B, C, T] (else [B, T, C]); the result has x's shape."""
    if in_place:
        return x
    cm = x if time_last else x.transpose(1, 2)
    B, Cc, T = cm.shape
    stored = torch.zeros((B, Cc, -(-T // 4) * 4), dtype=torch.float32, device=x.device)
    stored[:, :, :T] = cm
    return stored[:, :, :T] if time_last else stored.transpose(1, 2)[:, :T]


def host_lengths(lengths, B: int, T_max: int, min_len: int):
    """Per-utterance frame counts of a ragged batch (list, numpy array or int tensor on any device) -> a contiguous host
    int32 numpy array, checked against the batch: one length per row, each in [min_len, T_max]."""
    import numpy as np

    if isinstance(lengths, torch.Tensor):
        if lengths.is_floating_point() or lengths.is_complex():
            raise ValueError(f"lengths must be integers, got a {lengths.dtype} tensor")
        lengths = lengths.detach().cpu().numpy()
    arr = np.asarray(lengths)
    if arr.ndim != 1:
        raise ValueError(f"lengths must be one-dimensional, got shape {arr.shape}")
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"lengths must be integers, got dtype {arr.dtype}")
    if arr.shape[0] != B:
        raise ValueError(f"got {arr.shape[0]} lengths for a batch of {B}")
    bad = np.nonzero((arr < min_len) | (arr > T_max))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"lengths[{i}]={int(arr[i])} is outside [{min_len}, T_max={T_max}]")
    return np.ascontiguousarray(arr, dtype=np.int32)
