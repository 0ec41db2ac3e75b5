"""Per-utterance CMN / CVMN feature normalisation -- counterpart of NormalizedDataset.__getitem__
(src/compare_normalization.py:53-62, src/compare_kernels.py:83-90); DESIGN.md section 3.17.

For a stored utterance feat [F, T]:  cmn: feat - mean_t;  cvmn: (feat - mean_t) / std_t.clamp(min=1e-8), std unbiased.
`normalize_utterance` is the reference's host expression (the DataLoader path).  `normalize_batch` / `normalize_packed_` run on the
GPU (dfa_utt_norm, dfa_utt_norm_packed): each utterance over its own `lengths[b]` frames, zero behind them.  "raw" is no call."""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import numpy as np
import torch

from . import _lib

MODES = ("raw", "cmn", "cvmn")
_CODES = {"cmn": _lib.NORM_CMN, "cvmn": _lib.NORM_CVMN}


def check_mode(mode: str) -> str:
    if mode not in MODES:
        raise ValueError(f"norm must be one of {MODES}, got {mode!r}")
    return mode


def normalize_utterance(feat: torch.Tensor, mode: str) -> torch.Tensor:
    """The reference's expression on one stored utterance [F, T] (time is dim 1), on whatever device it is."""
    check_mode(mode)
    feat = feat.float()
    if mode == "cmn":
        feat = feat - feat.mean(dim=1, keepdim=True)
    elif mode == "cvmn":
        mean = feat.mean(dim=1, keepdim=True)
        std = feat.std(dim=1, keepdim=True).clamp(min=1e-8)
        feat = (feat - mean) / std
    return feat


def _time_fastest(x: torch.Tensor) -> bool:
    """x [B, T, F] is the stored [B][F][T_pad] layout the time-fastest kernel reads in place: time fastest, 16-byte rows, and
    every row's whole 16-byte pieces (T rounded up to 4 frames) inside x's storage -- the kernel reads and writes them."""
    B, T, F = x.shape
    sb, st, sc = x.stride()
    if st != 1 or sc % 4 or sc < T or sb % 4 or sb < 0 or x.data_ptr() % 16:
        return False
    last = x.storage_offset() + (B - 1) * sb + (F - 1) * sc + -(-T // 4) * 4
    return last <= x.untyped_storage().nbytes() // 4


def _feature_fastest(x: torch.Tensor) -> bool:
    return x.stride(2) == 1 and x.stride(1) != 1 and x.stride(1) >= x.shape[2] and x.stride(0) >= 0


def _empty_like_layout(x: torch.Tensor, time_fastest: bool) -> torch.Tensor:
    """A fresh tensor with x's shape and strides.  Time fastest: the kernel writes whole 16-byte pieces, so the last row's
    pitch is allocated too."""
    B, T, F = x.shape
    if not time_fastest:
        return torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    t_pad = -(-T // 4) * 4
    sb = x.stride(0) if B > 1 else 0
    buf = torch.empty((B - 1) * sb + (F - 1) * x.stride(2) + t_pad, dtype=torch.float32, device=x.device)
    if buf.data_ptr() % 16:
        raise RuntimeError("the output buffer is not 16-byte aligned")
    return buf.as_strided(x.shape, x.stride())


def normalize_batch(x: torch.Tensor, mode: str, lengths=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """x [B, T, F] float32 on the GPU (any layout) -> the normalised batch, each utterance over its own lengths[b] frames
    (None: all T), +0.0 behind them.  "raw" returns x itself.  A layout the kernels do not read in place (neither the stored
    [B][F][T_pad] form nor feature fastest) is first copied with _lib.stored_layout; the result then has that layout.
    out: a tensor of x's shape AND strides (x itself: in place), else a new one is returned."""
    check_mode(mode)
    if mode == "raw":
        return x
    if x.dim() != 3:
        raise ValueError(f"normalize_batch takes [B, T, F], got shape {tuple(x.shape)}")
    if x.device.type != "cuda":
        raise RuntimeError("normalize_batch runs on the GPU only (normalize_utterance is the host expression)")
    if x.dtype != torch.float32:
        raise ValueError(f"normalize_batch takes float32 input, got {x.dtype}")
    B, T, F = x.shape
    lens = None if lengths is None else _lib.host_lengths(lengths, B, T, 2 if mode == "cvmn" else 1)
    tf = _time_fastest(x)
    if not tf and not _feature_fastest(x):
        if out is not None:
            raise ValueError("out= needs an input the kernels read in place (the stored [B][F][T_pad] layout or feature fastest)")
        x = _lib.stored_layout(x, False, time_last=False)
        tf = True
        out = x                                            # the copy is ours: normalise it in place
    if out is None:
        out = _empty_like_layout(x, tf)
    elif out.shape != x.shape or out.stride() != x.stride() or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError("out must have x's shape, strides, dtype and device")
    elif tf and not _time_fastest(out):
        raise ValueError("out must be 16-byte aligned and hold every row up to T rounded up to 4 frames")
    ctx = _lib.Context.get(x.device)
    with torch.cuda.device(ctx.index):
        ctx.use_current_stream()
        nbytes = int(ctx.lib.dfa_utt_norm_workspace_bytes(B))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)    # (not the context's: a model's forward may be using that)
        code = ctx.lib.dfa_utt_norm(ctx.handle, _CODES[mode], _lib.ptr(x), _lib.ptr(out), B, T, F, x.stride(0), x.stride(1), x.stride(2),
                                    None if lens is None else C.c_void_p(lens.ctypes.data), _lib.ptr(ws), nbytes)
        _lib.check(ctx.handle, code)
    return out


def normalize_stored(feats: torch.Tensor, mode: str, lengths=None) -> torch.Tensor:
    """normalize_batch for a batch in the stored layout [B, F, T] (time last, as a features.pkl and the flat file hold it and
    the loaders yield it): what the reference's dataset does to each utterance before the loop swaps the axes."""
    if check_mode(mode) == "raw":
        return feats
    return normalize_batch(feats.transpose(1, 2), mode, lengths).transpose(1, 2)


def normalize_packed_(packed: torch.Tensor, offsets, lengths, C_: int, mode: str) -> torch.Tensor:
    """In place on a packed resident set (dataloaders.plan_packed_set: utterance i = C_ rows of pitch ceil(T_i / 4) * 4 floats
    from float offset offsets[i] of the flat float32 device buffer `packed`).  The set is walked in chunks of the ABI's cap."""
    check_mode(mode)
    if mode == "raw":
        return packed
    if packed.device.type != "cuda" or packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("normalize_packed_ takes a flat contiguous float32 buffer on the GPU")
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
    if offs.shape != lens.shape:
        raise ValueError(f"got {offs.shape[0]} offsets for {lens.shape[0]} lengths")
    ctx = _lib.Context.get(packed.device)
    cap = _lib.UTT_NORM_MAX_PACKED
    with torch.cuda.device(ctx.index):
        ctx.use_current_stream()
        for lo in range(0, lens.shape[0], cap):
            n = min(cap, lens.shape[0] - lo)
            nbytes = int(ctx.lib.dfa_utt_norm_workspace_bytes(n))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
            o, l = offs[lo:lo + n], lens[lo:lo + n]
            code = ctx.lib.dfa_utt_norm_packed(ctx.handle, _CODES[mode], _lib.ptr(packed), packed.numel(), C.c_void_p(o.ctypes.data),
                                               C.c_void_p(l.ctypes.data), n, int(C_), _lib.ptr(ws), nbytes)
            _lib.check(ctx.handle, code)
    return packed


class _NormFlag(argparse.Action):
    """--norm: stores the mode and records that it was given (a scoring CLI lets an explicit flag overrule the checkpoint)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.norm_explicit = True


def add_norm_argument(parser) -> None:
    """`--norm {raw,cmn,cvmn}` (default raw) on a CLI's parser; args.norm_explicit tells whether it was given."""
    parser.add_argument("--norm", default="raw", choices=list(MODES), action=_NormFlag,
                        help="per-utterance feature normalisation on the GPU: cmn = subtract each feature row's mean over time, "
                             "cvmn = also divide by its standard deviation (src/compare_normalization.py); default raw = none")
    parser.set_defaults(norm_explicit=False)


def explicit_norm(args):
    """The --norm a user typed, or None."""
    return args.norm if getattr(args, "norm_explicit", False) else None


def resolve_norm(flag, checkpoint_blob) -> str:
    """The mode a scoring CLI uses.  Pure: an explicit `flag` wins; else the checkpoint's "norm_mode" (the key
    src/compare_kernels.py:178-184 writes); else "raw".  A flag that contradicts the checkpoint warns on stderr."""
    saved = checkpoint_blob.get("norm_mode") if isinstance(checkpoint_blob, dict) else None
    if saved is not None:
        check_mode(saved)
    if flag is None:
        return saved or "raw"
    check_mode(flag)
    if flag != (saved or "raw"):
        print(f"warning: --norm {flag} but the checkpoint was trained with norm_mode={saved or 'raw'}", file=sys.stderr)
    return flag
