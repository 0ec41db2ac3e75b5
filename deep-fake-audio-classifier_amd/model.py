"""CNN2D -- MI355X counterpart of the reference's src/model.py:5-42.

Same constructor, same state_dict keys/shapes/parameter order, same call contract
(`model(x[B,T,F]) -> logits[B,1]`, `model(x, return_embedding=True) -> (logits, emb[B, 128*F])`), but `forward`
enqueues the hand-written HIP kernels of libdfa_hip.so (conv1 -> MFMA block 2 -> MFMA block 3 + time mean ->
linear) instead of torch layers.  Input may be the non-contiguous transposed view the reference harness feeds
(src/predict.py:105): strides are passed through, nothing is copied.
"""
from __future__ import annotations

import ctypes as C
import os

import torch
from torch import nn

from . import _lib
from ._params import BatchNormParams, ConvParams, LinearParams, Slots


class CNN2D(nn.Module):
    """2-D CNN over the time x feature grid (reference: src/model.py:5-42).

    precision: "fp32" (default; exact-fp32 MFMA, logits within 1e-4 of the reference), "bf16" (bf16 storage, fp32
    accumulate: the throughput mode of BASELINE.json configs[1]) or "bf16x3" (eval only: hi + lo bf16 operands, three bf16
    MFMAs per product -- logits within 1e-4 of the reference at several times the fp32 rate).  Env DFA_PRECISION overrides
    the default.
    """

    # reference nn.Sequential indices that own parameters (src/model.py:13-29)
    _CONV_IDX = (0, 5, 10)
    _BN_IDX = (1, 6, 11)

    def __init__(self, in_features=180, base_channels=32, num_classes=1, dropout=0.2, precision=None):
        super().__init__()
        if num_classes != 1:
            raise ValueError("dfa_amd.CNN2D implements the binary head (num_classes=1) the reference trains")
        bc = base_channels
        chans = [(1, bc), (bc, 2 * bc), (2 * bc, 4 * bc)]
        slots = {}
        for ci, bi, (cin, cout) in zip(self._CONV_IDX, self._BN_IDX, chans):
            slots[ci] = ConvParams(cin, cout, (3, 3))      # draws RNG in reference order: conv weight, conv bias
            slots[bi] = BatchNormParams(cout)
        self.conv = Slots(slots)
        self.classifier = LinearParams(4 * bc * in_features, num_classes)
        self.in_features = in_features
        self.base_channels = base_channels
        self.dropout = float(dropout)
        self.precision = (precision or os.environ.get("DFA_PRECISION", "fp32")).lower()
        if self.precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {self.precision!r}")
        self._prepared = None   # (device index, precision, tensors signature)

    # ---- parameter plumbing ------------------------------------------------------------------------------------
    def _abi_tensors(self):
        """The 20 tensors of dfa_cnn2d_set_params, in include/dfa_hip.h order."""
        out = []
        for ci, bi in zip(self._CONV_IDX, self._BN_IDX):
            c, b = self.conv[ci], self.conv[bi]
            out += [c.weight, c.bias, b.weight, b.bias, b.running_mean, b.running_var]
        out += [self.classifier.weight, self.classifier.bias]
        return out

    def set_precision(self, precision: str) -> "CNN2D":
        precision = precision.lower()
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        self.precision = precision
        return self

    def _ensure_prepared(self, ctx: "_lib.Context"):
        _lib.ensure_prepared(self, ctx, "cnn2d", "dfa_cnn2d_set_params", (self.in_features, self.base_channels),
                             "dfa_cnn2d_prepare", self.precision)

    # ---- forward -----------------------------------------------------------------------------------------------
    def forward(self, x, return_embedding=False, lengths=None):
        """lengths: None (every utterance spans all T frames: the reference's call), or the per-utterance frame counts of a
        ragged batch padded to T (a list, numpy array or int tensor): utterance b is scored as x[b:b+1, :lengths[b]] alone
        would be, and its padding rows are never read.  Ragged batches run in bf16 precision, eval mode only."""
        if x.dim() != 3:
            raise ValueError(f"CNN2D expects x of shape (B, T, F), got {tuple(x.shape)}")
        if self.training:
            if lengths is not None:
                raise NotImplementedError("ragged batches (lengths=...) are eval-only: batch-norm statistics over a "
                                          "variable-length batch have no reference definition")
            from .training import cnn2d_train_forward  # train-mode path (batch-stat BN, dropout, autograd)
            return cnn2d_train_forward(self, x, return_embedding)
        if lengths is not None:
            lengths = _lib.host_lengths(lengths, x.shape[0], x.shape[1], 4)
        return self._forward(x, return_embedding, lengths)

    def _forward(self, x, return_embedding, lengths):
        """lengths: None, or the checked host int32 array of a ragged batch"""
        B, T, F = x.shape
        with _lib.launch(self, x) as ctx:
            lib, prec = ctx.lib, _lib.PRECISIONS[self.precision]
            planner = lib.dfa_workspace_bytes if lengths is None else lib.dfa_ragged_workspace_bytes
            ws = ctx.workspace(planner(ctx.handle, _lib.MODEL_CNN2D, B, T, F, prec))
            logits = torch.empty((B, 1), dtype=torch.float32, device=x.device)
            emb = torch.empty((B, 4 * self.base_channels * F), dtype=torch.float32, device=x.device) \
                if return_embedding else None
            head = (ctx.handle, _lib.ptr(x), _lib.x_dtype_code(x), B, T, F, *x.stride())
            tail = (_lib.ptr(logits), _lib.ptr(emb), _lib.ptr(ws), ws.numel())
            if lengths is None:
                code = lib.dfa_cnn2d_forward(*head, *tail)
            else:
                code = lib.dfa_cnn2d_forward_ragged(*head, C.c_void_p(lengths.ctypes.data), *tail)
            _lib.check(ctx.handle, code)
        if return_embedding:
            return logits, emb
        return logits


if __name__ == "__main__":
    model = CNN2D().to("cuda").eval()
    x = torch.randn(4, 321, 180, device="cuda")
    print(f"CNN2D output shape: {model(x).shape}")
