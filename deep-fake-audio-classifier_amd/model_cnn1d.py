"""CNN1D -- MI355X counterpart of the reference's src/model_cnn1d.py:5-46.

Same constructor / state_dict / call contract (`model(x[B,T,F]) -> logits[B,1]`).  The reference transposes to
[B,F,T] for Conv1d (model_cnn1d.py:40); here that transpose is free: the kernels address x through its strides, and
the stored feature layout [B,180,321] already is channel-major.  Arithmetic is fp32 (this path is bound by reading
the input once: 30.8 MFLOP per 231 KB utterance)."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib
from ._params import BatchNormParams, ConvParams, LinearParams, Slots


KERNEL_SETS = ((3, 3, 3), (5, 3, 3))     # the Conv1d kernel sizes the HIP path is built for


def check_kernels(kernels) -> tuple:
    """`kernels` as a tuple of three ints, or ValueError naming the two supported sets: (3, 3, 3) -- src/model_cnn1d.py -- and
    (5, 3, 3), the reference's CNN1D_Variant (src/compare_kernels.py:38-67)."""
    try:
        k = tuple(int(v) for v in kernels)
    except (TypeError, ValueError):
        k = None
    if k not in KERNEL_SETS:
        raise ValueError(f"CNN1D kernels={kernels!r}: the HIP path is built for kernels=(3, 3, 3) and kernels=(5, 3, 3) only")
    return k


def parse_kernels(text: str) -> tuple:
    """The CLIs' `--kernels 5,3,3`."""
    try:
        return check_kernels(int(v) for v in text.split(","))
    except ValueError:
        raise ValueError(f"--kernels {text}: the supported sets are 3,3,3 and 5,3,3") from None


def resolve_kernels(flag, checkpoint_blob) -> tuple:
    """The kernel sizes a scoring CLI builds its CNN1D with.  Pure, the rule of normalization.resolve_norm: an explicit `flag`
    wins; else the checkpoint's "kernels" (the key src/compare_kernels.py:178-184 writes); else (3, 3, 3).  A flag that
    contradicts the checkpoint warns on stderr."""
    import sys
    saved = checkpoint_blob.get("kernels") if isinstance(checkpoint_blob, dict) else None
    if saved is not None:
        saved = check_kernels(saved)
    if flag is None:
        return saved or (3, 3, 3)
    flag = check_kernels(flag)
    if flag != (saved or (3, 3, 3)):
        print(f"warning: --kernels {','.join(map(str, flag))} but the checkpoint was trained with "
              f"kernels={saved or (3, 3, 3)}", file=sys.stderr)
    return flag


class CNN1D(nn.Module):
    _CONV_IDX = (0, 4, 8)     # reference nn.Sequential indices that own parameters (src/model_cnn1d.py:15-32)
    _BN_IDX = (1, 5, 9)

    def __init__(self, in_features=180, base_channels=32, num_classes=1, dropout=0.2, kernels=(3, 3, 3)):
        """kernels: (3, 3, 3), or (5, 3, 3) -- the reference's CNN1D_Variant(kernels=(5, 3, 3)) of src/compare_kernels.py:38-67
        (conv.0.weight [32, F, 5], padding 2; same state_dict keys).  That variant has the eval forward, uniform and ragged, and
        the uniform training step; its ragged training step is refused by name."""
        super().__init__()
        if num_classes != 1:
            raise ValueError("dfa_amd.CNN1D implements the binary head (num_classes=1) the reference trains")
        self.kernels = check_kernels(kernels)
        bc = base_channels
        chans = [(in_features, bc), (bc, 2 * bc), (2 * bc, 4 * bc)]
        slots = {}
        for ci, bi, (cin, cout), k in zip(self._CONV_IDX, self._BN_IDX, chans, self.kernels):
            slots[ci] = ConvParams(cin, cout, (k,))
            slots[bi] = BatchNormParams(cout)
        self.conv = Slots(slots)
        self.classifier = LinearParams(4 * bc, num_classes)
        self.in_features, self.base_channels, self.dropout = in_features, base_channels, float(dropout)
        self._prepared = None

    def _abi_tensors(self):
        out = []
        for ci, bi in zip(self._CONV_IDX, self._BN_IDX):
            c, b = self.conv[ci], self.conv[bi]
            out += [c.weight, c.bias, b.weight, b.bias, b.running_mean, b.running_var]
        return out + [self.classifier.weight, self.classifier.bias]

    def _ensure_prepared(self, ctx):
        _lib.ensure_prepared(self, ctx, "cnn1d", "dfa_cnn1d_set_params", (self.in_features, self.base_channels),
                             "dfa_cnn1d_prepare", before=("dfa_cnn1d_set_kernels", self.kernels))

    def forward(self, x, lengths=None):
        """lengths: None (every utterance spans all T frames: the reference's call), or the per-utterance frame counts of a
        ragged batch padded to T (a list, numpy array or int tensor, each in [3, T]): utterance b is scored from
        x[b, :lengths[b]] alone, in one kernel launch for the whole batch, whatever its length; its padding is never used.
        Eval mode only."""
        if x.dim() != 3:
            raise ValueError(f"CNN1D expects x of shape (B, T, F), got {tuple(x.shape)}")
        if self.training:
            if lengths is not None:
                raise NotImplementedError("ragged batches (lengths=...) are eval-only: batch-norm statistics over a "
                                          "variable-length batch have no reference definition")
            from .training import cnn1d_train_forward
            return cnn1d_train_forward(self, x)
        if lengths is not None:
            lengths = _lib.host_lengths(lengths, x.shape[0], x.shape[1], 3)
        return self._forward(x, lengths)

    def _forward(self, x, lengths):
        """x: float32 [B, T, F] on the GPU; lengths: None, or the checked host int32 array of a ragged batch.  The ragged kernel
        reads the stored channel-major layout -- the transposed view of a [B, F, T_pad] batch with T_pad % 4 == 0, what
        dataloaders.RaggedBatcher yields -- in place.  A tensor in any other layout (a contiguous [B, T, F], a pitch that is not a
        multiple of 4, a misaligned base) is first copied into such a zero-padded channel-major batch on the GPU; the result is
        the same."""
        _lib.require_gpu(self, x)       # (launch() asks again: here it keeps its place in front of the dtype check)
        if x.dtype != torch.float32:
            raise ValueError(f"CNN1D takes float32 input, got {x.dtype}")
        B, T, F = x.shape
        if lengths is not None:
            sb, st, sf = x.stride()
            x = _lib.stored_layout(x, not B or (st == 1 and sf % 4 == 0 and sf >= T and sb % 4 == 0 and sb >= 0
                                                and x.data_ptr() % 16 == 0), time_last=False)
        with _lib.launch(self, x) as ctx:
            lib = ctx.lib
            planner = lib.dfa_workspace_bytes if lengths is None else lib.dfa_ragged_workspace_bytes
            ws = ctx.workspace(planner(ctx.handle, _lib.MODEL_CNN1D, B, T, F, _lib.PREC_F32))
            logits = torch.empty((B, 1), dtype=torch.float32, device=x.device)
            head = (ctx.handle, _lib.ptr(x), _lib.DTYPE_F32, B, T, F, *x.stride())
            tail = (_lib.ptr(logits), _lib.ptr(ws), ws.numel())
            if lengths is None:
                code = lib.dfa_cnn1d_forward(*head, *tail)
            else:
                code = lib.dfa_cnn1d_forward_ragged(*head, C.c_void_p(lengths.ctypes.data), *tail)
            _lib.check(ctx.handle, code)
        return logits


if __name__ == "__main__":
    model = CNN1D().to("cuda").eval()
    print(f"CNN1D output shape: {model(torch.randn(4, 321, 180, device='cuda')).shape}")
