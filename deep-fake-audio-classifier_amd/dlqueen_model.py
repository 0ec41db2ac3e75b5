"""DeepfakeDetector -- MI355X counterpart of the reference's src/dlqueen_model.py:115-173 (1D conv + StatsPool + wide channels,
the model its findings name as the winning recipe), eval forward and prediction CLI.  Training lives beside it:
training.DlqTrainer (the all-C-ABI step) and the CLI `python -m dfa_amd.train_dlqueen`.

Same constructor / state_dict / call contract: `model(x[B, C, T], lengths) -> logits[B]`.  x is the stored [C, T] layout of a
features.pkl row padded to the batch's longest utterance; the pool runs over each utterance's own frames.

The padded-batch rule.  The reference's encoder is NOT masked, only its pool is: frames past an
utterance's end hold zeros in x but GELU(BN(bias)) after layer 1, and the next layer reads them.  An utterance's logit therefore
depends on the utterance and on min(T - len, 2) -- how many padding frames follow it, up to two -- and on nothing else.  The HIP
forward reproduces exactly that, bit for bit independent of the batch: x past `len` is taken as zero and never used (it may hold
NaN), layer 1 exists on frames < min(T, len + 2), layer 2 on < min(T, len + 1), layer 3 on < len.

This module is eval-only: `model.train()(x, lengths)` and `--epochs > 0` are refused with a message that points at the trainer.
The training step is NOT a function of the utterance alone: the reference's BatchNorm1d counts every frame of the padded batch, so
a step depends on the batch's composition and on T_max; the promise above is an eval promise."""
from __future__ import annotations

import argparse
import ctypes as C
import os

import numpy as np
import torch
from torch import nn

from . import _lib
from ._params import BatchNormParams, ConvParams, LinearParams, Slots

TILE_FRAMES = 64     # DFA_DLQ_TILE_FRAMES: frames of one utterance a workgroup owns (tests probe the sizes around it)
_EVAL_ONLY = ("dfa_amd.dlqueen_model is eval-only: the DeepfakeDetector training step runs through dfa_amd.training.DlqTrainer "
              "(forward_train, BCE(pos_weight), backward, clip, AdamW, EMA on the C ABI) and the CLI `python -m dfa_amd.train_dlqueen`")


class _Encoder(nn.Module):
    """holds `net`, the reference's nn.Sequential indices that own parameters (src/dlqueen_model.py:135-150)"""

    def __init__(self, in_ch: int, hidden: int):
        super().__init__()
        slots = {}
        for ci, bi, (cin, k) in zip(DeepfakeDetector._CONV_IDX, DeepfakeDetector._BN_IDX, ((in_ch, 5), (hidden, 3), (hidden, 3))):
            slots[ci] = ConvParams(cin, hidden, (k,))
            slots[bi] = BatchNormParams(hidden)
        self.net = Slots(slots)


class DeepfakeDetector(nn.Module):
    _CONV_IDX = (0, 4, 8)
    _BN_IDX = (1, 5, 9)

    def __init__(self, in_ch: int, hidden: int = 256, dropout: float = 0.3):
        super().__init__()
        self.enc = _Encoder(in_ch, hidden)
        self.head = Slots({0: LinearParams(2 * hidden, hidden), 3: LinearParams(hidden, 1)})
        self.in_ch, self.hidden, self.dropout = int(in_ch), int(hidden), float(dropout)
        self._prepared = None

    def _abi_tensors(self):
        out = []
        for ci, bi in zip(self._CONV_IDX, self._BN_IDX):
            c, b = self.enc.net[ci], self.enc.net[bi]
            out += [c.weight, c.bias, b.weight, b.bias, b.running_mean, b.running_var]
        return out + [self.head[0].weight, self.head[0].bias, self.head[3].weight, self.head[3].bias]

    def _ensure_prepared(self, ctx):
        _lib.ensure_prepared(self, ctx, "dlq", "dfa_dlq_set_params", (self.in_ch, self.hidden), "dfa_dlq_prepare")

    @staticmethod
    def _conforms(x) -> bool:
        """float32, time fastest, 16-byte rows, and every row readable up to T rounded up to 4 frames"""
        B, Cc, T = x.shape
        sb, sc, st = x.stride()
        if x.dtype != torch.float32 or st != 1 or sc % 4 or sc < T or sb % 4 or sb < 0 or x.data_ptr() % 16:
            return False
        last = x.storage_offset() + (B - 1) * sb + (Cc - 1) * sc + -(-T // 4) * 4
        return last <= x.untyped_storage().nbytes() // 4

    def forward(self, x, lengths, return_pooled: bool = False):
        """x: [B, C, T] on the GPU; lengths: per-utterance frame counts (list, numpy array or int tensor), each in [1, T].
        -> logits [B] (and the pooled [B, 512] = [mean | std] vectors with return_pooled).  A float32 batch with time fastest and
        16-byte rows (what dataloaders.RaggedBatcher stages) is read in place; any other layout or dtype is first copied into
        such a batch on the GPU."""
        if self.training:
            raise NotImplementedError(_EVAL_ONLY + "; call model.eval()")
        if x.dim() != 3:
            raise ValueError(f"DeepfakeDetector expects x of shape (B, C, T), got {tuple(x.shape)}")
        _lib.require_gpu(self, x)       # (launch() asks again: here it keeps its place in front of the checks below)
        if not x.is_floating_point():
            raise ValueError(f"DeepfakeDetector takes a floating-point input, got {x.dtype}")
        B, Cc, T = x.shape
        lengths = _lib.host_lengths(lengths, B, T, 1)
        if B == 0:
            empty = torch.empty(0, dtype=torch.float32, device=x.device)
            return (empty, empty.reshape(0, 2 * self.hidden)) if return_pooled else empty
        x = _lib.stored_layout(x, self._conforms(x), time_last=True)
        sb, sc, _ = x.stride()
        with _lib.launch(self, x) as ctx:
            ws = ctx.workspace(ctx.lib.dfa_dlq_workspace_bytes(ctx.handle, B, T, Cc))
            logits = torch.empty(B, dtype=torch.float32, device=x.device)
            pooled = torch.empty((B, 2 * self.hidden), dtype=torch.float32, device=x.device) if return_pooled else None
            code = ctx.lib.dfa_dlq_forward(ctx.handle, _lib.ptr(x), B, T, Cc, sb, sc, C.c_void_p(lengths.ctypes.data),
                                           _lib.ptr(logits), _lib.ptr(pooled), _lib.ptr(ws), ws.numel())
            _lib.check(ctx.handle, code)
        return (logits, pooled) if return_pooled else logits


def _file_order_batches(feature_list, batch_size, device):
    """the reference's batches (src/dlqueen_model.py:98-111, shuffle=False): consecutive files, padded to the batch's longest"""
    for lo in range(0, len(feature_list), batch_size):
        utts = [torch.as_tensor(f).float() for f in feature_list[lo:lo + batch_size]]
        lengths = np.array([u.shape[-1] for u in utts], dtype=np.int32)
        T = int(lengths.max())
        host = torch.zeros((len(utts), utts[0].shape[0], -(-T // 4) * 4), dtype=torch.float32)
        for j, u in enumerate(utts):
            host[j, :, :u.shape[-1]] = u
        yield host.to(device)[:, :, :T], lengths


@torch.no_grad()
def run_inference(model, feature_list, batch_size: int = 32, device="cuda", use_prob: bool = False, file_order: bool = False,
                  norm: str = "raw"):
    """Scores of a list of per-utterance [C, T_i] tensors, in input order, as one tensor on `device`.  Default: batches from
    dataloaders.RaggedBatcher (longest first, order restored) -- an utterance's padding class min(T - len, 2) can then differ
    from the reference's file-order batches; file_order=True batches consecutive files as the reference does.
    norm: "cmn" / "cvmn" normalise every utterance over its own frames, in place in the batch's device copy."""
    from .dataloaders import RaggedBatcher
    from .normalization import normalize_batch
    model.eval()
    outs = []
    if file_order:
        for x, lengths in _file_order_batches(feature_list, batch_size, device):
            if norm != "raw":
                xt = x.transpose(1, 2)
                normalize_batch(xt, norm, lengths, out=xt)
            outs.append(model(x, lengths))
        scores = torch.cat(outs) if outs else torch.empty(0, device=device)
    else:
        batcher = RaggedBatcher(feature_list, None, batch_size, device=device, dtype=torch.float32)
        for xt, _, lengths in batcher:           # xt: [b, T_pad, C], the transposed view of the staged [b, C, T_pad] batch
            T = int(lengths.max())               # T_pad rounds the rows up to 16 bytes: the batch ends at its longest utterance
            if norm != "raw":
                normalize_batch(xt, norm, lengths, out=xt)
            outs.append(model(xt.transpose(1, 2)[:, :, :T], lengths))
        scores = batcher.restore(outs) if outs else torch.empty(0, device=device)
    return torch.sigmoid(scores) if use_prob else scores


@torch.no_grad()
def evaluate_eer(model, feature_list, labels, batch_size: int = 32, device="cuda", file_order: bool = False, norm: str = "raw") -> float:
    """EER of the logits against 0 / 1 labels (src/dlqueen_model.py:236-252)"""
    from .evaluation import calculate_eer
    scores = run_inference(model, feature_list, batch_size, device=device, file_order=file_order, norm=norm).cpu().numpy()
    eer, _thr = calculate_eer(np.asarray(scores, dtype=np.float64), np.asarray(labels))
    return float(eer)


@torch.no_grad()
def run_inference_resident(model, rset, batch_size: int = 32, use_prob: bool = False):
    """run_inference(..., file_order=True) on a dataloaders.DlqResidentSet: the same file-order batches, assembled on the device
    by the set's gather and read in place by the forward; the same scores, bit for bit.  (A set built with norm= holds
    normalised utterances: nothing is normalised here.)"""
    model.eval()
    outs = []
    for lo in range(0, len(rset), batch_size):
        x, lengths, _ = rset.batch(np.arange(lo, min(lo + batch_size, len(rset))))
        outs.append(model(x, lengths))
    scores = torch.cat(outs) if outs else torch.empty(0, device=rset.device)
    return torch.sigmoid(scores) if use_prob else scores


@torch.no_grad()
def evaluate_eer_resident(model, rset, labels, batch_size: int = 32) -> float:
    """evaluate_eer(..., file_order=True) on a resident set"""
    from .evaluation import calculate_eer
    scores = run_inference_resident(model, rset, batch_size).cpu().numpy()
    eer, _thr = calculate_eer(np.asarray(scores, dtype=np.float64), np.asarray(labels))
    return float(eer)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="DeepfakeDetector (Conv1d + StatsPool) prediction on the MI355X")
    ap.add_argument("--data_dir", default="data")
    ap.add_argument("--test_split", default="test2")
    ap.add_argument("--ckpt_path", default="best_model.pth")
    ap.add_argument("--prediction_pkl", default="prediction.pkl")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--epochs", type=int, default=0, help="must stay 0: training is dfa_amd.train_dlqueen")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--dropout", type=float, default=0.3)
    ap.add_argument("--use_prob", action="store_true", help="save sigmoid(prob) instead of logits")
    ap.add_argument("--file-order", dest="file_order", action="store_true",
                    help="batch consecutive files as the reference does (same padding classes) instead of sorting by length")
    from .normalization import add_norm_argument
    add_norm_argument(ap)         # not given: the checkpoint's "norm_mode", else raw (normalization.resolve_norm)
    args = ap.parse_args(argv)
    if args.epochs > 0:
        ap.exit(2, f"--epochs {args.epochs}: {_EVAL_ONLY}; train with `python -m dfa_amd.train_dlqueen` (or the reference) and pass its --ckpt_path\n")
    return args


def main(argv=None):
    import pandas as pd

    args = parse_args(argv)
    feat_path = os.path.join(args.data_dir, args.test_split, "features.pkl")
    lab_path = os.path.join(args.data_dir, args.test_split, "labels.pkl")
    df = pd.read_pickle(feat_path)
    if "uttid" not in df.columns or "features" not in df.columns:
        raise ValueError(f"{feat_path} needs the columns 'uttid' and 'features'")
    feats = [torch.as_tensor(f) for f in df["features"].tolist()]
    uttids = df["uttid"].tolist()
    if not os.path.exists(args.ckpt_path):
        raise FileNotFoundError(f"Checkpoint not found: {args.ckpt_path}")
    model = DeepfakeDetector(in_ch=int(feats[0].shape[0]), hidden=args.hidden, dropout=args.dropout)
    from .normalization import explicit_norm, resolve_norm
    blob = torch.load(args.ckpt_path, map_location="cpu")
    model.load_state_dict(blob["model_state"] if isinstance(blob, dict) and "model_state" in blob else blob)
    norm = resolve_norm(explicit_norm(args), blob)
    model = model.to(args.device).eval()
    logits = run_inference(model, feats, args.batch_size, device=args.device, file_order=args.file_order, norm=norm)
    scores = torch.sigmoid(logits) if args.use_prob else logits
    pred = pd.DataFrame({"uttid": uttids, "predictions": [float(s) for s in scores.cpu().numpy()]})
    pred.to_pickle(args.prediction_pkl)
    print(f"Saved prediction file -> {args.prediction_pkl}")
    print(pred.head())
    print("shape:", pred.shape)
    if os.path.exists(lab_path):
        from .evaluation import calculate_eer
        lab = pd.read_pickle(lab_path)
        label_map = dict(zip(lab["uttid"].tolist(), lab["label"].tolist()))
        y = np.array([int(label_map[u]) for u in uttids])
        eer, _thr = calculate_eer(logits.cpu().numpy().astype(np.float64), y)
        print(f"\nEER on split '{args.test_split}': {float(eer):.6f}")
    else:
        print("\nDone! (Inference only on unlabeled split, no EER computed)")


if __name__ == "__main__":
    main()
