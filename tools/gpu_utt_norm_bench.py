"""Cost of the per-utterance CMN / CVMN normalisation at the real shape, in one process: B = 256
utterances of 180 features x 321 frames, float32, both modes.  Alternating timed legs, device events around `iters` calls each:
  hip_time     dfa_utt_norm on the stored [256][180][324] batch (time fastest; one read, one write)
  hip_feat     dfa_utt_norm on a contiguous [256, 321, 180] tensor (feature fastest; cmn reads x twice, cvmn three times)
  hip_packed   dfa_utt_norm_packed, in place, on the same utterances as a packed resident set (its table is staged per call)
  torch_time   the reference's expression in torch on the GPU, x [256, 180, 321]: x - mean(-1) [/ std(-1).clamp(1e-8)]
  torch_feat   the same on x [256, 321, 180] over dim 1
Every leg walks `--buffers` distinct input / output pairs in turn (8 x 59 MB: more than the 256 MB Infinity Cache), so a call
reads its input from HBM, as the call in front of a forward does.  Prints one JSON line: per leg the median / min / max ms over
the pairs, and the bytes a single read and a single write of the batch take (2 x B x 180 x 321 x 4) over the median time, beside the
6.3 TB/s a float4 copy reaches on this chip (MI355X_MICROARCH.md): a fraction of the best a one-read-one-write pass could do.
usage: timeout -k 10 300 python tools/gpu_utt_norm_bench.py [--pairs 5] [--iters 16] [--buffers 8]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dfa_amd  # noqa: E402,F401
from dfa_amd import _lib  # noqa: E402
from dfa_amd.dataloaders import plan_packed_set  # noqa: E402

COPY_RATE = 6.3e12
B, F, T = 256, 180, 321
MODES = {"cmn": _lib.NORM_CMN, "cvmn": _lib.NORM_CVMN}


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def torch_norm(x, dim, mode):
    mean = x.mean(dim=dim, keepdim=True)
    if mode == "cmn":
        return x - mean
    return (x - mean) / x.std(dim=dim, keepdim=True).clamp(min=1e-8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--buffers", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("gpu_utt_norm_bench.py measures on the GPU: there is nothing to time without one")
    ctx = _lib.Context.get(torch.device("cuda", 0))
    lib, h = ctx.lib, ctx.handle
    R = args.buffers
    g = torch.Generator().manual_seed(1)
    base = torch.randn(B, F, T, generator=g) * 3.2 - 0.07
    t_pad = -(-T // 4) * 4
    stored = torch.zeros(B, F, t_pad)
    stored[:, :, :T] = base
    xs_time = [stored.to("cuda") for _ in range(R)]
    ys_time = [torch.empty_like(x) for x in xs_time]
    xs_feat = [base.transpose(1, 2).contiguous().to("cuda") for _ in range(R)]
    ys_feat = [torch.empty_like(x) for x in xs_feat]
    xs_tt = [base.to("cuda") for _ in range(R)]
    offsets, total = plan_packed_set([T] * B, F)
    lengths = np.full(B, T, dtype=np.int32)
    sets = [stored.reshape(-1).to("cuda") for _ in range(R)]                 # [T] * B packs to exactly the stored batch
    assert sets[0].numel() == total
    nbytes = int(lib.dfa_utt_norm_workspace_bytes(B))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ctx.use_current_stream()

    def hip(x, y, code):
        xv = x.transpose(1, 2)[:, :T] if x.shape[1] == F else x             # [B, T, F] either way
        rc = lib.dfa_utt_norm(h, code, _lib.ptr(x), _lib.ptr(y), B, T, F, *xv.stride(), None, _lib.ptr(ws), nbytes)
        _lib.check(h, rc)

    def hip_packed(s, code):
        rc = lib.dfa_utt_norm_packed(h, code, _lib.ptr(s), total, C.c_void_p(offsets.ctypes.data), C.c_void_p(lengths.ctypes.data), B, F,
                                     _lib.ptr(ws), nbytes)
        _lib.check(h, rc)

    out = {"B": B, "F": F, "T": T, "pairs": args.pairs, "iters": args.iters, "buffers": R, "copy_rate_TBps": COPY_RATE / 1e12}
    useful = 2.0 * B * F * T * 4
    for mode, code in MODES.items():
        legs = {
            "hip_time": lambda i: hip(xs_time[i % R], ys_time[i % R], code),
            "hip_feat": lambda i: hip(xs_feat[i % R], ys_feat[i % R], code),
            "hip_packed": lambda i: hip_packed(sets[i % R], code),
            "torch_time": lambda i: torch_norm(xs_tt[i % R], 2, mode),
            "torch_feat": lambda i: torch_norm(xs_feat[i % R], 1, mode),
        }
        res = {k: [] for k in legs}
        for fn in legs.values():
            for i in range(R):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(args.pairs):
            for name, fn in legs.items():
                res[name].append(timed(fn, args.iters))
        r = {}
        for name, v in res.items():
            med = float(np.median(v))
            r[name] = {"ms": [med, float(np.min(v)), float(np.max(v))], "one_read_one_write_TBps": useful / (med * 1e-3) / 1e12,
                       "fraction_of_copy_rate": useful / (med * 1e-3) / COPY_RATE}
        r["torch_time_over_hip_time"] = r["torch_time"]["ms"][0] / r["hip_time"]["ms"][0]
        r["torch_feat_over_hip_feat"] = r["torch_feat"]["ms"][0] / r["hip_feat"]["ms"][0]
        # the legs computed the same thing: the HIP outputs against torch's, at the tests' kind of bound (float32 rounding of the mean)
        want = torch_norm(xs_tt[0].double(), 2, mode)
        scale = float((xs_tt[0].abs().amax(dim=2) / (xs_tt[0].double().std(dim=2) if mode == "cvmn" else 1.0)).max())
        r["max_abs_diff_vs_float64_torch"] = {"time": float((ys_time[0][:, :, :T].double() - want).abs().max()),
                                              "feat": float((ys_feat[0].transpose(1, 2).double() - want).abs().max()),
                                              "unit_2^-24_max|x|/s": scale * 2.0 ** -24}
        out[mode] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
