"""Ragged CNN2D throughput (bf16): in one process, alternating timed legs of
  ragged   B=256, F=180, lengths drawn with a fixed seed uniformly from [161, 481] (mean 321),
  uniform  [256, 321, 180],
  ragged32 the first 32 of those lengths (the reference's predict batch size),
  loop     the same 32 utterances one call at a time (what a user runs without lengths=).
Prints one JSON line: per leg the median utt/s and frames/s over the pairs, with min and max.
usage: timeout -k 10 300 python tools/gpu_ragged_bench.py [--pairs 5] [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dfa_amd  # noqa: E402,F401
from dfa_amd.model import CNN2D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    model = CNN2D(precision="bf16").to("cuda").eval()
    lengths = np.random.default_rng(321).integers(161, 482, size=256)
    T_max = int(lengths.max())
    gen = torch.Generator().manual_seed(1)
    xr = (torch.randn(256, 180, T_max, generator=gen) * 3.2).to(torch.bfloat16).to("cuda").transpose(1, 2)
    xu = (torch.randn(256, 180, 321, generator=gen) * 3.2).to(torch.bfloat16).to("cuda").transpose(1, 2)
    l32 = lengths[:32]
    x32 = xr[:32, :int(l32.max())]
    legs = {
        "ragged": (lambda: model(xr, lengths=lengths), 256, int(lengths.sum())),
        "uniform": (lambda: model(xu), 256, 256 * 321),
        "ragged32": (lambda: model(x32, lengths=l32), 32, int(l32.sum())),
        "loop": (lambda: [model(xr[i:i + 1, :int(T)]) for i, T in enumerate(l32)], 32, int(l32.sum())),
    }
    res = {k: [] for k in legs}
    for _ in range(2):                                   # warm-up: preparation, workspace, clocks
        for fn, _, _ in legs.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.pairs):
        for name, (fn, n_utt, n_frames) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            t1.synchronize()
            s = t0.elapsed_time(t1) / 1e3 / args.iters
            res[name].append((n_utt / s, n_frames / s))
    out = {"precision": "bf16", "pairs": args.pairs, "iters": args.iters, "mean_length": float(lengths.mean())}
    for name, v in res.items():
        u = np.array([a for a, _ in v]); f = np.array([b for _, b in v])
        out[name] = {"utt_per_s": float(np.median(u)), "utt_min": float(u.min()), "utt_max": float(u.max()),
                     "frames_per_s": float(np.median(f)), "frames_min": float(f.min()), "frames_max": float(f.max())}
    out["ragged_over_uniform_utt"] = out["ragged"]["utt_per_s"] / out["uniform"]["utt_per_s"]
    out["ragged_over_uniform_frames"] = out["ragged"]["frames_per_s"] / out["uniform"]["frames_per_s"]
    out["ragged32_over_loop"] = out["ragged32"]["utt_per_s"] / out["loop"]["utt_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
