"""Ragged throughput of CNN2D (bf16, the default), CNN1D (--model cnn1d, fp32 features) or the auto-encoder's anomaly score
(--model cae, bf16, raw features with the z-score fused): in one process, alternating timed legs of
  ragged   B=256, F=180, lengths drawn with a fixed seed uniformly from [161, 481] (mean 321),
  uniform  [256, 321, 180],
  ragged32 the first 32 of those lengths (the reference's predict batch size),
  loop     the same 32 utterances one call at a time (what a user runs without lengths=; for cnn1d each utterance is its own
           contiguous [F, T_i] tensor, copied outside the timed region, so the uniform split-bf16 kernel takes those it can).
Prints one JSON line: per leg the median utt/s and frames/s over the pairs, with min and max, and per pair ragged32 / loop.
--stamps (cnn1d): one extra ragged call with the kernel's clock stamps on, reporting the share of the stamped workgroups'
time spent in multi-segment utterances.
--model cnn1d --train: the TRAINING step (NativeTrainer.step: forward, loss, backward, fused AdamW; dropout 0.2, tiny lr) in
three alternating legs: ragged B=256 with lengths drawn with a fixed seed from [161, 384] (the matrix-core convolutions reach
T <= 384), uniform_tmax [256, 384, 180] (the same convolution work) and uniform_mean [256, mean length, 180] (the same frames).
usage: timeout -k 10 300 python tools/gpu_ragged_bench.py [--model cnn2d|cnn1d|cae] [--train] [--pairs 5] [--iters 20] [--stamps]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dfa_amd  # noqa: E402,F401
from dfa_amd.model import CNN2D  # noqa: E402


def train_legs(args):
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.training.train_step import NativeTrainer
    lengths = np.random.default_rng(321).integers(161, 385, size=256)
    T_max, T_mean = 384, int(round(float(lengths.mean())))
    gen = torch.Generator().manual_seed(1)
    y = (torch.rand(256, generator=gen) > 0.5).float().to("cuda")
    xs = {T: (torch.randn(256, 180, T, generator=gen) * 3.2 - 0.07).to("cuda").transpose(1, 2) for T in (T_max, T_mean)}
    torch.manual_seed(0)
    tr = NativeTrainer(CNN1D(dropout=0.2).to("cuda"), label_smoothing=0.05, lr=1e-6)     # tiny lr: every leg times the same regime
    legs = {
        "ragged": (lambda: tr.step(xs[T_max], y, lengths), int(lengths.sum())),
        "uniform_tmax": (lambda: tr.step(xs[T_max], y), 256 * T_max),
        "uniform_mean": (lambda: tr.step(xs[T_mean], y), 256 * T_mean),
    }
    res = {k: [] for k in legs}
    for _ in range(3):
        for fn, _ in legs.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.pairs):
        for name, (fn, _) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            t1.synchronize()
            res[name].append(t0.elapsed_time(t1) / args.iters)
    out = {"model": "cnn1d", "mode": "train", "pairs": args.pairs, "iters": args.iters, "T_max": T_max, "T_mean": T_mean,
           "mean_length": float(lengths.mean())}
    for name, v in res.items():
        ms = np.array(v)
        out[name] = {"step_ms": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
                     "utt_per_s": 256e3 / float(np.median(ms)), "frames_per_s": legs[name][1] * 1e3 / float(np.median(ms))}
    out["ragged_over_uniform_tmax_ms"] = out["ragged"]["step_ms"] / out["uniform_tmax"]["step_ms"]
    out["ragged_over_uniform_mean_ms"] = out["ragged"]["step_ms"] / out["uniform_mean"]["step_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model", default="cnn2d", choices=["cnn2d", "cnn1d", "cae"])
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--train", action="store_true", help="cnn1d: time the training step instead of the forward")
    args = ap.parse_args()
    if args.train:
        if args.model != "cnn1d":
            ap.error("--train: the variable-length training step exists for --model cnn1d only")
        return train_legs(args)
    torch.manual_seed(0)
    lengths = np.random.default_rng(321).integers(161, 482, size=256)
    T_max = int(lengths.max())
    gen = torch.Generator().manual_seed(1)
    l32 = lengths[:32]
    if args.model == "cnn1d":
        from dfa_amd.model_cnn1d import CNN1D
        model = CNN1D().to("cuda").eval()
        T_pad = -(-T_max // 4) * 4                       # 16-byte rows, as dataloaders.RaggedBatcher pads
        xr = (torch.randn(256, 180, T_pad, generator=gen) * 3.2).to("cuda").transpose(1, 2)[:, :T_max]
        xu = (torch.randn(256, 180, 321, generator=gen) * 3.2).to("cuda").transpose(1, 2)
        own = [xr[i, :int(T)].t().contiguous()[None].transpose(1, 2) for i, T in enumerate(l32)]
        loop = lambda: [model(u) for u in own]           # noqa: E731
    elif args.model == "cae":
        from dfa_amd.model_cae import ConvAutoencoder
        cae = ConvAutoencoder(precision="bf16").to("cuda").eval()
        mean, std = torch.randn(180, generator=gen).to("cuda"), (torch.rand(180, generator=gen) + 0.5).to("cuda")
        xr = (torch.randn(256, 180, T_max, generator=gen) * 3.2).to(torch.bfloat16).to("cuda").transpose(1, 2)
        xu = (torch.randn(256, 180, 321, generator=gen) * 3.2).to(torch.bfloat16).to("cuda").transpose(1, 2)
        model = lambda x, lengths=None: cae.score(x, mean, std, lengths=lengths)     # noqa: E731
        loop = lambda: [model(xr[i:i + 1, :int(T)]) for i, T in enumerate(l32)]      # noqa: E731
    else:
        model = CNN2D(precision="bf16").to("cuda").eval()
        xr = (torch.randn(256, 180, T_max, generator=gen) * 3.2).to(torch.bfloat16).to("cuda").transpose(1, 2)
        xu = (torch.randn(256, 180, 321, generator=gen) * 3.2).to(torch.bfloat16).to("cuda").transpose(1, 2)
        loop = lambda: [model(xr[i:i + 1, :int(T)]) for i, T in enumerate(l32)]      # noqa: E731
    x32 = xr[:32, :int(l32.max())]
    legs = {
        "ragged": (lambda: model(xr, lengths=lengths), 256, int(lengths.sum())),
        "uniform": (lambda: model(xu), 256, 256 * 321),
        "ragged32": (lambda: model(x32, lengths=l32), 32, int(l32.sum())),
        "loop": (loop, 32, int(l32.sum())),
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
    out = {"model": args.model, "precision": "fp32 (split bf16)" if args.model == "cnn1d" else "bf16", "pairs": args.pairs, "iters": args.iters, "mean_length": float(lengths.mean())}
    for name, v in res.items():
        u = np.array([a for a, _ in v]); f = np.array([b for _, b in v])
        out[name] = {"utt_per_s": float(np.median(u)), "utt_min": float(u.min()), "utt_max": float(u.max()),
                     "frames_per_s": float(np.median(f)), "frames_min": float(f.min()), "frames_max": float(f.max())}
    out["ragged_over_uniform_utt"] = out["ragged"]["utt_per_s"] / out["uniform"]["utt_per_s"]
    out["ragged_over_uniform_frames"] = out["ragged"]["frames_per_s"] / out["uniform"]["frames_per_s"]
    out["ragged32_over_loop"] = out["ragged32"]["utt_per_s"] / out["loop"]["utt_per_s"]
    out["ragged32_over_loop_pairs"] = [a[0] / b[0] for a, b in zip(res["ragged32"], res["loop"])]
    if args.stamps and args.model == "cnn1d":
        # stamps of the (up to 128) first utterances: [8b] start, [8b + 3] end (s_memtime), [8b + 5] / [8b + 6] the same in
        # s_memrealtime, [8b + 4] length, [8b + 7] segments
        import ctypes as C
        from dfa_amd import _lib
        ctx = _lib.Context.get(torch.device("cuda"))
        ctx.set_option("clock_probe", 1)
        model(xr, lengths=lengths)
        torch.cuda.synchronize()
        buf = (C.c_longlong * 1024)()
        _lib.check(ctx.handle, ctx.lib.dfa_ctx_debug_read(ctx.handle, buf, 1024))
        ctx.set_option("clock_probe", 0)
        st = np.array(buf[:], dtype=np.int64).reshape(128, 8)
        dur, nseg = (st[:, 3] - st[:, 0]).astype(np.float64), st[:, 7]
        ok = (st[:, 4] == lengths[:128]) & (dur > 0)
        real = (st[:, 6] - st[:, 5]).astype(np.float64) / 100.0          # s_memrealtime ticks at 100 MHz -> microseconds
        out["stamps"] = {"workgroups": int(ok.sum()), "longest_workgroup_us": float(real[ok].max()),
                         "median_workgroup_us": float(np.median(real[ok])),
                         "span_first_start_to_last_end_us": float((st[ok, 6].max() - st[ok, 5].min()) / 100.0), "multi_segment_workgroups": int((ok & (nseg > 1)).sum()),
                         "multi_segment_time_share": float(dur[ok & (nseg > 1)].sum() / max(dur[ok].sum(), 1.0)),
                         "cycles_per_frame_one_segment": float((dur / np.maximum(st[:, 4], 1))[ok & (nseg == 1)].mean()) if (ok & (nseg == 1)).any() else None,
                         "cycles_per_frame_multi_segment": float((dur / np.maximum(st[:, 4], 1))[ok & (nseg > 1)].mean()) if (ok & (nseg > 1)).any() else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
