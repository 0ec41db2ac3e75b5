"""Throughput of the DeepfakeDetector (Conv1d + StatsPool) eval forward, in one process, alternating timed legs of
  uniform   [256, 180, 321] (every length 321),
  ragged    B=256, lengths drawn with a fixed seed uniformly from [161, 481] (mean 321),
  ragged32  the first 32 of those lengths (the reference's batch size) in one call,
  loop      the same 32 utterances one call at a time.
Prints one JSON line: per leg the median utt/s and frames/s over the pairs with min and max, per pair ragged32 / loop, the
per-kernel times of the uniform and ragged legs from the timing slots (4-6 = layers 1-3, 7 = pool + head; one extra call each,
outside the timed loops), the useful FLOP rate (1,247,232 FLOP per frame) and the rate of the bf16 matrix-core work issued
(six MFMAs per product: 6 x the padded GEMM FLOP of the launched tiles) as a fraction of the 2.5 PFLOP/s dense bf16 peak.
--cpu: also the fp32 torch statement of the model on the host's cores (uniform [32, 180, 321], utt/s), as the CPU baseline.
--parity: prints max |gpu - float64| / S of the golden fixture's padded batch instead of timing.
usage: timeout -k 10 300 python tools/gpu_dlqueen_bench.py [--pairs 5] [--iters 10] [--cpu] [--parity]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dfa_amd  # noqa: E402,F401
from dfa_amd import _lib  # noqa: E402
from dfa_amd.dlqueen_model import TILE_FRAMES, DeepfakeDetector  # noqa: E402

FLOP_PER_FRAME = 2 * 256 * (5 * 180 + 3 * 256 + 3 * 256)        # 1,247,232
PEAK_BF16 = 2.5e15


def issued_flop(lengths, T_max, C=180):
    """bf16 matrix-core FLOP of the launched tiles: 64-frame tiles (a tile whose frames end in its first half runs one of its
    two 32-frame halves), K padded to 16 channels per tap, six MFMAs per product"""
    total = 0
    for ext, k in ((2, 5 * -(-C // 16) * 16), (1, 3 * 256), (0, 3 * 256)):
        for n in lengths:
            e = min(T_max, int(n) + ext)
            full, rest = divmod(e, TILE_FRAMES)
            frames = full * TILE_FRAMES + (0 if rest == 0 else (32 if rest <= 32 else 64))
            total += 6 * 2 * 256 * k * frames
    return total


def parity():
    import dlqueen_oracle as DO
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "dlqueen_eval.npz")))
    sd = DO.fixture_state_dict(g, DeepfakeDetector)
    m = DeepfakeDetector(180)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    x, lengths = DO.pad_batch(DO.split_utts(g))
    lg, pooled = m(x._base.to("cuda")[:, :, :x.shape[2]], lengths, return_pooled=True)
    S = float(g["S"])
    print(json.dumps({"logits_err_over_S": float(np.abs(lg.double().cpu().numpy() - g["batch.logits64"]).max()) / S,
                      "pooled_err_over_max": float(np.abs(pooled.double().cpu().numpy() - g["batch.pooled64"]).max()
                                                   / np.abs(g["batch.pooled64"]).max()), "bound": 2.0 ** -17}))


def cpu_baseline(model):
    import dlqueen_oracle as DO
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x = torch.randn(32, 180, 321) * 3.2 - 0.07
    DO.forward(sd, x, [321] * 32, dtype=torch.float32)
    t0 = time.perf_counter()
    for _ in range(3):
        DO.forward(sd, x, [321] * 32, dtype=torch.float32)
    return 3 * 32 / (time.perf_counter() - t0), torch.get_num_threads()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--parity", action="store_true")
    args = ap.parse_args()
    if args.parity:
        return parity()
    torch.manual_seed(0)
    model = DeepfakeDetector(180).to("cuda").eval()
    lengths = np.random.default_rng(321).integers(161, 482, size=256).astype(np.int32)
    gen = torch.Generator().manual_seed(1)

    def batch(lens):
        T = int(max(lens))
        x = torch.zeros(len(lens), 180, -(-T // 4) * 4)
        for i, n in enumerate(lens):
            x[i, :, :n] = torch.randn(180, int(n), generator=gen) * 3.2 - 0.07
        return x.to("cuda")[:, :, :T]

    uni_l = np.full(256, 321, dtype=np.int32)
    x_uni, x_rag, x_32 = batch(uni_l), batch(lengths), batch(lengths[:32])
    singles = [batch(lengths[i:i + 1]) for i in range(32)]
    legs = {
        "uniform": (lambda: model(x_uni, uni_l), 256, int(uni_l.sum())),
        "ragged": (lambda: model(x_rag, lengths), 256, int(lengths.sum())),
        "ragged32": (lambda: model(x_32, lengths[:32]), 32, int(lengths[:32].sum())),
        "loop": (lambda: [model(s, lengths[i:i + 1]) for i, s in enumerate(singles)], 32, int(lengths[:32].sum())),
    }
    res = {k: [] for k in legs}
    for _ in range(2):
        for fn, _, _ in legs.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.pairs):
        for name, (fn, _, _) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            t1.synchronize()
            res[name].append(t0.elapsed_time(t1) / args.iters)
    out = {"model": "dlqueen", "pairs": args.pairs, "iters": args.iters, "mean_length": float(lengths.mean())}
    for name, v in res.items():
        ms = np.array(v)
        _, n, frames = legs[name]
        out[name] = {"ms": [float(np.median(ms)), float(ms.min()), float(ms.max())],
                     "utt_per_s": [float(n / np.median(ms) * 1e3), float(n / ms.max() * 1e3), float(n / ms.min() * 1e3)],
                     "frames_per_s": float(frames / np.median(ms) * 1e3)}
    out["ragged32_over_loop"] = [float(a / b) for a, b in zip(res["loop"], res["ragged32"])]
    ctx = _lib.Context.get(torch.device("cuda"))
    for name, lens in (("uniform", uni_l), ("ragged", lengths)):
        ctx.timing_reset()
        ctx.timing(1)
        legs[name][0]()
        torch.cuda.synchronize()
        ctx.timing(0)
        slots = {s: ctx.timing_read(s)[0] for s in (4, 5, 6, 7)}
        layers = sum(slots[s] for s in (4, 5, 6))
        out[name]["kernel_ms"] = {"layer1": slots[4], "layer2": slots[5], "layer3": slots[6], "pool_head": slots[7]}
        out[name]["useful_tflops"] = float(FLOP_PER_FRAME * int(lens.sum()) / (np.median(res[name]) * 1e-3) / 1e12)
        out[name]["issued_bf16_fraction_of_peak"] = float(issued_flop(lens, int(lens.max())) / (layers * 1e-3) / PEAK_BF16)
    if args.cpu:
        out["cpu_fp32_utt_per_s"], out["cpu_threads"] = cpu_baseline(model)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
