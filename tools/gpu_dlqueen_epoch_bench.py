"""DeepfakeDetector training EPOCH on the MI355X: the host loop (train_dlqueen.epoch_batches: batches built in Python, SpecAugment
by slice assignment, x.to(device), the step's own re-layout copy) against the resident loop (dataloaders.DlqResidentSet +
train_dlqueen.resident_epoch_batches: one dfa_dlq_gather_batch launch per batch), both feeding the same DlqTrainer.step.

Synthetic data: 2048 utterances, C = 180, lengths uniform in [161, 321], batch sizes 32 and 256, SpecAugment at the CLI's
defaults.  Per batch size one child process times whole epochs (wall clock between device synchronisations) in alternating legs
host, resident, steps-only, host, ...; steps-only runs the same steps on batches that already lie on the device, so
steps-only / resident is the share of the resident epoch that is the step itself.  A last child times the gather kernel alone
(the C ABI's timing slot 14: HIP events around the launch) and reports it against the bytes it moves.  Median with min-max over
the legs, clocks before and after.  The parent touches no GPU: every child runs under its own time limit, and the first one that
fails ends the run.  One JSON line per measurement."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_RATE = 6.29e12      # bytes/s of a float4 copy, read + written (MI355X_MICROARCH.md)
N_UTTS, C_IN, SPECAUG = 2048, 180, (30, 2, 24, 2)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # noqa: BLE001
        return [f"unavailable: {e}"]


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def make_data():
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(161, 322, (N_UTTS,), generator=g).tolist()
    feats = [torch.randn(C_IN, T, generator=g) * 3.2 - 0.07 for T in lens]
    labels = (torch.rand(N_UTTS, generator=g) < 0.25).long().numpy()
    return feats, labels


def epoch_child(bs, legs):
    from dfa_amd import train_dlqueen as TD
    from dfa_amd.dataloaders import DlqResidentSet
    from dfa_amd.dlqueen_model import DeepfakeDetector
    from dfa_amd.training import DlqTrainer
    dev = torch.device("cuda", 0)
    feats, labels = make_data()
    t0 = time.perf_counter()
    rset = DlqResidentSet(feats, labels, device=dev)
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    torch.manual_seed(0)
    tr = DlqTrainer(DeepfakeDetector(C_IN, dropout=0.3).to(dev), lr=1e-6, weight_decay=1e-4, pos_weight=3.0, grad_clip=5.0, ema_decay=0.999)
    order = TD.sample_order(labels, torch.Generator().manual_seed(2))
    on_device = [(x.clone(), ln, y.clone()) for x, ln, y in TD.resident_epoch_batches(rset, order, bs, SPECAUG, random.Random(3))]

    def host():
        return TD.train_epoch(tr, TD.epoch_batches(feats, labels, order, bs, SPECAUG, random.Random(3)), dev)

    def resident():
        return TD.train_epoch(tr, TD.resident_epoch_batches(rset, order, bs, SPECAUG, random.Random(3)), dev)

    def steps_only():
        return TD.train_epoch(tr, on_device, dev)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                 # (train_epoch ends with a host read of the mean loss)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fns = {"host_loop": host, "resident_loop": resident, "steps_only": steps_only}
    for fn in (resident, steps_only):        # warm-up: workspaces, weight images, the batch buffer
        fn()
    times = {k: [] for k in fns}
    for _ in range(legs):
        for k, fn in fns.items():
            times[k].append(leg(fn))
    nsteps = len(on_device)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"what": "epoch", "utterances": N_UTTS, "batch_size": bs, "steps_per_epoch": nsteps, "legs": legs,
                      "resident_bytes": rset.bytes_resident, "upload_ms": round(upload_ms, 1),
                      "epoch_ms": {k: summary(v) for k, v in times.items()},
                      "per_step_ms": {k: round(v / nsteps, 4) for k, v in med.items()},
                      "host_over_resident": round(med["host_loop"] / med["resident_loop"], 2),
                      "step_share_of_resident_epoch": round(med["steps_only"] / med["resident_loop"], 3)}), flush=True)


def gather_child(reps):
    from dfa_amd import _lib
    from dfa_amd import train_dlqueen as TD
    from dfa_amd.dataloaders import DlqResidentSet
    dev = torch.device("cuda", 0)
    feats, labels = make_data()
    rset = DlqResidentSet(feats, labels, device=dev)
    ctx = _lib.Context.get(dev)
    r = random.Random(5)
    for bs in (32, 256):
        for masked in (False, True):
            batches = []
            for _ in range(reps):
                idx = [r.randrange(N_UTTS) for _ in range(bs)]
                spans = np.stack([TD.draw_spans(r, C_IN, int(rset.lengths[i]), *SPECAUG) for i in idx]) if masked else None
                batches.append((idx, spans))
            for idx, spans in batches[:3]:
                rset.batch(idx, spans, 2)
            torch.cuda.synchronize()
            ctx.timing(1 << 14)
            ctx.timing_reset()
            moved = 0
            t0 = time.perf_counter()
            for idx, spans in batches:
                x, ln, _ = rset.batch(idx, spans, 2)
                t_pad = -(-int(ln.max()) // 4) * 4
                moved += 4 * C_IN * (bs * t_pad + int(((ln.astype(np.int64) + 3) // 4 * 4).sum()))     # written + read (at most)
            torch.cuda.synchronize()
            wall_ms = (time.perf_counter() - t0) * 1e3 / reps
            ms, n = ctx.timing_read(14)
            ctx.timing(False)
            assert n == reps
            rate = moved / (ms * 1e-3)
            print(json.dumps({"what": "gather", "batch_size": bs, "specaug": masked, "calls": reps, "kernel_us": round(ms / n * 1e3, 2),
                              "call_wall_us_back_to_back": round(wall_ms * 1e3, 2), "mbytes_per_call": round(moved / reps / 1e6, 2),
                              "tbytes_per_s": round(rate / 1e12, 3), "share_of_hbm_copy_rate": round(rate / HBM_COPY_RATE, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--child", choices=["epoch", "gather"])
    ap.add_argument("--batch_size", type=int, default=32)
    args = ap.parse_args()
    if args.child == "epoch":
        return epoch_child(args.batch_size, args.legs)
    if args.child == "gather":
        return gather_child(args.reps)
    print("clocks before:", clocks(), flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    jobs = [me + ["--child", "epoch", "--batch_size", str(bs), "--legs", str(args.legs)] for bs in args.batches]
    jobs.append(me + ["--child", "gather", "--reps", str(args.reps)])
    for cmd in jobs:                         # a fresh process each, under its own limit; nothing more starts after a failure
        rc = subprocess.run(["timeout", "-k", "10", str(args.limit)] + cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"child {' '.join(cmd[2:])} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    print("clocks after:", clocks(), flush=True)


if __name__ == "__main__":
    main()
