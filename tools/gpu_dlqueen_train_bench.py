"""DeepfakeDetector training step on the MI355X: DlqTrainer.step (forward_train, BCE(pos_weight), backward, clip, fused AdamW, EMA;
dropout 0.3) against a torch-ROCm fp32 eager step of the same model (the test oracle's statement: unmasked encoder, masked pool,
BCEWithLogitsLoss(pos_weight), clip_grad_norm_, AdamW, EMA) on the same GPU, at [32, 180, 321] (the reference's batch size) and
[256, 180, 321], lengths in [161, 321].

Legs alternate (native, eager, native, ...), each leg times `--steps` steps between device synchronisations after a warm-up; the
result is the median with min-max over the legs.  Per-kernel-group times come from the C ABI's timing slots in a run of their own
(slot 8 weight images, 9 forward convolutions, 10 statistics / activation passes / pool + head, 11 backward elementwise passes,
12 data gradients, 13 weight gradients).  The share of the bf16 matrix rate is the 6x issued MFMA FLOPs of the convolutions, data
gradients and weight gradients over the time of slots 9 + 12 + 13 and the dense bf16 peak.  Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BF16 = 2.5168e15        # dense bf16 matrix rate, FLOP/s (MI355X_MICROARCH.md)


class Eager(torch.nn.Module):
    """the reference model's definition in plain torch (fp32, no autocast)"""

    def __init__(self, C, p):
        super().__init__()
        nn = torch.nn
        self.enc = nn.Sequential(nn.Conv1d(C, 256, 5, padding=2), nn.BatchNorm1d(256), nn.GELU(), nn.Dropout(p),
                                 nn.Conv1d(256, 256, 3, padding=1), nn.BatchNorm1d(256), nn.GELU(), nn.Dropout(p),
                                 nn.Conv1d(256, 256, 3, padding=1), nn.BatchNorm1d(256), nn.GELU(), nn.Dropout(p))
        self.head = nn.Sequential(nn.Linear(512, 256), nn.GELU(), nn.Dropout(p), nn.Linear(256, 1))

    def forward(self, x, lengths):
        h = self.enc(x)
        mask = (torch.arange(h.shape[-1], device=h.device)[None, :] < lengths[:, None]).unsqueeze(1).to(h.dtype)
        n = lengths[:, None].to(h.dtype)
        mean = (h * mask).sum(-1) / n
        var = (((h - mean.unsqueeze(-1)) ** 2) * mask).sum(-1) / n
        return self.head(torch.cat([mean, torch.sqrt(var.clamp(min=1e-6))], dim=1)).squeeze(-1)


def clocks():
    try:
        import subprocess
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # noqa: BLE001
        return [f"unavailable: {e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    args = ap.parse_args()
    from dfa_amd import _lib
    from dfa_amd.dlqueen_model import DeepfakeDetector
    from dfa_amd.training import DlqTrainer
    dev = torch.device("cuda", 0)
    print("clocks before:", clocks(), flush=True)
    for B in args.batches:
        C, T = 180, 321
        g = torch.Generator().manual_seed(1)
        x = (torch.randn((B, C, 324), generator=g) * 3.2 - 0.07)[:, :, :T]
        lengths = torch.randint(161, 322, (B,), generator=g)
        lengths[0] = T
        for b in range(B):
            x[b, :, int(lengths[b]):] = 0.0
        y = (torch.rand(B, generator=g) > 0.5).float()
        x, y = x.to(dev), y.to(dev)
        lens_host, lens_dev = lengths.numpy(), lengths.to(dev)
        torch.manual_seed(0)
        tr = DlqTrainer(DeepfakeDetector(C, dropout=0.3).to(dev), lr=1e-6, weight_decay=1e-4, pos_weight=2.5, grad_clip=5.0, ema_decay=0.999)
        eager = Eager(C, 0.3).to(dev).train()
        opt = torch.optim.AdamW(eager.parameters(), lr=1e-6, weight_decay=1e-4)
        crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.5], device=dev))
        shadow = [p.detach().clone() for p in eager.parameters()]
        xe = x.contiguous()

        def native():
            return tr.step(x, lens_host, y)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            loss = crit(eager(xe, lens_dev), y)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(eager.parameters(), 5.0)
            opt.step()
            torch._foreach_lerp_(shadow, [p.detach() for p in eager.parameters()], 1e-3)
            return loss

        def leg(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

        for fn in (native, torch_step):
            for _ in range(args.warmup):
                fn()
        times = {"native": [], "eager": []}
        for _ in range(args.legs):
            times["native"].append(leg(native))
            times["eager"].append(leg(torch_step))
        ctx = _lib.Context.get(dev)
        ctx.timing(True)
        ctx.timing_reset()
        nslot = 4
        for _ in range(nslot):
            native()
        torch.cuda.synchronize()
        slots = {s: ctx.timing_read(s)[0] / nslot for s in (8, 9, 10, 11, 12, 13)}
        ctx.timing(False)
        N = B * T
        useful = 2.0 * N * 256 * (5 * C + 3 * 256 + 3 * 256) + 2.0 * N * 256 * 2 * 3 * 256 + 2.0 * N * 256 * (5 * C + 3 * 256 + 3 * 256)
        mfma_ms = slots[9] + slots[12] + slots[13]

        def summary(v):
            return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        print(json.dumps({"shape": [B, C, T], "steps_per_leg": args.steps, "legs": args.legs, "native_step": summary(times["native"]),
                          "eager_fp32_step": summary(times["eager"]),
                          "speedup_median": round(statistics.median(times["eager"]) / statistics.median(times["native"]), 3),
                          "slot_ms_per_step": {str(k): round(v, 4) for k, v in slots.items()},
                          "useful_gflop_per_step": round(useful / 1e9, 2), "issued_gflop_per_step": round(6 * useful / 1e9, 2),
                          "share_of_bf16_matrix_rate_issued": round(6 * useful / (mfma_ms * 1e-3) / PEAK_BF16, 4)}), flush=True)
    print("clocks after:", clocks(), flush=True)


if __name__ == "__main__":
    main()
