"""Cost of the k = (5, 3, 3) CNN1D eval forward beside the three-tap forward, at the real shape: B = 256
utterances of 180 features x 321 frames, float32, the stored [B][F][T] layout (one launch per forward).  Legs, each a fresh
child process (a process binds one build of the library), run in alternating rounds:
  k3_parent   CNN1D() on the library named by --parent-lib (a build of the parent commit under lib/); left out without it
  k3          CNN1D() on this tree's library
  k3_as_parent  (with --parent-lib) this tree's library driven exactly as the parent's is -- named by file, symbol table filtered,
              dfa_cnn1d_set_kernels never called: separates what the library costs from what the leg's host path costs
  k5_parent   (with --parent-lib) CNN1D(kernels=(5, 3, 3)) on the parent's library
  k5          CNN1D(kernels=(5, 3, 3)) on this tree's library
A child walks `--buffers` distinct inputs in turn (8 x 59 MB: more than the 256 MB Infinity Cache, so every forward reads x from
HBM), warms up, then times `--reps` groups of `--iters` forwards between device events and reports the median group.  Prints one
JSON line: per leg the per-round medians, their median / min / max (the run-to-run spread the comparison has to be read
against), k3 over k3_parent, k5 over k5_parent and k5 over k3 (MAC ratio per frame: 59,520 / 48,000 = 1.24).
--what train times the all-native training step instead (NativeTrainer.step on one resident batch, dropout 0.2, label smoothing
0.05, lr 1e-6 so that every leg stays in one activation regime; 5 groups of 20 steps per child), the same legs.
usage: timeout -k 10 600 python tools/gpu_cnn1d_k5_bench.py [--what forward|train] [--parent-lib libdfa_hip_parent.so] [--rounds 4]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, F, T = 256, 180, 321


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from dfa_amd import _lib
    if args.lib:
        import ctypes
        _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), args.lib)
        probe = ctypes.CDLL(_lib.LIB_PATH)
        _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]   # an older build lacks the newer entry points
    from dfa_amd.model_cnn1d import CNN1D
    torch.manual_seed(0)
    k5 = args.leg.startswith("k5")       # (a parent that has the variant has dfa_cnn1d_set_kernels: its k5 leg is driven as this tree's)
    if k5:
        model = CNN1D(kernels=(5, 3, 3))
    else:
        model = CNN1D()
        if args.lib:                   # the parent's library has no dfa_cnn1d_set_kernels: bind as the parent's Python did
            model._ensure_prepared = lambda ctx: _lib.ensure_prepared(model, ctx, "cnn1d", "dfa_cnn1d_set_params",
                                                                      (model.in_features, model.base_channels), "dfa_cnn1d_prepare")
    g = torch.Generator().manual_seed(1)
    base = torch.randn(B, F, T, generator=g) * 3.2 - 0.07
    if args.what == "train":
        from dfa_amd.training import train_step
        if args.lib and not k5:        # the parent's library has no dfa_cnn1d_set_kernels: its _bind did not call it
            class _NoKernels:
                def __init__(self, lib):
                    self._lib = lib

                def __getattr__(self, name):
                    return (lambda *a: 0) if name == "dfa_cnn1d_set_kernels" else getattr(self._lib, name)
            ctx = _lib.Context.get(torch.device("cuda", 0))
            ctx.lib = _NoKernels(ctx.lib)
        model.dropout = 0.2
        tr = train_step.NativeTrainer(model.to("cuda"), label_smoothing=0.05, lr=1e-6)
        x = base.to("cuda").transpose(1, 2)
        y = (torch.rand(B, generator=g) > 0.5).float().to("cuda")
        for _ in range(5):
            last = tr.step(x, y)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(20):
                last = tr.step(x, y)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1) / 20)
        print(json.dumps({"leg": args.leg, "ms": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)),
                          "checksum": float(last)}))
        return
    model = model.to("cuda").eval()
    xs = [base.to("cuda").transpose(1, 2) for _ in range(args.buffers)]
    with torch.no_grad():
        for x in xs:
            out = model(x)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(args.iters):
                out = model(xs[i % len(xs)])
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1) / args.iters)
    print(json.dumps({"leg": args.leg, "ms": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)),
                      "checksum": float(out.double().sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="file name under dfa_amd's lib/: a build of the parent commit")
    ap.add_argument("--what", default="forward", choices=["forward", "train"])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process")
    ap.add_argument("--lib", default=None, help="(internal) the leg's library")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    legs = ([("k3_parent", args.parent_lib), ("k3_as_parent", "libdfa_hip.so")] if args.parent_lib else []) + [("k3", None)]
    legs += ([("k5_parent", args.parent_lib)] if args.parent_lib else []) + [("k5", None)]
    res = {name: [] for name, _ in legs}
    sums = {}
    for _ in range(args.rounds):
        for name, lib in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--what", args.what, "--reps", str(args.reps), "--iters", str(args.iters),
                   "--buffers", str(args.buffers)] + (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
            if p.returncode != 0:            # a leg that failed ends the run: nothing more is started on the GPU
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"leg {name} exited with {p.returncode}")
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[name].append(r["ms"])
            sums[name] = r["checksum"]
    import numpy as np
    out = {"what": args.what, "B": B, "F": F, "T": T, "rounds": args.rounds, "reps": args.reps, "iters": args.iters, "buffers": args.buffers}
    for name, v in res.items():
        out[name] = {"round_ms": v, "median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "checksum": sums[name]}
    if "k3_parent" in out:
        out["k3_over_k3_parent"] = out["k3"]["median"] / out["k3_parent"]["median"]
        out["k3_checksum_equals_parent"] = out["k3"]["checksum"] == out["k3_parent"]["checksum"]
        out["k3_as_parent_over_k3_parent"] = out["k3_as_parent"]["median"] / out["k3_parent"]["median"]
        out["k5_over_k5_parent"] = out["k5"]["median"] / out["k5_parent"]["median"]
        out["k5_checksum_equals_parent"] = out["k5"]["checksum"] == out["k5_parent"]["checksum"]
    out["k5_over_k3"] = out["k5"]["median"] / out["k3"]["median"]
    out["mac_ratio"] = 59520 / 48000
    print(json.dumps(out))


if __name__ == "__main__":
    main()
