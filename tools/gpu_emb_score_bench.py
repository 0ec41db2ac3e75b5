"""Cost of embedding anomaly scoring at the real shape, in one process: B = 256 utterances of [321, 180] through the bf16 CNN2D
forward (D = 23040), a PCA + GMM detector with P = 256, K = 8, and a One-Class SVM with n_sv support vectors (500 and 2000).
Alternating timed legs, device events around `iters` calls each:
  forward        the forward with return_embedding=True alone
  device         (a) forward + both detectors on the device (EmbeddingScorer.score_features), scores left on the device
  ocsvm, gmm     the scoring calls alone on a resident embedding batch: the kernels' times
  copy           (b, first half) forward + the 23.6 MB embedding batch to the host
and, on the host clock, `host_scoring`: the float32 numpy statement of both scores (tests/emb_oracle.py) on the copied batch with
the process's CPU threads -- the route a user had before the device scorer: forward, copy, score on the host.
Prints one JSON line: per leg the median / min / max ms over the pairs; the scoring kernels' FLOP (2 N D n_sv; 2 N D P +
2 K N P_pad^2) over their time, and as a fraction of the 157.3 TFLOP/s of v_mfma_f32_32x32x2_f32.
usage: timeout -k 10 500 python tools/gpu_emb_score_bench.py [--pairs 5] [--iters 10] [--n-sv 500 2000]"""
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
import emb_oracle as EO  # noqa: E402
from dfa_amd import embedding_anomaly as EA  # noqa: E402
from dfa_amd.model import CNN2D  # noqa: E402

PEAK_F32_MFMA = 157.3e12
B, T, F, P, K = 256, 321, 180, 256, 8
D = 128 * F
KEYS = ("mean", "inv_scale", "sv", "dual_coef", "gamma", "intercept", "pca_mean", "components", "means", "prec_chol", "log_const")


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--n-sv", type=int, nargs="+", default=[500, 2000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("gpu_emb_score_bench.py measures on the GPU: there is nothing to time without one")
    torch.manual_seed(0)
    model = CNN2D(in_features=F, precision="bf16").to("cuda").eval()
    x = (torch.randn(B, F, T, generator=torch.Generator().manual_seed(1)) * 3.2 - 0.07).to("cuda").to(torch.bfloat16).transpose(1, 2)
    out = {"B": B, "D": D, "P": P, "K": K, "pairs": args.pairs, "iters": args.iters, "cpu_threads": torch.get_num_threads()}
    for n_sv in args.n_sv:
        det, _ = EO.random_detectors(9, D, n_sv, P, K)
        scorer = EA.EmbeddingScorer(EA.Detectors(**{k: det[k] for k in KEYS}), "cuda")
        with torch.no_grad():
            _, emb = model(x, return_embedding=True)
        legs = {
            "forward": lambda: model(x, return_embedding=True),
            "device": lambda: scorer.score_features(model, x),
            "ocsvm": lambda: scorer.ocsvm_scores(emb),
            "gmm": lambda: scorer.gmm_scores(emb),
            "copy": lambda: model(x, return_embedding=True)[1].cpu(),
        }
        res = {k: [] for k in legs}
        with torch.no_grad():
            for _ in range(2):
                for fn in legs.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.pairs):
                for name, fn in legs.items():
                    res[name].append(timed(fn, args.iters))
        host = emb.cpu().numpy()
        EO.ocsvm_scores(det, host[:8], np.float32)
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            EO.ocsvm_scores(det, host, np.float32)
            EO.gmm_scores(det, host, np.float32)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        r = {name: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for name, v in res.items()}
        r["host_scoring"] = [float(np.median(host_ms)), float(np.min(host_ms)), float(np.max(host_ms))]
        r["parent_route_ms"] = r["copy"][0] + r["host_scoring"][0]
        flop = {"ocsvm": 2.0 * B * D * n_sv, "gmm": 2.0 * B * D * P + 2.0 * K * B * (-(-P // 32) * 32) ** 2}
        for name, f in flop.items():
            r[name + "_tflops"] = f / (r[name][0] * 1e-3) / 1e12
            r[name + "_fraction_of_f32_mfma_peak"] = f / (r[name][0] * 1e-3) / PEAK_F32_MFMA
        r["scoring_over_forward"] = (r["ocsvm"][0] + r["gmm"][0]) / r["forward"][0]
        out[f"n_sv={n_sv}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
