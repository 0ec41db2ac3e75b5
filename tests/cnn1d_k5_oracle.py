"""Float64 statement of the CNN1D with per-layer kernel sizes -- the reference's CNN1D_Variant (src/compare_kernels.py:38-67):
three blocks Conv1d(k, padding k // 2) -> BatchNorm1d -> ReLU (dropout 0 / eval), the mean over time, a linear head.  Written
with torch's functional ops on float64 tensors: F.conv1d, F.batch_norm, mean, F.linear -- no module of either project.

    forward(sd, x)            eval logits [B, 1] of x [B, T, F] (running statistics)
    forward_ragged(sd, utts)  each utterance [F, T_i] alone on its own frames -> [N, 1]
    train_step(sd, x, y)      train-mode (batch statistics, dropout 0) BCE-with-logits loss and the 14 gradients by float64 autograd

tests/golden/make_golden_cnn1d_k533.py checks it against the reference's own float32 module before it writes the fixtures;
tests/test_cnn1d_k5.py repeats that check on the committed fixtures."""
import numpy as np
import torch
import torch.nn.functional as F

CONV_IDX, BN_IDX = (0, 4, 8), (1, 5, 9)
EPS = 1e-5
GRAD_KEYS = tuple(f"conv.{i}.{n}" for c, b in zip(CONV_IDX, BN_IDX) for i, n in ((c, "weight"), (c, "bias"), (b, "weight"), (b, "bias"))) \
    + ("classifier.weight", "classifier.bias")


def _t(v):
    return torch.as_tensor(np.asarray(v), dtype=torch.float64)


def kernels_of(sd):
    return tuple(int(np.asarray(sd[f"conv.{c}.weight"]).shape[2]) for c in CONV_IDX)


def _run(p, x, training):
    """p: float64 tensors by state_dict key; x [B, T, F] float64 -> logits [B, 1]"""
    h = x.transpose(1, 2)
    for c, b in zip(CONV_IDX, BN_IDX):
        w = p[f"conv.{c}.weight"]
        h = F.conv1d(h, w, p[f"conv.{c}.bias"], padding=w.shape[2] // 2)
        h = F.batch_norm(h, None if training else p[f"conv.{b}.running_mean"], None if training else p[f"conv.{b}.running_var"],
                         p[f"conv.{b}.weight"], p[f"conv.{b}.bias"], training=training, eps=EPS)
        h = torch.relu(h)
    return F.linear(h.mean(dim=2), p["classifier.weight"], p["classifier.bias"])


def forward(sd, x):
    p = {k: _t(v) for k, v in sd.items() if "num_batches" not in k}
    with torch.no_grad():
        return _run(p, _t(x), False).numpy()


def forward_ragged(sd, utts):
    """utts: per-utterance [F, T_i] arrays; every utterance is scored alone, on its own frames"""
    return np.concatenate([forward(sd, np.asarray(u, dtype=np.float64).T[None]) for u in utts], axis=0)


def train_step(sd, x, y):
    """-> (logits [B, 1], loss, {key: gradient}) of mean BCE-with-logits, train mode, dropout 0; all float64 numpy"""
    p = {k: _t(v) for k, v in sd.items() if "num_batches" not in k}
    for k in GRAD_KEYS:
        p[k] = p[k].clone().requires_grad_(True)
    logits = _run(p, _t(x), True)
    loss = F.binary_cross_entropy_with_logits(logits.squeeze(-1), _t(y))
    loss.backward()
    return logits.detach().numpy(), float(loss.detach()), {k: p[k].grad.numpy() for k in GRAD_KEYS}


def asymmetric_state(in_features=180, kernels=(5, 3, 3), seed=0):
    """A state dict (float32 numpy, the reference's keys and shapes) whose weights differ from tap to tap -- tap k of every
    filter is scaled in proportion to (1 + 0.35 k) -- so a reversed or shifted tap order cannot pass; non-trivial running
    statistics.  The scales keep every layer's pre-activations of order one for inputs of the stored features' scale (std 3.2:
    layer 1 divides by it) and the logits at a few units, the range of the reference fixtures' logits -- the range the absolute
    1e-4 bar of the three-tap tests is stated for."""
    g = np.random.default_rng(seed)
    chans = [(in_features, 32), (32, 64), (64, 128)]
    sd = {}
    for li, ((cin, cout), k, c, b) in enumerate(zip(chans, kernels, CONV_IDX, BN_IDX)):
        tap = 1.0 + 0.35 * np.arange(k)
        w = g.standard_normal((cout, cin, k)) / np.sqrt(cin * k) * (tap / np.sqrt((tap ** 2).mean()))
        sd[f"conv.{c}.weight"] = (w / (3.2 if li == 0 else 1.0)).astype(np.float32)
        sd[f"conv.{c}.bias"] = (0.1 * g.standard_normal(cout)).astype(np.float32)
        sd[f"conv.{b}.weight"] = (0.5 + g.random(cout)).astype(np.float32)
        sd[f"conv.{b}.bias"] = (0.1 * g.standard_normal(cout)).astype(np.float32)
        sd[f"conv.{b}.running_mean"] = (0.2 * g.standard_normal(cout)).astype(np.float32)
        sd[f"conv.{b}.running_var"] = (0.5 + g.random(cout)).astype(np.float32)
        sd[f"conv.{b}.num_batches_tracked"] = np.asarray(7, dtype=np.int64)
    sd["classifier.weight"] = (0.3 * g.standard_normal((1, 128))).astype(np.float32)
    sd["classifier.bias"] = (0.1 * g.standard_normal(1)).astype(np.float32)
    return sd


def utterances(lengths, seed, F_=180):
    """per-utterance [F, T_i] float32 arrays at the scale of the stored features"""
    g = np.random.default_rng(seed)
    return [(g.standard_normal((F_, int(T))) * 3.2 - 0.07).astype(np.float32) for T in lengths]
