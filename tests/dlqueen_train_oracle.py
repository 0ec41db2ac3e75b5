"""float64 torch-autograd statement of the DeepfakeDetector TRAINING step on a padded batch -- TEST INFRASTRUCTURE ONLY.

Written from the step's definition, not from any implementation.  Inputs x[B, C, T_max], lengths, labels
y in {0, 1}, pos_weight, the dropout probability p and the four keep masks (what a Philox draw, or all ones for p = 0, kept):
  1. encoder, DENSE over all T_max frames: x at t >= len_b counts as zero (a select: it may hold NaN); per layer
     z = Conv1d(h) (k5 pad 2, then twice k3 pad 1), BatchNorm1d on the batch statistics of ALL N = B T_max frames, padding included
     (biased variance, eps 1e-5), a = GELU(gamma zhat + beta) (erf form), h = keep a / (1 - p); running statistics move with
     momentum 0.1 and the unbiased variance N / (N - 1);
  2. StatsPool on h3 over t < len_b: mean, biased two-pass variance, std = sqrt(max(var, 1e-6)), z = [mean | std];
  3. head Linear(512 -> 256) -> GELU -> dropout -> Linear(256 -> 1);
  4. loss = mean_b -[pw y log sigmoid(l) + (1 - y) log sigmoid(-l)];
  5. backward by autograd: the 16 gradients in parameters() order."""
import numpy as np
import torch
import torch.nn.functional as F

from dlqueen_oracle import CONVS, _gelu, _t

PARAMS = [f"{m}.{k}" for conv, bn, _ in CONVS for m in (conv, bn) for k in ("weight", "bias")] + \
         ["head.0.weight", "head.0.bias", "head.3.weight", "head.3.bias"]
CASES = {          # name: (B, C, T_max, lengths)
    "A": (3, 180, 65, [65, 64, 1]),
    "B": (2, 8, 5, [5, 2]),
    "C": (5, 180, 130, [130, 129, 67, 33, 3]),
    "D": (1, 180, 2, [2]),
}
POS_WEIGHT = 2.5
CASE_SEED = {"A": 20, "B": 325, "C": 21, "D": 20}     # chosen so that no pooled variance lies within (0, 1e-5] (test_dlqueen_train_cpu.py)


def make_state_dict(model_cls, C, seed=1234):
    """seeded default initialisation with BatchNorm gamma / beta drawn away from 1 / 0 and running statistics away from 0 / 1"""
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in model_cls(C).state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for _, bn, _ in CONVS:
        n = sd[bn + ".weight"].numel()
        sd[bn + ".weight"] = 0.6 + 0.8 * torch.rand(n, generator=g)
        sd[bn + ".bias"] = 0.5 + 0.4 * torch.randn(n, generator=g)
        sd[bn + ".running_mean"] = 0.2 * torch.randn(n, generator=g)
        sd[bn + ".running_var"] = 0.5 + torch.rand(n, generator=g)
    return sd


def make_case(name, garbage=float("nan")):
    """(x[B, C, T] float32 in the stored layout with `garbage` behind every utterance's end, lengths, y[B] float32)"""
    B, C, T, lengths = CASES[name]
    g = torch.Generator().manual_seed(CASE_SEED[name])
    buf = torch.zeros((B, C, -(-T // 4) * 4), dtype=torch.float32)
    buf[:, :, :T] = torch.randn((B, C, T), generator=g) * 3.2 - 0.07
    for b, n in enumerate(lengths):
        buf[b, :, n:] = garbage
    y = torch.tensor([float((b + 1) % 2) for b in range(B)], dtype=torch.float32)
    return buf[:, :, :T], list(lengths), y


def ones_masks(B, T, H=256):
    return [np.ones((B, T, H), dtype=np.uint8)] * 3 + [np.ones((B, H), dtype=np.uint8)]


def split_keep(keep, B, T, H=256):
    """the flat keep_out of dfa_dlq_forward_train -> [three [B, T, H] masks, the head's [B, H]]"""
    keep = np.asarray(keep).reshape(-1)
    n = B * T * H
    return [keep[i * n:(i + 1) * n].reshape(B, T, H) for i in range(3)] + [keep[3 * n:].reshape(B, H)]


def step(sd, x, lengths, y, pos_weight=POS_WEIGHT, p=0.0, masks=None, dtype=torch.float64, momentum=0.1):
    """-> dict of numpy arrays: logits [B], pooled [B, 2H], loss, grads (16, parameters() order), mean / var (3 x [H], batch
    statistics, biased variance), running_mean / running_var (3 x [H], after the update)."""
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    B, _, T = x.shape
    lengths = [int(v) for v in lengths]
    masks = ones_masks(B, T) if masks is None else masks
    prm = {k: _t(sd, k, dtype).clone().requires_grad_(True) for k in PARAMS}
    valid = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    h = torch.where(valid[:, None, :], x.to(dtype), torch.zeros((), dtype=dtype))
    N = B * T
    out = {"mean": [], "var": [], "running_mean": [], "running_var": []}
    for l, (conv, bn, pad) in enumerate(CONVS):
        z = F.conv1d(h, prm[conv + ".weight"], prm[conv + ".bias"], padding=pad)
        mean = z.sum(dim=(0, 2)) / N
        var = ((z - mean[None, :, None]) ** 2).sum(dim=(0, 2)) / N
        zh = (z - mean[None, :, None]) / torch.sqrt(var + 1e-5)[None, :, None]
        a = _gelu(prm[bn + ".weight"][None, :, None] * zh + prm[bn + ".bias"][None, :, None])
        keep = torch.as_tensor(np.asarray(masks[l])).to(dtype).permute(0, 2, 1)          # [B, T, H] -> [B, H, T]
        h = keep * a / (1.0 - p)
        out["mean"].append(mean.detach().numpy())
        out["var"].append(var.detach().numpy())
        out["running_mean"].append(((1 - momentum) * _t(sd, bn + ".running_mean", dtype) + momentum * mean.detach()).numpy())
        out["running_var"].append(((1 - momentum) * _t(sd, bn + ".running_var", dtype) + momentum * var.detach() * N / (N - 1)).numpy())
    pooled, pool_var = [], []
    for b, n in enumerate(lengths):
        hv = h[b, :, :n]
        m = hv.sum(dim=1) / n
        v = ((hv - m[:, None]) ** 2).sum(dim=1) / n
        pooled.append(torch.cat([m, torch.sqrt(v.clamp(min=1e-6))]))
        pool_var.append(v.detach().numpy())
    zp = torch.stack(pooled)
    u = _gelu(zp @ prm["head.0.weight"].T + prm["head.0.bias"])
    u = torch.as_tensor(np.asarray(masks[3])).to(dtype) * u / (1.0 - p)
    logits = (u @ prm["head.3.weight"].T + prm["head.3.bias"])[:, 0]
    yy = torch.as_tensor(np.asarray(y)).to(dtype)
    loss = -(pos_weight * yy * F.logsigmoid(logits) + (1 - yy) * F.logsigmoid(-logits)).mean()
    grads = torch.autograd.grad(loss, [prm[k] for k in PARAMS])
    out.update(logits=logits.detach().numpy(), pooled=zp.detach().numpy(), pool_var=np.stack(pool_var), loss=loss.detach().numpy(),
               grads=[g.numpy() for g in grads])
    return out
