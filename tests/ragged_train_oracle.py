"""float64 torch-CPU statement of the CNN1D training step on a variable-length (ragged) batch -- TEST INFRASTRUCTURE ONLY.

The definition: a batch is x[B, T_max, F] with lengths[b] in [3, T_max]; utterance b is x[b, :T_b, :].
The step is what the reference model (src/model_cnn1d.py:13-46 in train mode, src/train.py:71-76) computes if BatchNorm1d sees
the utterances concatenated along time:
  * every Conv1d (k = 3, pad 1) runs per utterance, zero-padded at that utterance's own two ends;
  * each BatchNorm1d is torch's own F.batch_norm(training=True) on the concatenation [1, C, N], N = sum T_b: batch statistics
    over the valid frames only, biased variance to normalise, N / (N - 1) in the running variance;
  * ReLU; dropout 0; the time mean of utterance b over its T_b frames; Linear; BCE-with-logits on smoothed labels, mean over B.
Gradients come from autograd.  Frames t >= T_b of x are never read.
"""
import torch
import torch.nn.functional as F

from oracle import torch_ref as R

BLOCKS = (("conv.0", "conv.1"), ("conv.4", "conv.5"), ("conv.8", "conv.9"))


def cnn1d_ragged_train_step(sd, x, lengths, y, label_smoothing=0.0, return_margins=False, dtype=torch.float64):
    """sd: CNN1D state_dict (tensors or numpy); x: [B, T_max, F] (the view the trainer is fed); lengths: B ints; y: [B] 0/1.
    Returns a dict, everything float64: logits [B], loss (float), grads {parameter name: gradient},
    stats {BatchNorm prefix: (batch mean [C], biased batch variance [C], N)}; with return_margins=True also
    margins {BatchNorm prefix: smallest |BatchNorm output| of that layer}.  dtype=torch.float32 runs the same statement in fp32."""
    f64 = dtype
    lengths = [int(v) for v in lengths]
    B = x.shape[0]
    assert len(lengths) == B and all(3 <= t <= x.shape[1] for t in lengths), lengths
    P = {k: R._t(sd, k).to(f64).clone().requires_grad_(True) for k in sd
         if k.endswith(("weight", "bias")) and not k.endswith(("running_mean", "running_var"))}
    stats, margins = {}, {}
    hs = [x[b, :lengths[b], :].to(f64).transpose(0, 1).unsqueeze(0) for b in range(B)]          # [1, F, T_b] each
    for conv, bn in BLOCKS:
        zs = [F.conv1d(h, P[conv + ".weight"], P[conv + ".bias"], padding=1) for h in hs]
        zc = torch.cat(zs, dim=2)                                                               # [1, C, N]
        stats[bn] = (zc.detach().mean(dim=(0, 2)), zc.detach().var(dim=(0, 2), unbiased=False), zc.shape[2])
        yc = F.batch_norm(zc, None, None, P[bn + ".weight"], P[bn + ".bias"], training=True, momentum=0.1, eps=1e-5)
        margins[bn] = float(yc.detach().abs().min())
        a = F.relu(yc)
        hs = list(torch.split(a, lengths, dim=2))
    pooled = torch.cat([h.mean(dim=2) for h in hs], dim=0)                                      # [B, 128]
    logits = F.linear(pooled, P["classifier.weight"], P["classifier.bias"]).squeeze(-1)
    ys = y.to(f64) * (1.0 - label_smoothing) + 0.5 * label_smoothing if label_smoothing > 0 else y.to(f64)
    loss = F.binary_cross_entropy_with_logits(logits, ys)
    loss.backward()
    out = {"logits": logits.detach(), "loss": float(loss.detach()), "grads": {k: v.grad.clone() for k, v in P.items()}, "stats": stats}
    if return_margins:
        out["margins"] = margins
    return out


def state_after_step(sd, out, lr=1e-3, weight_decay=0.01, momentum=0.1):
    """The state_dict after the step's AdamW update and running-statistics update (oracle.torch_ref.state_after_adamw_step on the
    helper's gradients and statistics, in the float32 the optimiser runs in)."""
    grads = {k: v.float() for k, v in out["grads"].items()}
    stats = {k: (m.float(), v.float(), n) for k, (m, v, n) in out["stats"].items()}
    return R.state_after_adamw_step(sd, grads, stats, lr=lr, weight_decay=weight_decay, momentum=momentum)


def cnn1d_state(F_in=180, seed=5, classifier_gain=40.0):
    """A CNN1D state_dict with non-trivial BatchNorm affine parameters and a classifier that gives logits of order 1 (the weights
    tests/test_train_shapes_gpu.py::test_cnn1d_fp32_train_step_matches_oracle trains on)."""
    from dfa_amd.model_cnn1d import CNN1D
    torch.manual_seed(seed)
    m = CNN1D(in_features=F_in, dropout=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in m._BN_IDX:
            m.conv[i].weight.copy_(0.5 + torch.rand(m.conv[i].weight.shape, generator=g))
            m.conv[i].bias.copy_(0.1 * torch.randn(m.conv[i].bias.shape, generator=g))
        m.classifier.weight.mul_(classifier_gain)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def ragged_batch(lengths, T_max, F_in=180, seed=0, pad=0.0):
    """(stored [B, F, T_max] float32 with every frame t >= lengths[b] set to `pad`, y [B] float 0/1 with both classes present)."""
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    stored = torch.randn(B, F_in, T_max, generator=g) * 3.2 - 0.07
    y = (torch.rand(B, generator=g) > 0.5).float()
    if B > 1:
        y[0] = 1.0 - y[1]
    for b, t in enumerate(lengths):
        stored[b, :, int(t):] = pad
    return stored, y
