"""float64 torch-CPU statement of the DeepfakeDetector eval forward on a padded variable-length batch -- TEST INFRASTRUCTURE ONLY.

Written from the model's definition, not from any implementation:
  x[B, C, T] float, time fastest, utterance b owns frames t < len_b; frames t >= len_b count as zero whatever they hold;
  1. Conv1d(C -> H, k = 5, pad 2) -> BatchNorm1d (running statistics, eps 1e-5) -> exact GELU (erf form)
  2. Conv1d(H -> H, k = 3, pad 1) -> BatchNorm1d -> GELU           3. the same again
     -- over ALL T frames of the padded row: the encoder is not masked, so frames past len_b hold GELU(BN(.)) != 0 after
     layer 1 and the next layer reads them; past T the convolution's own zero padding applies;
  4. pool over t < len_b: mean, biased variance, std = sqrt(max(var, 1e-6)), z = [mean | std]
  5. Linear(2H -> H) -> GELU -> Linear(H -> 1).
Hence logit_b = f(x[b, :, :len_b], len_b, min(T - len_b, 2))."""
import math

import numpy as np
import torch
import torch.nn.functional as F

LENGTHS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 130, 321]     # the fixture's utterances (tests/golden/dlqueen_eval.npz)
INIT_SEED = 1234                                                 # torch.manual_seed before the model is built
CONVS = (("enc.net.0", "enc.net.1", 2), ("enc.net.4", "enc.net.5", 1), ("enc.net.8", "enc.net.9", 1))


def _t(sd, key, dtype):
    v = sd[key]
    return (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(dtype)


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


def forward(sd, x, lengths, dtype=torch.float64):
    """sd: DeepfakeDetector state_dict (tensors or numpy); x: [B, C, T]; lengths: B ints in [1, T].
    -> (logits [B], pooled [B, 2H]) as numpy arrays of `dtype`."""
    x = (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)))
    B, _, T = x.shape
    lengths = [int(v) for v in lengths]
    assert len(lengths) == B and all(1 <= n <= T for n in lengths), lengths
    valid = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]                     # [B, T]
    h = torch.where(valid[:, None, :], x.to(dtype), torch.zeros((), dtype=dtype))
    for conv, bn, pad in CONVS:
        h = F.conv1d(h, _t(sd, conv + ".weight", dtype), _t(sd, conv + ".bias", dtype), padding=pad)
        scale = _t(sd, bn + ".weight", dtype) / torch.sqrt(_t(sd, bn + ".running_var", dtype) + 1e-5)
        h = (h - _t(sd, bn + ".running_mean", dtype)[None, :, None]) * scale[None, :, None] + _t(sd, bn + ".bias", dtype)[None, :, None]
        h = _gelu(h)
    pooled = []
    for b, n in enumerate(lengths):
        hv = h[b, :, :n]
        mean = hv.sum(dim=1) / n
        var = ((hv - mean[:, None]) ** 2).sum(dim=1) / n
        pooled.append(torch.cat([mean, torch.sqrt(var.clamp(min=1e-6))]))
    z = torch.stack(pooled)
    g = _gelu(z @ _t(sd, "head.0.weight", dtype).T + _t(sd, "head.0.bias", dtype))
    logits = (g @ _t(sd, "head.3.weight", dtype).T + _t(sd, "head.3.bias", dtype))[:, 0]
    return logits.numpy(), z.numpy()


def pad_batch(utts, T=None, fill=0.0):
    """list of [C, T_i] arrays -> ([B, C, T] float32 batch, rows rounded up to 4 frames in memory but sliced to T; lengths)"""
    lengths = [int(u.shape[-1]) for u in utts]
    T = max(lengths) if T is None else T
    buf = torch.full((len(utts), utts[0].shape[0], -(-T // 4) * 4), float(fill), dtype=torch.float32)
    for i, u in enumerate(utts):
        buf[i, :, :lengths[i]] = torch.as_tensor(np.asarray(u), dtype=torch.float32)
    return buf[:, :, :T], lengths


def split_utts(g):
    """the fixture's utterances: x_cat [C, sum LENGTHS] cut at LENGTHS"""
    cuts = np.cumsum([0] + LENGTHS)
    return [g["x_cat"][:, cuts[i]:cuts[i + 1]] for i in range(len(LENGTHS))]


def exact_sums(values):
    """(sum, sum of magnitudes), exactly rounded: independent of summation order and thread count"""
    return math.fsum(values), math.fsum(abs(v) for v in values)


def fixture_state_dict(g, model_cls):
    """The fixture's state dict.  The file holds the tensors that were drawn or scaled after construction (BatchNorm, head.3)
    in full; the large ones (convolutions, head.0: 3 MB) are the seeded default initialisation, rebuilt here with `model_cls`
    under INIT_SEED and checked against the sums and leading values the reference's own tensors had."""
    torch.manual_seed(INIT_SEED)
    sd = {k: v.detach().clone() for k, v in model_cls(180).state_dict().items()}
    for k in sd:
        if "full." + k in g:
            sd[k] = torch.from_numpy(np.asarray(g["full." + k]))
        else:
            v = sd[k].double().reshape(-1).tolist()
            np.testing.assert_array_equal(sd[k].reshape(-1)[:32].numpy(), g["head32." + k], err_msg=k)
            assert exact_sums(v) == (float(g["sum." + k]), float(g["abssum." + k])), k
    return sd
