"""ReLU-saturated training states and the tight fp32 gradient comparator -- TEST INFRASTRUCTURE ONLY.

Both classifiers use ReLU behind a batch-statistics BatchNorm and average pools, so ReLU is their only discrete decision.  The
states built here keep every BatchNorm output far from zero: gamma uniform in [0.05, 0.15], beta = +3, and beta = -3 on every
fourth channel (c % 4 == 3).  A normalised value would have to lie 20 standard deviations out to reach zero, so three channels
in four are wholly on, one in four is wholly off, and no rounding difference between two implementations can move an element
across its ReLU.  The training step is then a smooth function of its inputs which fp32 and float64 arithmetic agree on to about
1e-5, and its gradients can be held to the [4,16,180] fixture's 2e-4 at the real frame count, where the flip-tolerant bounds of
tests/test_train_shapes_gpu.py are 3e-2 / 3e-3.  The data path is the ordinary one: same convolutions, BatchNorm kernels, pool
rows, dropped frame, strips and reductions.

The auto-encoder (kind "cae") has seven BatchNorm + ReLU layers -- four convolution blocks with 2x2 floor pools, three
ConvTranspose2d blocks -- and takes the same recipe; its input is randn of standard deviation 1 (it sees z-scored features) and
its cases need no classifier shrink.  Its encoder gradients are tiny in these states (max |grad| 1e-10 .. 1e-6 against
1e-2 .. 1e+3 in the decoder: every BatchNorm layer between the loss and them scales the gradient by its gamma / sigma) but as
well conditioned as the rest -- the float32 oracle's distance from the float64 one is 1e-5 .. 1e-4 of their scale -- so they are
compared at their TRUE scale: the comparator's scale clamp, 1e-6 for the classifiers, is a parameter and 0 for the auto-encoder.

A case is computed once per process and shared; nothing in it is modified afterwards.
"""
import math
from collections import namedtuple

import numpy as np
import torch

import ragged_train_oracle as RO
from oracle import torch_ref as R
from test_cnn1d_ragged_train_gpu import SETS as RAGGED_SETS      # the four length sets of the ragged step's own tests

EPS = 0.05                      # label smoothing of every case
MARGIN = 0.25                   # every BatchNorm output of every case is at least this far from zero (asserted on the CPU)
LOGIT_MAX = 4.0                 # every oracle logit stays inside +-LOGIT_MAX: sigmoid is not saturated
_LOGIT_AIM = 3.5                # what the classifier is scaled to when the default one exceeds it
ABS_TOL, L2_TOL, FLOOR_FACTOR = 2e-4, 1e-4, 8.0

BLOCKS = {"cnn2d": (("conv.0", "conv.1"), ("conv.5", "conv.6"), ("conv.10", "conv.11")),
          "cnn1d": (("conv.0", "conv.1"), ("conv.4", "conv.5"), ("conv.8", "conv.9")),
          "cae": (("encoder.0", "encoder.1"), ("encoder.4", "encoder.5"), ("encoder.8", "encoder.9"), ("encoder.12", "encoder.13"),
                  ("decoder.0", "decoder.1"), ("decoder.3", "decoder.4"), ("decoder.6", "decoder.7"))}
NOISE = {kind: tuple(conv + ".bias" for conv, _ in blocks) for kind, blocks in BLOCKS.items()}

# the cases of tests/test_train_saturated_gpu.py; tests/test_train_saturated_cpu.py checks the margin of every one
CNN2D_SHAPES = [(2, 321, 180), (3, 322, 180), (2, 323, 180), (3, 21, 65), (2, 33, 5)]
CNN1D_SHAPES = [(3, 321, 180), (2, 37, 180), (2, 384, 180)]
# T = 321, 322, 335: one dropped row and one zero tail row, an odd 161 -> 80, 15 zero tail rows; T = 47, 31: odd at every level;
# T = 17: latent height 1; F = 20: the narrowest F = 16k + 4.  [B,16,20], the smallest shape the ABI takes, is left out: its latent
# map is 1x1 and the float32 oracle itself lies 5e-3 .. 6e-3 of scale from the float64 one whatever B is.
CAE_SHAPES = [(2, 321, 180), (3, 322, 180), (2, 335, 180), (3, 47, 36), (4, 31, 52), (8, 17, 36), (6, 33, 20)]
CAE_CLAMP = 0.0                 # the auto-encoder's gradients are compared at their true scale max |want|
FLOOR_CAP = 2e-4                # a case whose float32 floor exceeds this is not used (the derived bound stays <= 1.6e-3 of scale)
SCALE_MIN = 1e-20               # every compared auto-encoder gradient is normal in fp32 with room below it
FAULT_SET = ([372, 384, 384, 384], 384)     # the ragged case of the planted time-mean fault (tests/test_train_saturated_cpu.py)

# want: the float64 oracle's logits (classifiers) or recon and latent (auto-encoder), loss, grads, stats, margins
Case = namedtuple("Case", "kind sd stored y lengths want")


def is_off(c):
    return c % 4 == 3


def _model(kind, F):
    if kind == "cnn2d":
        from dfa_amd.model import CNN2D
        return CNN2D(in_features=F, dropout=0.0)
    if kind == "cae":
        from dfa_amd.model_cae import ConvAutoencoder
        return ConvAutoencoder()
    from dfa_amd.model_cnn1d import CNN1D
    return CNN1D(in_features=F, dropout=0.0)


def _batchnorms(kind, m):
    if kind == "cae":
        return [m.encoder[b] for _, b in m._ENC] + [m.decoder[b] for _, b in m._DEC if b is not None]
    return [m.conv[i] for i in m._BN_IDX]


def saturated_state(kind, F, seed):
    """state_dict of a default-initialised CNN2D / CNN1D / ConvAutoencoder with the saturating BatchNorm affine parameters (a
    classifier is still the default one: `oracle_step` users go through `make_case`, which scales it for its batch)."""
    torch.manual_seed(seed)
    m = _model(kind, F)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in _batchnorms(kind, m):
            bn.weight.copy_(0.05 + 0.1 * torch.rand(bn.weight.shape, generator=g))
            bn.bias.fill_(3.0)
            bn.bias[[c for c in range(bn.bias.numel()) if is_off(c)]] = -3.0
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def batch(B, T, F, seed, lengths=None, pad=float("nan")):
    """stored [B, F, T] = randn * 3.2 - 0.07 (fed as the strided [B, T, F] view), y with both labels; frames past an utterance's
    length hold `pad`."""
    g = torch.Generator().manual_seed(seed)
    stored = torch.randn(B, F, T, generator=g) * 3.2 - 0.07
    y = (torch.arange(B) % 2 == int(torch.randint(0, 2, (1,), generator=g))).float()
    for b, t in enumerate(lengths or ()):
        stored[b, :, int(t):] = pad
    return stored, y


def cae_batch(B, T, F, seed):
    """stored [B, F, T] = randn (the auto-encoder sees z-scored features); fed as the contiguous [B, T, F] copy, or as the strided
    view by the one test that is about it."""
    return torch.randn(B, F, T, generator=torch.Generator().manual_seed(seed))


def oracle_step(kind, sd, stored, y, lengths=None, dtype=torch.float64):
    """The oracle of `kind` on the [B, T, F] view of `stored`, as one dict of float32/float64 CPU tensors whatever the oracle."""
    x = stored.transpose(1, 2)
    if lengths is not None:
        out = RO.cnn1d_ragged_train_step(sd, x, lengths, y, EPS, return_margins=True, dtype=dtype)
        return {"logits": out["logits"].double(), "loss": out["loss"], "grads": {k: v.double() for k, v in out["grads"].items()},
                "stats": {k: (m.float(), v.float(), n) for k, (m, v, n) in out["stats"].items()}, "margins": out["margins"]}
    if kind == "cae":
        loss, grads, recon, latent, stats, margins = R.cae_train_step_emulated(sd, x, emulate=None, dtype=dtype, return_stats=True,
                                                                               return_margins=True)
        return {"recon": recon.double(), "latent": latent.double(), "loss": loss, "grads": {k: v.double() for k, v in grads.items()},
                "stats": stats, "margins": margins}
    if kind == "cnn2d":
        logits, loss, grads, stats, margins = R.cnn2d_train_step_emulated(sd, x, y, EPS, emulate=None, return_stats=True,
                                                                          return_margins=True, dtype=dtype)
    else:
        logits, loss, grads, stats, margins = R.cnn1d_train_step(sd, x, y, EPS, return_stats=True, return_margins=True, dtype=dtype)
    return {"logits": logits.double(), "loss": loss, "grads": {k: v.double() for k, v in grads.items()}, "stats": stats,
            "margins": margins}


_cases, _floors = {}, {}


def make_case(kind, B, T, F, seed, lengths=None):
    """The saturated state, batch and float64 oracle result of one case.  The logits are linear in the classifier, so one fp32
    run of the oracle with the default classifier tells by how much weight and bias have to shrink for |logit| <= 3.5.  (The
    auto-encoder has no classifier and no labels: its case is the state and the batch as they are.)"""
    key = (kind, B, T, F, seed, None if lengths is None else tuple(lengths))
    if key not in _cases:
        sd = saturated_state(kind, F, seed)
        if kind == "cae":
            stored, y = cae_batch(B, T, F, seed + 1000), None
        else:
            stored, y = batch(B, T, F, seed + 1000, lengths)
            top = float(oracle_step(kind, sd, stored, y, lengths, torch.float32)["logits"].abs().max())
            shrink = min(1.0, _LOGIT_AIM / top)
            sd["classifier.weight"] = sd["classifier.weight"] * shrink
            sd["classifier.bias"] = sd["classifier.bias"] * shrink
        _cases[key] = Case(kind, sd, stored, y, lengths, oracle_step(kind, sd, stored, y, lengths))
    return _cases[key]


def cnn2d_case(B, T, F):
    return make_case("cnn2d", B, T, F, seed=200 + T + F)


def cnn1d_case(B, T, F):
    return make_case("cnn1d", B, T, F, seed=5 + T)


def cae_case(B, T, F):
    return make_case("cae", B, T, F, seed=400 + T + F)


def ragged_case(name):
    lengths, T_max = RAGGED_SETS[name]
    return make_case("cnn1d", len(lengths), T_max, 180, seed=5 + T_max, lengths=lengths)


def fault_case():
    lengths, T_max = FAULT_SET
    return make_case("cnn1d", len(lengths), T_max, 180, seed=77, lengths=lengths)


def fp32_step(case):
    """The float32 run of the same oracle on the same state and batch: its distance from the float64 one is the noise floor of
    fp32 arithmetic on this case."""
    if id(case) not in _floors:
        _floors[id(case)] = (case, oracle_step(case.kind, case.sd, case.stored, case.y, case.lengths, torch.float32))
    return _floors[id(case)][1]


def fp32_grads(case):
    return fp32_step(case)["grads"]


def state_after(case):
    w = case.want
    return R.state_after_adamw_step(case.sd, {k: v.float() for k, v in w["grads"].items()}, w["stats"])


# ------------------------------------------------------------------------------------------------ which slices must vanish
def zero_slices(kind, sd):
    """{parameter name: boolean mask of the elements whose gradient is exactly zero because a channel is wholly off}: gamma, beta
    and the convolution-weight rows of an off channel, the next layer's weight columns for an off input channel, the
    classifier's columns of the off block-3 channels.  (The convolution biases vanish everywhere: NOISE.)  The auto-encoder's
    ConvTranspose2d weights are [C_in, C_out, 2, 2]: output channels on dim 1, input channels on dim 0 -- decoder.0's inputs
    are the latent channels, and the last layer, decoder.9, has the off channels of decoder.7 as inputs."""
    masks = {}
    blocks = BLOCKS[kind]
    for i, (conv, bn) in enumerate(blocks):
        w = sd[conv + ".weight"]
        out_dim = 1 if conv.startswith("decoder") else 0
        off = torch.tensor([is_off(c) for c in range(w.shape[out_dim])])
        m = torch.zeros(w.shape, dtype=torch.bool).transpose(0, out_dim)        # [output channels, input channels, ...] view
        m[off] = True
        if i > 0:
            m[:, torch.tensor([is_off(c) for c in range(m.shape[1])])] = True
        masks[conv + ".weight"] = m.transpose(0, out_dim)
        masks[bn + ".weight"] = masks[bn + ".bias"] = off
    if kind == "cae":
        masks["decoder.9.weight"] = torch.zeros(sd["decoder.9.weight"].shape, dtype=torch.bool)
        masks["decoder.9.weight"][off] = True
        return masks
    cw = sd["classifier.weight"]
    per = cw.shape[1] // off.numel()                    # CNN2D: F columns per block-3 channel (emb is [128, F] flattened); CNN1D: 1
    masks["classifier.weight"] = off.repeat_interleave(per)[None, :].expand(cw.shape).clone()
    return masks


def check_zero_slices(kind, sd, named_grads):
    masks = zero_slices(kind, sd)
    for name, g in named_grads:
        if name in masks:
            bad = g.detach().cpu()[masks[name]]
            assert bool((bad == 0).all()), (name, "off-channel gradient not exactly zero", float(bad.abs().max()))


# ------------------------------------------------------------------------------------------------ the tight comparator
def _dev(got, want, clamp=1e-6):
    """(max |got - want| / scale, relative L2 distance) in float64; scale = max(max |want|, clamp)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(np.abs(want).max(), clamp, 1e-300)
    d = np.abs(got - want)
    return float(d.max() / scale), float(math.sqrt((d * d).sum() / max((want * want).sum(), 1e-30)))


def _np(v):
    return v.detach().double().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


def tight_deviation(got, want, fp32, name, clamp=1e-6):
    """(name, max/scale, relative L2, the float32 oracle's max/scale and relative L2, the two bounds that follow from them)."""
    fmax, fl2 = _dev(_np(fp32), _np(want), clamp)
    emax, el2 = _dev(_np(got), _np(want), clamp)
    return (name, emax, el2, fmax, fl2, max(ABS_TOL, FLOOR_FACTOR * fmax), max(L2_TOL, FLOOR_FACTOR * fl2))


def _assert_row(row):
    name, emax, el2, fmax, fl2, bmax, bl2 = row
    assert emax <= bmax, (name, "max/scale", emax, "floor", fmax, "bound", bmax)
    assert el2 <= bl2, (name, "relative L2", el2, "floor", fl2, "bound", bl2)


def close_tight(got, want, fp32, name, log=None, clamp=1e-6):
    """Every element of `got` within max(2e-4, 8 * floor_max) of the tensor's scale and the tensor within max(1e-4, 8 * floor_L2)
    in relative L2 of the float64 result `want`, where floor_* is how far the float32 run `fp32` of the same oracle lies from it.
    2e-4 is the [4,16,180] fixture's bound; the factor 8 covers another summation order and longer serial chains than
    torch's CPU kernels have.  The floor is the reference arithmetic's own error, never the implementation's under test.
    clamp: the smallest scale a tensor is measured against (1e-6 for the classifiers, 0 -- the true scale -- for the auto-encoder)."""
    row = tight_deviation(got, want, fp32, name, clamp)
    if log is not None:
        log.append(row)
    _assert_row(row)


def check_grads_tight(case, named_grads, log=None, clamp=1e-6):
    """All of a step's gradients against the case's float64 oracle: the biases in front of a BatchNorm at the rounding-noise bound
    tests/test_train_shapes_gpu.py gives them, every other tensor at `close_tight`'s bounds, no element left out.  Every tensor is
    measured (and logged) before the first one that misses its bound raises.  The noise bound is 1e-4 of the weight gradient's
    scale plus the clamp; at clamp 0 that absolute term becomes 1e-6 of the weight gradient's scale, so it never exceeds it."""
    want, fp32 = case.want["grads"], fp32_grads(case)
    named_grads = list(named_grads)
    assert {n for n, _ in named_grads} == set(want)
    rows = [tight_deviation(got, want[n], fp32[n], n, clamp) for n, got in named_grads if n not in NOISE[case.kind]]
    if log is not None:
        log.extend(rows)
    for name, got in named_grads:
        if name in NOISE[case.kind]:
            wmax = float(want[name.replace("bias", "weight")].abs().max())
            floor = 1e-4 * wmax + (clamp if clamp > 0 else 1e-6 * wmax)
            assert float(got.abs().max()) < floor, (name, float(got.abs().max()), floor)
    for row in rows:
        _assert_row(row)


def print_tight_log(tag, log):
    """One line per case: the tensor closest to its bound (worst ratio), then the worst floor."""
    if not log:
        return
    w = max(log, key=lambda r: max(r[1] / r[5], r[2] / r[6]))
    f = max(log, key=lambda r: r[3])
    print(f"[{tag}] worst {w[0]}: max {w[1]:.2e} (floor {w[3]:.2e}, bound {w[5]:.2e}), l2 {w[2]:.2e} (floor {w[4]:.2e}, "
          f"bound {w[6]:.2e}); largest floor {f[0]} {f[3]:.2e}")
