"""The tight fp32 gradient check of the CNN2D, CNN1D and auto-encoder training steps at the real shapes: ReLU-saturated states
(tests/saturated_train_states.py) against the float64 oracles.

tests/test_train_shapes_gpu.py and tests/test_cnn1d_ragged_train_gpu.py have to let every gradient move by 3 % of its scale and
3e-3 in relative L2 at [B,321,180], because fp32 and float64 arithmetic place about one ReLU input per block on opposite sides
of zero.  Here no input is within 0.25 of zero (asserted per case on the CPU, tests/test_train_saturated_cpu.py), so the step is
smooth and the same kernels -- six strips, the dropped frame, odd H2, the per-utterance bounds of a ragged batch -- are held to
  * max(2e-4, 8 * floor_max) of the tensor's scale on every element and max(1e-4, 8 * floor_L2) in relative L2, where floor is
    the distance of the float32 run of the same oracle on the CPU from the float64 one (never the GPU's own output),
  * exactly zero on every gradient slice of a channel that is wholly off,
  * the same bound of the same oracle result when the utterances are permuted,
fp32 mode, dropout 0, label smoothing 0.05, default context options; logits, loss, running statistics and the state after the
AdamW step at the bounds of tests/test_train_shapes_gpu.py.

THE AUTO-ENCODER (ConvAutoencoder: four convolution blocks with 2x2 floor pools, three ConvTranspose2d + BatchNorm blocks, one
of them with output_padding (0, 1), a linear last layer, the crop or zero pad back to T) takes the same construction for its
seven BatchNorm + ReLU layers.  Its fp32 gradients were compared with an independent reference at [2,32,180] only, where no pool
drops a row, the decoder rebuilds exactly T rows and the MSE normaliser B T F equals the number of reconstructed elements; here
they are held at T = 321, 322, 335 (a dropped row and a zero tail row, an odd 161 -> 80, 15 zero tail rows), 47 and 31 (odd at
every level), 17 (latent height 1) and at F = 20 (the narrowest F = 16k + 4), through the autograd bridge (model(x), nn.MSELoss,
torch.optim.AdamW) and through CaeNativeTrainer.step, fp32 precision, default context options: loss to 1e-5, the reconstruction,
the latent map and all 30 gradients at the rule above, exact zeros on the off channels' slices and on the zero-padded tail rows,
running statistics and the state after one AdamW step.  The encoder's gradients are 1e-10 .. 1e-6 in these states, so every
tensor is measured against its TRUE scale max |want| (scale clamp 0; the classifiers keep 1e-6) and the noise bound of a bias in
front of a BatchNorm is 1.01e-4 of its weight gradient's scale with no absolute term.  Conditions asserted on the CPU per case
(tests/test_train_saturated_cpu.py): margin >= 0.25, float32 floor <= 2e-4 of scale, every scale >= 1e-20.  Measured -- the
margin and the largest float32 floor on the CPU that built the cases, and on one MI355X the tensor closest to its bound with
its deviation from the float64 oracle (fraction of scale / relative L2; bridge and trainer agree to the digits shown):
    case           smallest margin   largest floor (max / L2)              GPU worst tensor, max / L2
    [2,321,180]    0.634             encoder.4.weight 7.8e-05 / 3.8e-05    encoder.5.bias    1.1e-05 / 1.1e-05
    [3,322,180]    0.356             encoder.4.weight 6.6e-05 / 7.0e-05    encoder.1.bias    1.7e-05 / 1.8e-05
    [2,335,180]    0.963             encoder.4.weight 4.0e-05 / 5.3e-05    encoder.1.bias    1.6e-05 / 1.4e-05
    [3,47,36]      2.249             encoder.4.weight 1.2e-05 / 7.7e-06    decoder.6.weight  6.0e-06 / 6.5e-06
    [4,31,52]      2.170             encoder.4.weight 3.5e-05 / 1.4e-05    decoder.6.weight  1.4e-05 / 9.7e-06
    [8,17,36]      2.288             encoder.4.weight 1.9e-05 / 1.3e-05    decoder.6.weight  4.0e-06 / 5.1e-06
    [6,33,20]      2.272             encoder.4.weight 8.2e-06 / 5.9e-06    decoder.4.bias    8.7e-06 / 8.0e-06
    [2,321,180] utterances swapped                                         encoder.1.bias    1.8e-05 / 1.4e-05
    [3,47,36] strided x                                                    decoder.6.weight  6.0e-06 / 6.5e-06
so the bound is 2e-4 / 1e-4 for every tensor of every case and the GPU uses a tenth of it; the loss agrees to 2e-7 relative.
Left out: [B,16,20], the smallest shape the ABI accepts.  Its latent map is 1x1 and the step is ill-conditioned whatever B is --
the float32 oracle itself lies 5e-3 .. 6e-3 of scale from the float64 one for B = 2, 5, 12, 16 -- so it stays with the ABI error
and shape tests.  bf16 mode is not compared here: every stored activation is 3 +- 0.1 in these states and a bf16 ulp at 3 is
0.016, so storage rounding would dominate; tests/test_train_gpu.py keeps the emulated-oracle check of that mode.

The same states put channels with mean^2 / variance of 300 .. 3000 in front of BatchNorm (every convolution input behind block 1
is 3 +- 0.1); the last test here isolates that: batch statistics of channels whose mean is a hundred standard deviations out.
"""
import numpy as np
import pytest
import torch

import ragged_train_oracle as RO
import saturated_train_states as S
from test_train_shapes_gpu import _check_state, _cnn2d, _print_log, _to_np

pytestmark = pytest.mark.gpu


def _model(case):
    F = case.stored.shape[1]
    if case.kind == "cnn2d":
        return _cnn2d(case.sd, F)
    if case.kind == "cae":
        from dfa_amd.model_cae import ConvAutoencoder
        m = ConvAutoencoder(precision="fp32")
        m.load_state_dict({k: v.clone() for k, v in case.sd.items()})
        return m.to("cuda").train()
    from dfa_amd.model_cnn1d import CNN1D
    m = CNN1D(in_features=F, dropout=0.0)
    m.load_state_dict({k: v.clone() for k, v in case.sd.items()})
    return m.to("cuda").train()


def _batch(case, perm=None):
    """(x [B, T, F] strided view on the GPU, y, lengths), the utterances in the order `perm`."""
    stored, y, lengths = case.stored, case.y, case.lengths
    if perm is not None:
        stored, y = stored[perm].contiguous(), y[perm]
        lengths = None if lengths is None else [lengths[i] for i in perm]
    return stored.to("cuda").transpose(1, 2), y.to("cuda"), lengths


def _bridge_step(case):
    """src/train.py:71-76 over the autograd bridge: torch criterion, loss.backward(), torch.optim.AdamW."""
    m = _model(case)
    x, y, _ = _batch(case)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    logits = m(x).squeeze(-1)
    loss = torch.nn.BCEWithLogitsLoss()(logits, y * (1 - S.EPS) + 0.5 * S.EPS)
    opt.zero_grad()
    loss.backward()
    got = {"logits": logits.detach().clone(), "loss": loss.detach().clone(),
           "grads": [(n, p.grad.detach().clone()) for n, p in m.named_parameters()]}
    opt.step()
    got["state"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return got


def _native_step(case, perm=None):
    """One NativeTrainer.step; the gradients are the views of the trainer's flat buffer as they stand before the update."""
    from dfa_amd.training import train_step as TS
    m = _model(case)
    x, y, lengths = _batch(case, perm)
    tr = TS.NativeTrainer(m, lr=1e-3, weight_decay=0.01, label_smoothing=S.EPS)
    got = {}
    fwd, upd = TS.forward_train_raw, tr._exchange_and_update

    def forward(*a, **k):
        outs, st = fwd(*a, **k)
        got["logits"] = outs[0].detach().clone().squeeze(-1)
        return outs, st

    def update():
        got["grads"] = [(n, g.detach().clone()) for (n, _), g in zip(m.named_parameters(), tr.grad_views)]
        upd()
    tr._exchange_and_update = update
    TS.forward_train_raw = forward
    try:
        got["loss"] = tr.step(x, y, lengths).detach().clone().squeeze()
    finally:
        TS.forward_train_raw = fwd
    got["state"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.cuda.synchronize()
    return got


def _check(case, got, tag, perm=None):
    w = case.want
    want_logits = w["logits"].numpy() if perm is None else w["logits"].numpy()[perm]
    tight, state = [], []
    print(f"[{tag}] logits max err {np.abs(_to_np(got['logits']) - want_logits).max():.2e}, loss {got['loss'].item():.8f} vs {w['loss']:.8f}")
    try:
        np.testing.assert_allclose(_to_np(got["logits"]), want_logits, atol=2e-4, rtol=1e-5)
        np.testing.assert_allclose(got["loss"].item(), w["loss"], rtol=1e-5)
        assert len(got["grads"]) == len(w["grads"])
        for _, g in got["grads"]:
            assert bool(torch.isfinite(g).all())
        S.check_grads_tight(case, [(n, g.cpu()) for n, g in got["grads"]], log=tight)
        S.check_zero_slices(case.kind, case.sd, got["grads"])
        _check_state(got["state"], S.state_after(case), case.sd, S.NOISE[case.kind], log=state)
    finally:
        S.print_tight_log(tag, tight)
        _print_log(tag + " state", state or [("-", 0.0, 0.0, 0)])


# ------------------------------------------------------------------------------------------------ CNN2D
@pytest.mark.parametrize("B,T,F", S.CNN2D_SHAPES)
def test_cnn2d_saturated_train_step_matches_oracle_tightly(B, T, F):
    case = S.cnn2d_case(B, T, F)
    _check(case, _bridge_step(case), f"saturated cnn2d [{B},{T},{F}] bridge")
    _check(case, _native_step(case), f"saturated cnn2d [{B},{T},{F}] trainer")


def test_cnn2d_saturated_gradients_do_not_depend_on_the_utterance_order():
    case = S.cnn2d_case(2, 321, 180)
    _check(case, _native_step(case, perm=[1, 0]), "saturated cnn2d [2,321,180] trainer, utterances swapped", perm=[1, 0])


# ------------------------------------------------------------------------------------------------ CNN1D, uniform
@pytest.mark.parametrize("B,T,F", S.CNN1D_SHAPES)
def test_cnn1d_saturated_train_step_matches_oracle_tightly(B, T, F):
    case = S.cnn1d_case(B, T, F)
    _check(case, _bridge_step(case), f"saturated cnn1d [{B},{T},{F}] bridge")
    _check(case, _native_step(case), f"saturated cnn1d [{B},{T},{F}] trainer")


# ------------------------------------------------------------------------------------------------ CNN1D, ragged
def _ragged(name, x3, perm=None):
    from dfa_amd import _lib
    case = S.ragged_case(name)
    assert bool(torch.isnan(case.stored).any())                    # the padding frames hold NaN
    ctx = _lib.Context.get(torch.device("cuda"))
    ctx.set_option("cnn1d_train_x3", x3)
    try:
        got = _native_step(case, perm)
    finally:
        ctx.set_option("cnn1d_train_x3", 1)
    _check(case, got, f"saturated cnn1d ragged set {name} x3={x3}" + (f" order {perm}" if perm else ""), perm)


@pytest.mark.parametrize("x3", [1, 0, 3])
@pytest.mark.parametrize("name", list(S.RAGGED_SETS))
def test_cnn1d_ragged_saturated_train_step_matches_oracle_tightly(name, x3):
    """x3: the options tests/test_cnn1d_ragged_train_gpu.py sweeps -- 1 the default, 0 the fp32 vector-ALU convolutions and the
    fp32 matrix-core weight gradient, 3 two bf16 terms per operand."""
    _ragged(name, x3)


def test_cnn1d_ragged_saturated_gradients_do_not_depend_on_the_utterance_order():
    _ragged("B", 1, perm=[2, 0, 1])


# ------------------------------------------------------------------------------------------------ auto-encoder
def _cae_x(case, perm=None, strided=False):
    """x [B, T, F] fp32 on the GPU: the contiguous copy, or the strided view of the stored [B, F, T] tensor."""
    stored = case.stored if perm is None else case.stored[perm].contiguous()
    x = stored.to("cuda").transpose(1, 2)
    return x if strided else x.contiguous()


def _cae_bridge_step(case, **kw):
    """src/train_cae.py:58-82 over the autograd bridge: model(x), nn.MSELoss, loss.backward(), torch.optim.AdamW."""
    m, x = _model(case), _cae_x(case, **kw)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    recon, latent = m(x)
    loss = torch.nn.MSELoss()(recon, x)
    opt.zero_grad()
    loss.backward()
    got = {"recon": recon.detach().clone(), "latent": latent.detach().clone(), "loss": loss.detach().clone(),
           "grads": [(n, p.grad.detach().clone()) for n, p in m.named_parameters()]}
    opt.step()
    got["state"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return got


def _cae_native_step(case, **kw):
    """One CaeNativeTrainer.step; the gradients are the views of the trainer's flat buffer as they stand before the update."""
    from dfa_amd.training.train_step import CaeNativeTrainer
    m, x = _model(case), _cae_x(case, **kw)
    tr = CaeNativeTrainer(m, lr=1e-3, weight_decay=0.01)
    got, upd = {}, tr._exchange_and_update

    def update():
        got["grads"] = [(n, g.detach().clone()) for (n, _), g in zip(m.named_parameters(), tr.grad_views)]
        upd()
    tr._exchange_and_update = update
    got["loss"] = tr.step(x).detach().clone().squeeze()
    got["state"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.cuda.synchronize()
    return got


def _check_cae(case, got, tag, perm=None):
    """loss to 1e-5; reconstruction and latent map (the bridge returns them) and all 30 gradients at the tight rule with the scale
    clamp at 0, so the encoder gradients of 1e-10 .. 1e-6 are held at their own scale; exact zeros; the state after the step."""
    w, f32 = case.want, S.fp32_step(case)
    T = case.stored.shape[2]
    tight, state = [], []
    print(f"[{tag}] loss {got['loss'].item():.8f} vs {w['loss']:.8f}")
    try:
        np.testing.assert_allclose(got["loss"].item(), w["loss"], rtol=1e-5)
        for name in ("recon", "latent"):
            if name in got:
                want, floor = (w[name], f32[name]) if perm is None else (w[name][perm], f32[name][perm])
                assert got[name].shape == want.shape
                S.close_tight(got[name], want, floor, name, log=tight, clamp=S.CAE_CLAMP)
        if "recon" in got:
            assert bool((got["recon"][:, 16 * (T // 16):] == 0).all()), "zero-padded tail rows of the reconstruction"
        assert len(got["grads"]) == len(w["grads"]) == 30
        for _, g in got["grads"]:
            assert bool(torch.isfinite(g).all())
        S.check_grads_tight(case, [(n, g.cpu()) for n, g in got["grads"]], log=tight, clamp=S.CAE_CLAMP)
        S.check_zero_slices("cae", case.sd, got["grads"])
        _check_state(got["state"], S.state_after(case), case.sd, S.NOISE["cae"], log=state)
    finally:
        S.print_tight_log(tag, tight)
        _print_log(tag + " state", state or [("-", 0.0, 0.0, 0)])


@pytest.mark.parametrize("B,T,F", S.CAE_SHAPES)
def test_cae_saturated_train_step_matches_oracle_tightly(B, T, F):
    case = S.cae_case(B, T, F)
    _check_cae(case, _cae_bridge_step(case), f"saturated cae [{B},{T},{F}] bridge")
    _check_cae(case, _cae_native_step(case), f"saturated cae [{B},{T},{F}] trainer")


def test_cae_saturated_gradients_do_not_depend_on_the_utterance_order():
    case = S.cae_case(2, 321, 180)
    _check_cae(case, _cae_bridge_step(case, perm=[1, 0]), "saturated cae [2,321,180] bridge, utterances swapped", perm=[1, 0])
    _check_cae(case, _cae_native_step(case, perm=[1, 0]), "saturated cae [2,321,180] trainer, utterances swapped", perm=[1, 0])


def test_cae_saturated_train_step_on_a_strided_view():
    """x as the [B, T, F] view of a [B, F, T] tensor (strides (F*T, 1, T)), which the forward, the fused MSE gradient and block 1's
    weight gradient all read."""
    case = S.cae_case(3, 47, 36)
    assert not _cae_x(case, strided=True).is_contiguous()
    _check_cae(case, _cae_bridge_step(case, strided=True), "saturated cae [3,47,36] bridge, strided x")
    _check_cae(case, _cae_native_step(case, strided=True), "saturated cae [3,47,36] trainer, strided x")


# ------------------------------------------------------------------------------------------------ BatchNorm statistics, large mean
@pytest.mark.parametrize("lengths", [None, [40, 23]], ids=["uniform", "ragged"])
def test_cnn1d_batch_statistics_of_channels_with_a_large_mean(lengths):
    """conv.0.bias = 200 puts every block-1 channel's mean a hundred standard deviations from zero (mean^2 / variance about 1e4).
    A variance taken as E[z^2] - mean^2 from fp32 sums then loses 1e4 x 6e-8 of itself; cm_stats_kernel (uniform) and
    cm_stats_ragged_kernel sum z minus the channel's first sample instead.  The running statistics after one step against the
    float64 statement of the step: running_mean to 1e-6, running_var to 1e-5 relative.  Where 1e-5 comes from: z is stored in
    fp32, half an ulp of 256 = 1.5e-5 on a standard deviation of 1.4, so the variance of the stored z differs from the exact one
    by at most 2 x 1.5e-5 / 1.4 = 2e-5 of itself if every rounding error lined up with the signal (1e-6 when they do not), and
    running_var = 0.9 + 0.1 x var x n / (n - 1) carries a fifth of that: 4e-6, with fp32 storage of the result 6e-8 more."""
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.training.train_step import NativeTrainer
    B, T, F = 2, 40, 180
    torch.manual_seed(31)
    m = CNN1D(in_features=F, dropout=0.0)
    with torch.no_grad():
        m.conv[0].bias.fill_(200.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    stored, y = S.batch(B, T, F, seed=32, lengths=lengths)
    want = RO.cnn1d_ragged_train_step(sd, stored.transpose(1, 2), lengths or [T] * B, y, S.EPS)
    mean, var, n = want["stats"]["conv.1"]
    assert float((mean * mean / var).min()) > 3e3                      # the case is what it claims to be
    m = m.to("cuda").train()
    NativeTrainer(m, lr=1e-3, weight_decay=0.01, label_smoothing=S.EPS).step(stored.to("cuda").transpose(1, 2), y.to("cuda"), lengths)
    rm, rv = m.conv[1].running_mean.double().cpu(), m.conv[1].running_var.double().cpu()
    rm_w, rv_w = 0.1 * mean, 0.9 + 0.1 * var * (n / (n - 1))
    e_mean, e_var = float(((rm - rm_w) / rm_w).abs().max()), float(((rv - rv_w) / rv_w).abs().max())
    print(f"[cnn1d large-mean statistics {'ragged' if lengths else 'uniform'}] mean^2/var {float((mean * mean / var).min()):.0f} .. "
          f"{float((mean * mean / var).max()):.0f}, running_mean rel err {e_mean:.2e}, running_var rel err {e_var:.2e}")
    assert e_mean <= 1e-6, e_mean
    assert e_var <= 1e-5, e_var
