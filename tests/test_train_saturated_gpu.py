"""The tight fp32 gradient check of the CNN2D and CNN1D training steps at the real shapes: ReLU-saturated states
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
