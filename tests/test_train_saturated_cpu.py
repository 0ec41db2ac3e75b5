"""CPU side of the ReLU-saturated training checks (tests/saturated_train_states.py, tests/test_train_saturated_gpu.py).

For every case the GPU file runs, the float64 oracle must show what the tight bound rests on: every BatchNorm output at least
0.25 from zero (so no fp32 rounding difference, 1e-6 at most, can flip a ReLU), logits inside +-4, gradients exactly zero where
a channel is wholly off and alive everywhere else.  The margin is a CONDITION of the construction: a case that misses it gets
another seed, never a lower number.

The planted-fault tests show the gap the tight comparator closes: a strip-edge column a weight gradient does not accumulate
(CNN2D) and a time mean divided by T_max instead of the utterance's own length (ragged CNN1D) pass the flip-tolerant bound of
tests/test_train_shapes_gpu.py and are rejected by `close_tight`.

The auto-encoder's cases (seven BatchNorm + ReLU layers, S.CAE_SHAPES) have conditions of their own, all asserted here on the
oracle alone: every margin >= 0.25; the float32 oracle within 2e-4 of scale of the float64 one on every compared gradient (a
CONDITION that keeps the derived bound at or below 1.6e-3 of scale: a case that misses it gets another seed, never a higher
cap); every compared gradient's scale >= 1e-20 (the encoder's are 1e-10 .. 1e-6 and are compared at their true scale); exact
zeros on the off channels' slices and on the reconstruction rows 16 * (T // 16) and beyond.  Its two planted faults -- an MSE
gradient normalised by the reconstructed rows, a pool backward that writes into the dropped column -- show what the suite let
through before.
"""
import pytest
import torch
import torch.nn.functional as F

import saturated_train_states as S
from test_train_shapes_gpu import _close_up_to_relu_flips

CASES = ([("cnn2d", s) for s in S.CNN2D_SHAPES] + [("cnn1d", s) for s in S.CNN1D_SHAPES] + [("ragged", n) for n in S.RAGGED_SETS]
         + [("ragged", "planted-fault")])


def _case(kind, arg):
    if arg == "planted-fault":
        return S.fault_case()
    return S.ragged_case(arg) if kind == "ragged" else (S.cnn2d_case if kind == "cnn2d" else S.cnn1d_case)(*arg)


@pytest.mark.parametrize("kind,arg", CASES, ids=[f"{k}-{a}" for k, a in CASES])
def test_saturated_case_has_its_margin_and_its_zero_slices(kind, arg):
    case = _case(kind, arg)
    w = case.want
    print(f"[saturated {kind} {arg}] margins " + " / ".join(f"{v:.3f}" for v in w["margins"].values())
          + f", max |logit| {float(w['logits'].abs().max()):.3f}")
    assert len(w["margins"]) == 3
    for bn, margin in w["margins"].items():
        assert margin >= S.MARGIN, (bn, margin)
    assert float(w["logits"].abs().max()) <= S.LOGIT_MAX
    assert 0.0 < float(case.y.mean()) < 1.0                              # both labels
    if case.lengths is not None:                                         # the padding is NaN and was never read
        assert torch.isnan(case.stored).any() or all(t == case.stored.shape[2] for t in case.lengths)
    masks = S.zero_slices(case.kind, case.sd)
    assert set(masks) == set(w["grads"]) - set(S.NOISE[case.kind]) - {"classifier.bias"}
    S.check_zero_slices(case.kind, case.sd, w["grads"].items())
    for name, g in w["grads"].items():
        assert torch.isfinite(g).all(), name
        if name in S.NOISE[case.kind]:                                   # a bias in front of a batch-statistics BatchNorm
            assert float(g.abs().max()) < 1e-9, name
            continue
        live = g[~masks[name]] if name in masks else g
        assert live.numel() > 0 and float(live.abs().max()) > 0.0, name
        if name in masks:                                                # a quarter (rows) to 7/16 (rows and columns) is off
            assert 0.2 < float(masks[name].float().mean()) < 0.5, name


@pytest.mark.parametrize("B,T,F", S.CAE_SHAPES)
def test_saturated_cae_case_meets_the_conditions_of_the_tight_bound(B, T, F):
    case = S.cae_case(B, T, F)
    w, f32 = case.want, S.fp32_step(case)
    noise = S.NOISE["cae"]
    rows = [S.tight_deviation(f32["grads"][n], g, f32["grads"][n], n, S.CAE_CLAMP) for n, g in w["grads"].items() if n not in noise]
    scales = {n: float(g.abs().max()) for n, g in w["grads"].items()}
    worst, small = max(rows, key=lambda r: r[3]), min((n for n in scales if n not in noise), key=scales.get)
    print(f"[saturated cae [{B},{T},{F}]] margins " + " / ".join(f"{v:.3f}" for v in w["margins"].values())
          + f"; largest float32 floor {worst[0]} {worst[3]:.2e} of scale, {max(r[4] for r in rows):.2e} in L2; smallest scale {small} "
          f"{scales[small]:.2e}; loss {w['loss']:.6f}")
    assert list(w["margins"]) == [bn for _, bn in S.BLOCKS["cae"]] and len(w["grads"]) == 30
    for bn, margin in w["margins"].items():
        assert margin >= S.MARGIN, (bn, margin)
    for name, _, _, fmax, _, bmax, _ in rows:
        assert fmax <= S.FLOOR_CAP, (name, fmax)
        assert bmax <= 8 * S.FLOOR_CAP
    masks = S.zero_slices("cae", case.sd)
    assert set(masks) == set(w["grads"]) - set(noise) - {"decoder.9.bias"}
    S.check_zero_slices("cae", case.sd, w["grads"].items())
    for name, g in w["grads"].items():
        assert torch.isfinite(g).all(), name
        if name in noise:                                                # a bias in front of a batch-statistics BatchNorm
            assert scales[name] < 1e-9 * scales[name.replace("bias", "weight")], name
            continue
        assert scales[name] >= S.SCALE_MIN, (name, scales[name])
        live = g[~masks[name]] if name in masks else g
        assert live.numel() > 0 and float(live.abs().max()) > 0.0, name
        if name in masks:
            assert 0.2 < float(masks[name].float().mean()) < 0.5, name
    assert w["recon"].shape == (B, T, F) and w["latent"].shape == (B, 256, T // 16, F // 16)
    assert bool((w["recon"][:, 16 * (T // 16):] == 0).all())           # the zero-padded tail (none when T is a multiple of 16)
    assert bool((w["recon"][:, :16 * (T // 16)] != 0).any())
    off = torch.tensor([S.is_off(c) for c in range(256)])
    assert bool((w["latent"][:, off] == 0).all()) and bool((w["latent"][:, ~off] > S.MARGIN).all())
    for bn, (mean, var, n) in w["stats"].items():
        assert mean.dtype == var.dtype == torch.float32 and n > 1 and bool((var > 0).all()), bn
    assert [n for _, (_, _, n) in w["stats"].items()][:2] == [B * T * F, B * (T // 2) * (F // 2)]


def test_tight_comparator_applies_the_stated_rule():
    want = torch.ones(100)
    want[0] = -2.0                                                        # scale 2, norm 10.15
    one = torch.zeros(100)
    one[1] = 1.0
    S.close_tight(want + 3.9e-4 * one, want, want, "x")                  # 1.95e-4 of the scale
    with pytest.raises(AssertionError, match="max/scale"):
        S.close_tight(want + 4.1e-4 * one, want, want, "x")              # 2.05e-4
    with pytest.raises(AssertionError, match="relative L2"):             # every element 1.75e-4 of the scale, 3.4e-4 in L2
        S.close_tight(want + 3.5e-4, want, want, "x")
    floor = want + 2e-4 * one                                            # floor 1e-4 of the scale -> bound 8e-4; L2 floor 2e-5
    S.close_tight(want + 1.5e-3 * one, want, floor, "x")
    with pytest.raises(AssertionError, match="max/scale"):
        S.close_tight(want + 1.7e-3 * one, want, floor, "x")
    tiny = 1e-9 * want                                                   # scale 2e-9: below the default clamp, seen at clamp 0
    assert S._dev(tiny + 1e-10 * one, tiny)[0] == pytest.approx(1e-4)    # 5 % of the true scale is 1e-4 of the clamped one
    assert S._dev(tiny + 1e-10 * one, tiny, 0.0)[0] == pytest.approx(0.05)
    with pytest.raises(AssertionError, match="max/scale"):
        S.close_tight(tiny + 4.1e-13 * one, tiny, tiny, "x", clamp=0.0)  # 2.05e-4 of the true one
    S.close_tight(tiny + 3.9e-13 * one, tiny, tiny, "x", clamp=0.0)


# ------------------------------------------------------------------------------------------------ planted faults
def _grads_with_fault(monkeypatch, case, fn_name, nth, fault):
    """The case's float64 oracle gradients with `fault` applied to the gradient of the nth result of torch.nn.functional.<fn_name>
    (an autograd hook on that tensor; the forward is untouched)."""
    real, calls = getattr(F, fn_name), [0]

    def hooked(*a, **k):
        out = real(*a, **k)
        calls[0] += 1
        if calls[0] == nth:
            out.register_hook(fault)
        return out
    with monkeypatch.context() as mp:
        mp.setattr(F, fn_name, hooked)
        out = S.oracle_step(case.kind, case.sd, case.stored, case.y, case.lengths)
    assert calls[0] >= nth
    assert torch.equal(out["logits"], case.want["logits"])
    return out["grads"]


def _old_accepts_new_rejects(case, faulty, tag):
    clean, fp32 = case.want["grads"], S.fp32_grads(case)
    old, rejected = [], []
    for name, want in clean.items():
        if name in S.NOISE[case.kind]:         # both comparators hold these biases to one and the same rounding-noise bound
            continue
        _close_up_to_relu_flips(faulty[name], want, name, log=old)              # the flip-tolerant bound lets the fault through
        try:
            S.close_tight(faulty[name], want, fp32[name], name)
        except AssertionError:
            rejected.append(name)
    worst = max(old, key=lambda r: r[1])
    print(f"[planted fault {tag}] largest deviation {worst[0]}: max {worst[1]:.2e} of scale, l2 {worst[2]:.2e}; "
          f"rejected by the tight comparator: {rejected}")
    assert rejected, tag
    return rejected


def test_planted_strip_edge_fault_passes_the_loose_bound_and_fails_the_tight_one(monkeypatch):
    """CNN2D [2,321,180]: block 3's weight-gradient and data-gradient passes do not see dz3 at feature column 30 (the first column
    of the second 30-column strip) of utterance 0, row 0, output channels 0 and 1.  The whole column (80 rows, 128 channels)
    moves conv.6.bias by 1e-1 in relative L2 -- in a saturated state that gradient is a residue of cancelling sums -- which the
    flip-tolerant bound rejects as well; one row of two channels lands between the two bounds (measured: 2.1e-3 of the scale,
    1.3e-3 in L2 at worst)."""
    case = S.cnn2d_case(2, 321, 180)

    def fault(g):
        assert g.shape == (2, 128, 80, 180)
        g = g.clone()
        g[0, :2, :1, 30] = 0.0
        return g
    faulty = _grads_with_fault(monkeypatch, case, "conv2d", 3, fault)
    rejected = _old_accepts_new_rejects(case, faulty, "cnn2d strip edge")
    assert "conv.10.weight" in rejected


def test_planted_time_mean_fault_passes_the_loose_bound_and_fails_the_tight_one(monkeypatch):
    """Ragged CNN1D, lengths 372, 384, 384, 384: the backward of the time mean divides the shortest utterance's gradient by
    T_max = 384 instead of by its own 372 frames, a factor 0.969.  (At the length sets of the GPU tests the factor is 64 / 324 or
    3 / 40 and every gradient is off by its whole size, which any bound rejects; 3 % of one utterance in four lands between the
    two bounds.)"""
    lengths, T_max = S.FAULT_SET
    case = S.fault_case()                 # (margin, logits and zero slices: one of CASES above)

    def fault(g):
        assert g.shape == (1, 128, sum(lengths))
        g = g.clone()
        g[:, :, :lengths[0]] *= lengths[0] / T_max
        return g
    faulty = _grads_with_fault(monkeypatch, case, "relu", 3, fault)
    _old_accepts_new_rejects(case, faulty, "ragged time mean")


# ------------------------------------------------------------------------------------------------ auto-encoder
BF16_BOUND = {"encoder": 0.10, "decoder": 0.03}     # tests/test_train_gpu.py::test_cae_bf16_training_gradients_track_the_reference


def _cae_fault_fails_the_tight_comparator(monkeypatch, fn_name, nth, fault, tag):
    """The [2,321,180] case's float64 oracle with `fault` applied to the gradient of the nth result of torch.nn.functional.<fn_name>:
    the forward (loss, reconstruction) is untouched and `check_grads_tight` at the true scale rejects the gradients.  Returns
    (the tensors that miss their bound, {tensor: max deviation / scale})."""
    case = S.cae_case(2, 321, 180)
    real, calls = getattr(F, fn_name), [0]

    def hooked(*a, **k):
        out = real(*a, **k)
        calls[0] += 1
        if calls[0] == nth:
            out.register_hook(fault)
        return out
    with monkeypatch.context() as mp:
        mp.setattr(F, fn_name, hooked)
        out = S.oracle_step("cae", case.sd, case.stored, None)
    assert calls[0] >= nth and out["loss"] == case.want["loss"] and torch.equal(out["recon"], case.want["recon"])
    noise, fp32 = S.NOISE["cae"], S.fp32_grads(case)
    rows = [S.tight_deviation(out["grads"][n], g, fp32[n], n, S.CAE_CLAMP) for n, g in case.want["grads"].items() if n not in noise]
    rejected = [r[0] for r in rows if r[1] > r[5] or r[2] > r[6]]
    worst = max(rows, key=lambda r: r[1])
    print(f"[planted fault {tag}] largest deviation {worst[0]}: max {worst[1]:.2e} of scale, l2 {worst[2]:.2e}; "
          f"rejected by the tight comparator: {rejected}")
    with pytest.raises(AssertionError):
        S.check_grads_tight(case, out["grads"].items(), clamp=S.CAE_CLAMP)
    S.check_grads_tight(case, case.want["grads"].items(), clamp=S.CAE_CLAMP)       # (the unfaulted result passes)
    return rejected, {r[0]: r[1] for r in rows}


def test_planted_cae_mse_normaliser_fault_fails_the_tight_comparator(monkeypatch):
    """Auto-encoder [2,321,180]: the decoder rebuilds 320 rows and row 320 of the reconstruction is zero padding.  The fault
    normalises the MSE gradient by the reconstructed elements, B * 320 * F, instead of nn.MSELoss's B * 321 * F: every gradient is
    321 / 320 of what it should be, 0.31 % of its scale.  What let it through: at T = 32, the only shape whose fp32 gradients the
    suite compared with an independent reference (tests/golden/cae_train.npz), the two counts are equal; at T = 321 the bf16-mode
    test allows 10 % (encoder) and 3 % (decoder) of scale, and the kernel-against-twin tests share the normaliser."""
    def fault(g):
        assert g.shape == (2, 1, 320, 180)
        return g * (321.0 / 320.0)
    rejected, dev = _cae_fault_fails_the_tight_comparator(monkeypatch, "conv_transpose2d", 4, fault, "cae MSE normaliser")
    assert len(rejected) == 23                      # every gradient but the seven noise biases
    for name, emax in dev.items():                  # ... and every one of them inside the bf16-mode bound of its half
        assert emax < BF16_BOUND[name.split(".")[0]] / 9, (name, emax)


def test_planted_cae_pool_backward_fault_fails_the_tight_comparator(monkeypatch):
    """Auto-encoder [2,321,180]: encoder block 3's 2x2 floor pool takes 80 x 45 to 40 x 22 and drops column 44, whose gradient is
    zero.  The fault gives the dropped column its neighbour's gradient (column 43's).  What let such a fault through: the suite's
    only fp32 comparison with an independent reference, T = 32, has this pool on an 8-row map -- a kernel that goes wrong on the
    edge column only in a later row tile of the 80-row map is not seen there -- and at T = 321 there were the twin tests, which
    share the pool backward, and the bf16-mode bounds of 10 % (20 % for block 1) of an encoder gradient's scale.  In this state
    the fault is not subtle (measured: encoder.5.bias, a residue of cancelling sums, moves by 98 % of its scale,
    encoder.0.weight by 20 %, encoder.8.weight by 7 %); it touches nothing downstream of the pool in the backward order, so the
    decoder and encoder block 4 must stay clean."""
    def fault(g):
        assert g.shape == (2, 128, 80, 45)
        g = g.clone()
        g[..., 44] = g[..., 43]
        return g
    rejected, dev = _cae_fault_fails_the_tight_comparator(monkeypatch, "relu", 3, fault, "cae pool backward")
    assert rejected == [n for n in dev if n.startswith(("encoder.0", "encoder.1.", "encoder.4", "encoder.5", "encoder.8", "encoder.9"))]
    assert all(dev[n] == 0.0 for n in dev if n.startswith(("decoder", "encoder.12", "encoder.13")))
