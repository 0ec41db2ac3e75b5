"""CPU side of the ReLU-saturated training checks (tests/saturated_train_states.py, tests/test_train_saturated_gpu.py).

For every case the GPU file runs, the float64 oracle must show what the tight bound rests on: every BatchNorm output at least
0.25 from zero (so no fp32 rounding difference, 1e-6 at most, can flip a ReLU), logits inside +-4, gradients exactly zero where
a channel is wholly off and alive everywhere else.  The margin is a CONDITION of the construction: a case that misses it gets
another seed, never a lower number.

The planted-fault tests show the gap the tight comparator closes: a strip-edge column a weight gradient does not accumulate
(CNN2D) and a time mean divided by T_max instead of the utterance's own length (ragged CNN1D) pass the flip-tolerant bound of
tests/test_train_shapes_gpu.py and are rejected by `close_tight`.
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
