"""CPU side of the DeepfakeDetector training step: the float64 oracle (tests/dlqueen_train_oracle.py) is pinned to what the reference
itself computed (tests/golden/dlqueen_train.npz, written by tests/golden/make_golden_dlqueen_train.py), the padding-frame claims of
the step's definition hold in it, the test cases stay off the pool's clamp, and the host logic of the trainer and the CLI."""
import math
import os
import random

import numpy as np
import pytest
import torch

import dlqueen_oracle as DO
import dlqueen_train_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LARGE = ("enc.net.0.weight", "enc.net.4.weight", "enc.net.8.weight", "head.0.weight")
BNS = ("enc.net.1", "enc.net.5", "enc.net.9")


def _cls():
    from dfa_amd.dlqueen_model import DeepfakeDetector
    return DeepfakeDetector


def _step(name, dtype=torch.float64, T=None, garbage=float("nan")):
    B, C, Tc, lengths = O.CASES[name]
    x, lengths, y = O.make_case(name, garbage=garbage)
    if T is not None and T != Tc:               # the same utterances padded to T frames
        wide = torch.full((B, C, T), garbage, dtype=torch.float32)
        wide[:, :, :Tc] = x
        x = wide
    return O.step(O.make_state_dict(_cls(), C), x, lengths, y, dtype=dtype)


def _close(got, want, what, tol=1e-10):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    assert float(np.abs(got - want).max()) <= tol * scale, (what, float(np.abs(got - want).max()) / scale)


def test_oracle_equals_the_reference_on_case_a():
    g = np.load(os.path.join(HERE, "golden", "dlqueen_train.npz"))
    got = _step("A")
    _close(got["logits"], g["logits"], "logits")
    _close(got["loss"], g["loss"], "loss")
    for l, bn in enumerate(BNS):
        _close(got["running_mean"][l], g[f"state.{bn}.running_mean"], bn + ".running_mean")
        _close(got["running_var"][l], g[f"state.{bn}.running_var"], bn + ".running_var")
    for k, grad in zip(O.PARAMS, got["grads"]):
        if k in LARGE:
            s, a = DO.exact_sums(grad.reshape(-1).tolist())
            scale = float(g["gabssum." + k])
            assert abs(s - float(g["gsum." + k])) <= 1e-10 * scale and abs(a - scale) <= 1e-10 * scale, k
            # elementwise: relative to the tensor's scale, which the sampled elements bound from below
            assert float(np.abs(grad.reshape(-1)[::997] - g["g997." + k]).max()) <= 1e-10 * float(np.abs(grad).max()), k
        elif k.endswith("bias") and k.startswith("enc.net") and k.split(".")[2] in ("0", "4", "8"):
            # true gradient zero: both sides hold rounding noise of the weight gradient's scale
            wmax = float(np.abs(got["grads"][O.PARAMS.index(k.replace("bias", "weight"))]).max())
            assert float(np.abs(grad - g["grad." + k]).max()) <= 1e-10 * wmax, k
        else:
            _close(grad, g["grad." + k], k)


def test_padding_frames_take_part_in_the_step_but_their_contents_do_not():
    a = _step("A")
    wider = _step("A", T=66)                     # one more padding frame per utterance: BatchNorm counts it
    assert any(float(np.abs(g1 - g0).max()) > 1e-6 * float(np.abs(g0).max()) for g0, g1 in zip(a["grads"], wider["grads"]))
    assert float(np.abs(a["var"][0] - wider["var"][0]).max()) > 0
    other = _step("A", garbage=1e30)             # what lies behind len_b is never used
    for k, g0, g1 in zip(O.PARAMS, a["grads"], other["grads"]):
        assert np.array_equal(g0, g1), k
    assert np.array_equal(a["logits"], other["logits"])


@pytest.mark.parametrize("name", list(O.CASES))
def test_no_pooled_variance_lies_near_the_clamp(name):
    """exactly 0 (len = 1) or above 1e-5: fp32 and float64 cannot land on opposite sides of the clamp at 1e-6"""
    _, _, _, lengths = O.CASES[name]
    pv = _step(name)["pool_var"]
    for b, n in enumerate(lengths):
        if n == 1:
            assert (pv[b] == 0).all()
        else:
            assert float(pv[b].min()) > 1e-5, (name, b, float(pv[b].min()))


@pytest.mark.parametrize("name", list(O.CASES))
def test_float32_oracle_floors(name):
    """the per-tensor distance of the float32 run from the float64 one: the floor of the GPU test's bounds (printed)"""
    w, f = _step(name), _step(name, dtype=torch.float32)
    for k, a, b in [("logits", w["logits"], f["logits"])] + list(zip(O.PARAMS, w["grads"], f["grads"])):
        scale = max(float(np.abs(a).max()), 1e-6)
        d = np.abs(np.asarray(b, dtype=np.float64) - a)
        l2 = math.sqrt(float((d * d).sum()) / max(float((np.asarray(a) ** 2).sum()), 1e-30))
        print(f"[dlq train floor {name}] {k}: max/scale {float(d.max()) / scale:.2e} l2 {l2:.2e}")
        assert np.isfinite(b).all(), k


def test_trainer_refuses_a_cpu_model_and_symbols_are_declared():
    from dfa_amd import _lib
    from dfa_amd import training
    with pytest.raises(RuntimeError, match="GPU"):
        training.DlqTrainer(_cls()(8))
    names = {s[0] for s in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    for sym in ("dfa_dlq_train_workspace_bytes", "dfa_dlq_forward_train", "dfa_dlq_backward", "dfa_bce_pos_weight_fwd_bwd", "dfa_clip_grad_norm"):
        assert sym in names and sym + "(" in header, sym
    with pytest.raises(ValueError, match="DeepfakeDetector"):
        training.DlqTrainer(torch.nn.Linear(2, 2))


def test_eval_module_still_refuses_training_and_points_at_the_trainer(capsys):
    from dfa_amd import dlqueen_model as M
    with pytest.raises(NotImplementedError, match="DlqTrainer"):
        M.DeepfakeDetector(8).train()(torch.zeros(1, 8, 4), [4])
    with pytest.raises(SystemExit):
        M.parse_args(["--epochs", "1"])
    assert "dfa_amd.train_dlqueen" in capsys.readouterr().err


def test_train_cli_arguments(capsys):
    from dfa_amd import train_dlqueen as TD
    a = TD.parse_args([])
    assert (a.data_dir, a.train_split, a.dev_split, a.ckpt_path) == ("data", "train", "dev", "best_model.pth")
    assert (a.epochs, a.batch_size, a.lr, a.weight_decay, a.grad_clip, a.hidden, a.dropout, a.seed) == (30, 32, 1e-3, 1e-4, 5.0, 256, 0.3, 42)
    assert (a.specaug, a.time_mask_max, a.time_mask_n, a.freq_mask_max, a.freq_mask_n) == (False, 30, 2, 24, 2)
    assert (a.ema, a.ema_decay, a.patience) == (False, 0.999, 6)
    a = TD.parse_args(["--ema", "--specaug", "--epochs", "2", "--ema_decay", "0.9"])
    assert a.ema and a.specaug and a.epochs == 2 and a.ema_decay == 0.9
    for bad in (["--hidden", "128"], ["--epochs", "0"], ["--dropout", "1.0"]):
        with pytest.raises(SystemExit):
            TD.parse_args(bad)
    assert "hidden=256" in capsys.readouterr().err


def test_sampler_specaugment_and_batch_order_on_stub_data():
    from dfa_amd import train_dlqueen as TD
    labels = np.array([1] * 4 + [0] * 36)
    pw, w0, w1 = TD.compute_class_weights(labels)
    assert (pw, w0, w1) == (9.0, 1 / 36, 1 / 4)
    order = TD.sample_order(labels, torch.Generator().manual_seed(3))
    assert order == TD.sample_order(labels, torch.Generator().manual_seed(3)) and len(order) == 40
    assert len(set(order)) < 40                                  # with replacement
    drawn = sum(sum(labels[i] for i in TD.sample_order(labels, torch.Generator().manual_seed(s))) for s in range(50))
    assert abs(drawn / 2000 - 0.5) < 5 * math.sqrt(0.25 / 2000)  # the classes are balanced by the weights
    feats = [np.full((8, 3 + (i * 7) % 11), float(i + 1), dtype=np.float32) for i in range(40)]
    batches = list(TD.epoch_batches(feats, labels, order, 16))
    assert [len(b[1]) for b in batches] == [16, 16, 8]
    seen = []
    for x, lengths, y in batches:
        T = int(lengths.max())
        assert x.shape == (len(lengths), 8, T) and x.stride(1) % 4 == 0 and x.dtype == torch.float32
        for j, n in enumerate(lengths):
            i = int(x[j, 0, 0].item()) - 1                       # the utterance's value names it
            seen.append(i)
            assert n == feats[i].shape[1] and float(y[j]) == labels[i]
            assert bool((x[j, :, :n] == i + 1).all()) and bool((x[j, :, n:] == 0).all())
    assert seen == order                                         # sampler order, no sorting
    # SpecAugment: per sample, on a copy, zeros in whole columns / rows only, reproducible from the generator
    cfg = (2, 2, 3, 1)
    a = list(TD.epoch_batches(feats, labels, order, 16, cfg, random.Random(5)))
    b = list(TD.epoch_batches(feats, labels, order, 16, cfg, random.Random(5)))
    assert all(torch.equal(p[0], q[0]) for p, q in zip(a, b))
    assert any(not torch.equal(p[0], q[0]) for p, q in zip(a, batches))
    assert all(float(f.min()) > 0 for f in feats)                # the data set itself is untouched
    x = TD.spec_augment(torch.ones(8, 20), random.Random(1), 5, 2, 3, 2)
    cols, rows = (x == 0).all(dim=0), (x == 0).all(dim=1)
    assert bool(((x == 0) == (cols[None, :] | rows[:, None])).all()) and int(cols.sum()) <= 10 and int(rows.sum()) <= 6

    class Stub:
        def __init__(self):
            self.calls = []

        def step(self, x, lengths, y):
            self.calls.append((tuple(x.shape), list(lengths)))
            return torch.tensor([float(len(self.calls))])
    stub = Stub()
    assert TD.train_epoch(stub, iter(batches), "cpu") == 2.0     # the mean of 1, 2, 3
    assert [c[0][0] for c in stub.calls] == [16, 16, 8]
