"""CPU side of the CNN1D variable-length (ragged) training step: the float64 helper that states its definition
(tests/ragged_train_oracle.py) is pinned to the uniform training oracle and to the reference's own autograd results, and the
host-side pieces -- C ABI table, RaggedBatcher's shuffled epochs, the train CLI's argument check, length validation -- are
checked without a GPU."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ragged_train_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE1D = ("conv.0.bias", "conv.4.bias", "conv.8.bias")
NEW_SYMBOLS = ("dfa_cnn1d_train_ragged_workspace_bytes", "dfa_cnn1d_forward_train_ragged", "dfa_cnn1d_backward_ragged")


def _f32(v):
    return (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(v)).float().numpy()


def _uniform_cases(golden):
    _, g = golden("cnn1d_train")
    sd = {k[len("init.sd."):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("init.sd.")}
    yield "golden [4,32,180]", sd, torch.from_numpy(g["ls05.x"]).transpose(1, 2), torch.from_numpy(g["ls05.y"])
    stored, y = RO.ragged_batch([37, 37], 37, seed=3)
    yield "[2,37,180]", RO.cnn1d_state(seed=42), stored.transpose(1, 2), y


def test_helper_with_equal_lengths_is_the_uniform_oracle(golden):
    """All lengths = T: the helper (per-utterance conv1d, batch_norm on the concatenation) reproduces
    oracle.torch_ref.cnn1d_train_step -- logits, loss, every gradient, the batch statistics -- to 1e-12 (the oracle returns its
    float64 results rounded to float32, so the helper's are rounded the same way before the comparison)."""
    from oracle import torch_ref as R
    for tag, sd, x, y in _uniform_cases(golden):
        B, T, _ = x.shape
        logits_w, loss_w, grads_w, stats_w = R.cnn1d_train_step(sd, x, y, 0.05, return_stats=True)
        out = RO.cnn1d_ragged_train_step(sd, x, [T] * B, y, 0.05)
        np.testing.assert_allclose(_f32(out["logits"]), logits_w.numpy(), rtol=0, atol=1e-12, err_msg=tag)
        assert abs(out["loss"] - loss_w) <= 1e-12, (tag, out["loss"], loss_w)
        assert set(out["grads"]) == set(grads_w)
        for k, want in grads_w.items():
            if k in NOISE1D:          # exactly-zero gradients: float64 rounding noise on both sides
                assert float(out["grads"][k].abs().max()) < 1e-9 and float(want.abs().max()) < 1e-9, (tag, k)
                continue
            np.testing.assert_allclose(_f32(out["grads"][k]), want.numpy(), rtol=0, atol=1e-12, err_msg=f"{tag} {k}")
        for bn, (mean_w, var_w, n_w) in stats_w.items():
            mean, var, n = out["stats"][bn]
            assert n == n_w == B * T
            np.testing.assert_allclose(_f32(mean), mean_w.numpy(), rtol=0, atol=1e-12, err_msg=f"{tag} {bn} mean")
            np.testing.assert_allclose(_f32(var), var_w.numpy(), rtol=0, atol=1e-12, err_msg=f"{tag} {bn} var")


def test_helper_with_equal_lengths_matches_reference_autograd_at_321_frames(golden):
    """All lengths = 321: the helper against the reference's OWN autograd / AdamW results (tests/golden/cnn1d_train_t321.npz) at the
    bounds tests/test_oracle_golden.py holds the uniform oracle to on that fixture."""
    _, g = golden("cnn1d_train_t321")
    sd = {k[len("init.sd."):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("init.sd.")}
    x, y, eps = torch.from_numpy(g["x"]).transpose(1, 2), torch.from_numpy(g["y"]), float(g["label_smoothing"])
    out = RO.cnn1d_ragged_train_step(sd, x, [321, 321], y, eps)
    np.testing.assert_allclose(_f32(out["logits"]), g["logits"], atol=2e-4, rtol=1e-5)
    np.testing.assert_allclose(out["loss"], g["loss"], rtol=1e-5)
    for k, got in out["grads"].items():
        if k in NOISE1D:
            continue
        want = g["grad." + k].astype(np.float64)
        scale = max(np.abs(want).max(), 1e-6)
        d = np.abs(got.numpy() - want)
        assert d.max() <= 2e-4 * scale, (k, d.max() / scale)
        assert np.sqrt((d * d).sum()) <= 2e-3 * np.sqrt((want * want).sum()), k
    after = RO.state_after_step(sd, out)
    for k, v in after.items():
        want = g["after1." + k]
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(want), k
        elif k in NOISE1D:
            assert np.abs(v.numpy() - g["init.sd." + k]).max() <= 1.02e-3 + 1e-6, k
        elif k.endswith("running_mean"):
            np.testing.assert_allclose(v.numpy(), want, atol=1e-5 + 1e-3, rtol=2e-4, err_msg=k)
        elif k.endswith("running_var"):
            np.testing.assert_allclose(v.numpy(), want, atol=1e-6, rtol=2e-4, err_msg=k)
        else:
            assert np.abs(v.numpy().astype(np.float64) - want).max() <= 2.05e-3, k


def test_helper_never_reads_the_padding():
    lengths, T_max = [37, 3, 20, 36, 5], 40
    sd = RO.cnn1d_state(seed=7)
    zero, y = RO.ragged_batch(lengths, T_max, seed=1, pad=0.0)
    nan, _ = RO.ragged_batch(lengths, T_max, seed=1, pad=float("nan"))
    assert torch.isnan(nan).any()
    a = RO.cnn1d_ragged_train_step(sd, zero.transpose(1, 2), lengths, y, 0.05)
    b = RO.cnn1d_ragged_train_step(sd, nan.transpose(1, 2), lengths, y, 0.05)
    assert torch.equal(a["logits"], b["logits"]) and a["loss"] == b["loss"]
    for k in a["grads"]:
        assert torch.isfinite(b["grads"][k]).all() and torch.equal(a["grads"][k], b["grads"][k]), k
    for bn in a["stats"]:
        assert torch.equal(a["stats"][bn][0], b["stats"][bn][0]) and torch.equal(a["stats"][bn][1], b["stats"][bn][1])
        assert a["stats"][bn][2] == sum(lengths)


def test_ragged_training_symbols_are_exported():
    """The three prototypes are in the public header, in the ctypes table and in the built library."""
    from dfa_amd import _lib
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in table, name
        assert hasattr(lib, name), name
    assert table[NEW_SYMBOLS[0]][0] is C.c_size_t
    # forward: the uniform forward's arguments plus the host lengths pointer behind the strides; backward: the uniform backward's
    fwd, fwd_u = table[NEW_SYMBOLS[1]][1], table["dfa_cnn1d_forward_train"][1]
    assert fwd == fwd_u[:9] + [C.c_void_p] + fwd_u[9:]
    assert table[NEW_SYMBOLS[2]][1] == table["dfa_cnn1d_backward"][1]


# ---- RaggedBatcher
def _utts(n=23, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.full((4, int(t)), float(i)) for i, t in enumerate(rng.integers(3, 30, n))]


def test_ragged_batcher_default_iteration_is_unchanged():
    """Without shuffle_seed the batches are what they were before the keyword existed: `recorded` is the order the class gave for
    these lengths then (longest first, ties in input order)."""
    from dfa_amd.dataloaders import RaggedBatcher
    lens = [26, 20, 16, 10, 11, 4, 5, 3, 7, 24, 20, 27, 16, 19, 29, 22, 20, 17, 19, 28, 9, 13, 19]
    utts = [torch.full((4, t), float(i)) for i, t in enumerate(lens)]
    recorded = [[14, 19, 11, 0, 9], [15, 1, 10, 16, 13], [18, 22, 17, 2, 12], [21, 4, 3, 20, 8], [6, 5, 7]]
    for kw in ({}, {"shuffle_seed": None}, {"shuffle_seed": None, "bucket": 10}):
        b = RaggedBatcher(utts, np.arange(23, dtype=np.float32), 5, device="cpu", **kw)
        for _ in range(2):            # every pass is the same
            got = []
            for (x, y, lengths), want in zip(b, recorded):
                got.append([int(v) for v in y])
                assert [int(v) for v in lengths] == [lens[i] for i in want]
                assert x.shape[0] == len(want) and x.shape[2] == 4 and x.shape[1] >= max(lens[i] for i in want)
                for j, i in enumerate(want):
                    assert torch.equal(x[j, :lens[i]], utts[i].transpose(0, 1))
                    assert bool((x[j, lens[i]:] == 0).all())
            assert got == recorded
            assert [list(map(int, i)) for i in b.batches] == recorded and len(b) == 5


def test_ragged_batcher_shuffled_epochs():
    from dfa_amd.dataloaders import RaggedBatcher
    utts = _utts(48, seed=1)
    lens = np.array([u.shape[-1] for u in utts])

    def epochs(seed, n=3, **kw):
        b = RaggedBatcher(utts, np.arange(48, dtype=np.float32), 8, device="cpu", shuffle_seed=seed, **kw)
        out = []
        for _ in range(n):
            ep = [[int(v) for v in y] for _, y, _ in b]
            assert ep == [list(map(int, i)) for i in b.batches] and len(b) == len(ep)
            out.append(ep)
        return out, b
    (e1, e2, e3), b = epochs(11)
    for ep in (e1, e2, e3):
        assert sorted(i for batch in ep for i in batch) == list(range(48))       # every utterance exactly once
        assert all(len(batch) == 8 for batch in ep)
    assert e1 != e2 and e2 != e3 and e1 != e3
    assert sorted(map(sorted, e1)) != sorted(map(sorted, e2))                   # other companions, not only another order
    assert epochs(11)[0] == [e1, e2, e3]                                        # the same seed repeats
    assert epochs(12)[0][0] != e1
    # companions are similar in length: inside a bucket of 2 batches the batches are length-sorted, so the padding of an epoch is
    # below that of batches cut from the unsorted permutation
    (s1, *_), _ = epochs(11, bucket=16)
    pad = lambda ep: sum(int(lens[bt].max()) * len(bt) - int(lens[bt].sum()) for bt in ep)      # noqa: E731
    rng = np.random.default_rng(0)
    unsorted = [list(rng.permutation(48)[i:i + 8]) for i in range(0, 48, 8)]
    assert pad(s1) < pad(unsorted)
    # restore() follows the latest epoch
    outs = [torch.tensor(batch, dtype=torch.float32) for batch in b.batches]
    assert torch.equal(b.restore(outs), torch.arange(48, dtype=torch.float32))


# ---- train CLI argument check
def _args(**kw):
    base = dict(model="cnn1d", native=True, swap_tf=True, spec_augment=False, feature_mask=False, time_shift=False, channel_drop=False,
                gaussian_jitter=False, sync_bn=False)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("kw,world,word", [
    (dict(model="cnn2d"), 1, "cnn1d only"),
    (dict(swap_tf=False), 1, "--no-swap-tf"),
    (dict(spec_augment=True), 1, "--spec-augment"),
    (dict(feature_mask=True), 1, "--feature-mask"),
    (dict(time_shift=True), 1, "--time-shift"),
    (dict(channel_drop=True), 1, "--channel-drop"),
    (dict(gaussian_jitter=True), 1, "--gaussian-jitter"),
    (dict(sync_bn=True), 1, "--sync-bn"),
    (dict(), 2, "one rank"),
    (dict(native=False), 1, "--native"),
])
def test_check_ragged_train_args_refuses(kw, world, word):
    from dfa_amd.train import check_ragged_train_args
    with pytest.raises(ValueError, match="unequal lengths") as e:
        check_ragged_train_args(_args(**kw), world)
    assert word in str(e.value)


def test_check_ragged_train_args_accepts_cnn1d_native():
    from dfa_amd.train import check_ragged_train_args, parse_args
    check_ragged_train_args(_args(), 1)
    check_ragged_train_args(parse_args(["--model", "cnn1d", "--native"]), 1)
    with pytest.raises(ValueError):
        check_ragged_train_args(parse_args(["--native"]), 1)               # the default model is cnn2d


@pytest.mark.parametrize("lengths,idx", [([8, 2], 1), ([41, 6], 0)])
def test_host_lengths_names_the_bad_index(lengths, idx):
    from dfa_amd import _lib
    with pytest.raises(ValueError, match=rf"lengths\[{idx}\]={lengths[idx]}"):
        _lib.host_lengths(lengths, 2, 40, 3)
    assert _lib.host_lengths([3, 40], 2, 40, 3).tolist() == [3, 40]
