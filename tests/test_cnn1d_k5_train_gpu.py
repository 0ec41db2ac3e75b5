"""GPU tests of the uniform training step of the k = (5, 3, 3) CNN1D variant (dfa_cnn1d_forward_train / dfa_cnn1d_backward with a
five-tap layer 1), on both arithmetic options: cnn1d_train_x3 = 0 -- conv1d.hip<K = 5> forward, conv1d_wgrad_mfma_kernel<K = 5>
weight gradient; 1 -- the streamed conv1d_x3_kernel<K = 5> forward (conv1d_x3.hip), conv1d_wgrad_x3_kernel<K = 5> weight gradient.

Bounds are those of the three-tap cases of tests/test_train_shapes_gpu.py: logits atol 2e-4 / rtol 1e-5, loss rtol 1e-5, a
gradient within 3e-2 of its scale in every element and 3e-3 in relative L2 (LOOSE, L2TOL: tolerant of single ReLU flips), a conv
bias in front of a batch-statistics BatchNorm below 1e-4 of its weight gradient's scale.  conv.0.weight is held to them tap by tap."""
import functools
import random

import numpy as np
import pytest
import torch

import cnn1d_k5_oracle as KO

pytestmark = pytest.mark.gpu
K5 = (5, 3, 3)
NOISE1D = ("conv.0.bias", "conv.4.bias", "conv.8.bias")
LOOSE, L2TOL = 3e-2, 3e-3             # tests/test_train_shapes_gpu.py


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _close(got, want, name):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(np.abs(want).max(), 1e-6)
    d = np.abs(got - want)
    rel_l2 = float(np.sqrt((d * d).sum() / max((want * want).sum(), 1e-30)))
    print(f"    {name}: max {d.max() / scale:.2e} of scale, rel l2 {rel_l2:.2e}")
    assert d.max() <= LOOSE * scale, (name, float(d.max() / scale))
    assert rel_l2 <= L2TOL, (name, rel_l2)


def _check(model, logits, loss, want_logits, want_loss, want_grads, tag):
    print(f"[cnn1d k5 train {tag}] logits {logits.detach().cpu().numpy()} want {np.asarray(want_logits).reshape(-1)}")
    np.testing.assert_allclose(logits.detach().cpu().numpy(), np.asarray(want_logits).reshape(-1), atol=2e-4, rtol=1e-5)
    np.testing.assert_allclose(float(loss), float(want_loss), rtol=1e-5)
    for name, p in model.named_parameters():
        got = p.grad.detach().cpu().numpy()
        if name in NOISE1D:
            floor = 1e-4 * float(np.abs(want_grads[name.replace("bias", "weight")]).max()) + 1e-6
            assert float(np.abs(got).max()) < floor, (name, float(np.abs(got).max()), floor)
            continue
        _close(got, want_grads[name], name)
        if name == "conv.0.weight":
            assert got.shape[2] == 5
            for k in range(5):
                _close(got[:, :, k], want_grads[name][:, :, k], f"conv.0.weight tap {k}")


def _step(sd, x_btf, y, x3, F=180):
    """one train-mode forward + backward of the variant (dropout 0, plain BCE-with-logits) on the stored layout"""
    from dfa_amd.model_cnn1d import CNN1D
    ctx = _ctx()
    m = CNN1D(in_features=F, dropout=0.0, kernels=K5)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to("cuda").train()
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(x_btf).swapaxes(1, 2))).to("cuda").transpose(1, 2)
    try:
        ctx.set_option("cnn1d_train_x3", x3)
        logits = m(x).squeeze(-1)
        loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(np.asarray(y, dtype=np.float32)).to("cuda"))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ctx.set_option("cnn1d_train_x3", 1)
    return m, logits, loss


@pytest.mark.parametrize("x3", [0, 1])
def test_train_step_matches_reference_autograd(golden, x3):
    sd, _ = golden("cnn1d_k533_eval")
    _, t = golden("cnn1d_k533_train")
    m, logits, loss = _step(sd, t["x"], t["y"], x3)
    want = {k[5:]: v for k, v in t.items() if k.startswith("grad.")}
    _check(m, logits, loss, t["logits"], t["loss"], want, f"[2,33,180] x3={x3} vs reference autograd")


@functools.lru_cache(maxsize=None)
def _oracle_case(B, T, F):
    """seeded default initialisation with the BatchNorm affine and the classifier moved off their defaults (the construction of
    tests/test_train_shapes_gpu.py's three-tap case), an input at the stored features' scale, both labels present; the float64
    oracle's step is computed once and shared by the two arithmetic options"""
    from dfa_amd.model_cnn1d import CNN1D
    torch.manual_seed(5 + T)
    m = CNN1D(in_features=F, dropout=0.0, kernels=K5)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for i in (1, 5, 9):
            m.conv[i].weight.copy_(0.5 + torch.rand(m.conv[i].weight.shape, generator=g))
            m.conv[i].bias.copy_(0.1 * torch.randn(m.conv[i].bias.shape, generator=g))
        m.classifier.weight.mul_(40.0)
    sd = {k: v.detach().clone().numpy() for k, v in m.state_dict().items()}
    x = (torch.randn(B, F, T, generator=g) * 3.2 - 0.07).transpose(1, 2).numpy()
    y = np.asarray([float(i % 2) for i in range(B)], dtype=np.float32)
    return sd, x, y, KO.train_step(sd, x, y)


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("B,T,F", [(2, 3, 180), (3, 65, 8), (2, 321, 180), (2, 259, 20), (2, 33, 36)])
def test_train_step_matches_float64_oracle(B, T, F, x3):
    sd, x, y, (logits_w, loss_w, grads_w) = _oracle_case(B, T, F)
    m, logits, loss = _step(sd, x, y, x3, F)
    _check(m, logits, loss, logits_w, loss_w, grads_w, f"[{B},{T},{F}] x3={x3} vs float64 oracle")


def test_two_term_option_stays_within_the_three_tap_logit_bound():
    """option 3 (two bf16 terms per operand, conv1d_x3_kernel<1, 2, K = 5>): logits within 1e-4 * max(1, |logit|) of the fp32
    kernels', the bound tests/test_cnn1d_gpu.py holds the three-tap two-term arm to"""
    sd, x, y, _ = _oracle_case(2, 321, 180)
    _, l0, _ = _step(sd, x, y, 0)
    _, l3, _ = _step(sd, x, y, 3)
    err, scale = float((l3 - l0).abs().max()), max(1.0, float(l0.abs().max()))
    print(f"[cnn1d k5 train two terms] |logits - fp32| {err:.2e}, scale {scale:.2f}")
    assert err <= 1e-4 * scale


def test_augmentation_folded_into_the_five_tap_loads_equals_standalone_pass():
    """the construction of tests/test_augment_gpu.py's three-tap test: FusedAugment(fold="cnn1d") arms
    dfa_cnn1d_set_train_augment and the two kernels that read x (five-tap layer-1 convolution and weight gradient) apply the
    element formula in their loads -- logits and all 14 gradients bit-identical to the stand-alone dfa_augment_batch pass, on
    both arithmetic options, for the stored layout (a view) and a dense [B, T, F] batch"""
    from dfa_amd.augmentation import FusedAugment
    from dfa_amd.model_cnn1d import CNN1D
    cfg = dict(spec_augment=True, time_mask_ratio=0.2, feature_mask=True, feature_mask_ratio=0.1, time_shift=True,
               time_shift_ratio=0.1, channel_drop=True, channel_drop_prob=0.3, gaussian_jitter=True, gaussian_jitter_std=0.05)
    ctx = _ctx()
    g = torch.Generator().manual_seed(6)
    for layout, (B, T, F) in (("bft_view", (3, 70, 180)), ("btf", (2, 17, 45))):
        stored = (torch.randn(B, F, T, generator=g) if layout == "bft_view" else torch.randn(B, T, F, generator=g)) * 3.0
        x = stored.to("cuda").transpose(1, 2) if layout == "bft_view" else stored.to("cuda")
        y = (torch.rand(B, generator=g) > 0.5).float().to("cuda")
        for x3 in (0, 1, 3):
            results = []
            try:
                ctx.set_option("cnn1d_train_x3", x3)
                for fold in (False, "cnn1d"):
                    torch.manual_seed(9)
                    model = CNN1D(in_features=F, dropout=0.2, kernels=K5).to("cuda").train()
                    model._drop_seed = 123
                    with torch.no_grad():
                        model.classifier.weight.mul_(30.0)
                    random.seed(31)
                    torch.manual_seed(31)
                    xa = FusedAugment(seed=77, fold=fold, **cfg)(x)
                    if fold:
                        assert xa.data_ptr() == x.data_ptr()
                    logits = model(xa).squeeze(-1)
                    torch.nn.BCEWithLogitsLoss()(logits, y).backward()
                    results.append((logits.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
            finally:
                ctx.set_option("cnn1d_train_x3", 1)
            (l0, g0), (l1, g1) = results
            assert torch.equal(l0, l1), (layout, x3, float((l0 - l1).abs().max()))
            assert len(g0) == 14 and tuple(g0["conv.0.weight"].shape) == (32, F, 5)
            for n in g0:
                assert torch.equal(g0[n], g1[n]), (layout, x3, n, float((g0[n] - g1[n]).abs().max()))


def test_native_trainer_step_and_flat_gradient_size():
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.training.train_step import NativeTrainer
    torch.manual_seed(3)
    model = CNN1D(dropout=0.2, kernels=K5).to("cuda")
    nparams = sum(p.numel() for p in model.parameters())
    assert nparams == sum(p.numel() for p in CNN1D().parameters()) + 32 * 180 * 2
    tr = NativeTrainer(model, lr=1e-3, label_smoothing=0.05)
    assert tr.flat_g.numel() * tr.flat_g.element_size() == 4 * nparams == tr.flat_p.numel() * 4
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(4, 180, 33, generator=g) * 3.2 - 0.07).to("cuda").transpose(1, 2)
    y = torch.tensor([1.0, 0.0, 1.0, 0.0], device="cuda")
    before = tr.flat_p.clone()
    l0 = float(tr.step(x, y))
    l1 = float(tr.step(x, y))
    assert np.isfinite(l0) and np.isfinite(l1)
    assert torch.isfinite(tr.flat_g).all() and float(tr.flat_g.abs().max()) > 0
    w0 = model.conv[0].weight
    assert tuple(w0.shape) == (32, 180, 5) and w0.data_ptr() >= tr.flat_p.data_ptr()      # a view of the flat buffer
    moved = (tr.flat_p - before).abs()
    assert float(moved.max()) > 0 and float(moved.max()) <= 2.1e-3                          # two AdamW steps of lr 1e-3
