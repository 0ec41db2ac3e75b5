"""CNN1D training step on a variable-length (ragged) batch: dfa_cnn1d_forward_train_ragged / dfa_cnn1d_backward_ragged through
NativeTrainer.step(x, y, lengths) against the float64 statement of the definition (tests/ragged_train_oracle.py), bit-identity
with the uniform step at equal lengths, independence of whatever the padding frames, the workspace and LDS hold, the refusals,
and the train CLI end to end.

The oracle bounds are those tests/test_train_shapes_gpu.py holds the uniform CNN1D step to (imported from there): the ragged
step runs the same arithmetic plus masks.  Length sets: the smallest that cross every boundary the kernels have --
  A  every T mod 4, the minimum length 3, utterances shorter than one 16-frame k-step of the weight gradient;
  B  the 256-thread stride of the reductions, the 64-frame weight-gradient slab, the real frame count 321;
  C  T_max > 384: the vector-ALU convolution / data-gradient kernels;
  D  B > 64: a batch chunk of the reductions holds two utterances.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ragged_train_oracle as RO
from test_train_shapes_gpu import NOISE1D, _check_grads, _check_state, _print_log, _to_np

pytestmark = pytest.mark.gpu

F = 180
SETS = {
    "A": ([37, 3, 20, 36, 5], 40),
    "B": ([321, 64, 257], 324),
    "C": ([130, 400], 400),
    "D": ([int(v) for v in np.random.default_rng(70).integers(3, 49, 70)], 48),
}
EPS = 0.05


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _model(sd, dropout=0.0):
    from dfa_amd.model_cnn1d import CNN1D
    m = CNN1D(in_features=F, dropout=dropout)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.to("cuda").train()


_cache = {}


def _case(name):
    """(state_dict, stored [B, F, T_max] with zero padding, y, lengths, T_max, the helper's result, the state after its step):
    computed once per length set and shared, never modified."""
    if name not in _cache:
        lengths, T_max = SETS[name]
        sd = RO.cnn1d_state(seed=5 + T_max)
        stored, y = RO.ragged_batch(lengths, T_max, seed=1000 + T_max)
        want = RO.cnn1d_ragged_train_step(sd, stored.transpose(1, 2), lengths, y, EPS)
        _cache[name] = (sd, stored, y, lengths, T_max, want, RO.state_after_step(sd, want))
    return _cache[name]


def _x(stored, layout="stored"):
    """stored: the [B, F, T] storage seen as [B, T, F] (channel-major kernels); btf: contiguous [B, T, F] (strided kernels)."""
    x = stored.to("cuda").transpose(1, 2)
    return x if layout == "stored" else x.contiguous()


def _step(sd, x, y, lengths, dropout=0.0, before=None):
    """One NativeTrainer.step on a fresh model; returns logits, loss, the gradients as they stood before the update, the
    state_dict after it."""
    from dfa_amd.training import train_step as TS
    m = _model(sd, dropout)
    m._drop_seed, m._drop_offset = 1234, 0
    tr = TS.NativeTrainer(m, lr=1e-3, weight_decay=0.01, label_smoothing=EPS)
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
        if before is not None:
            before(m, x)
        got["loss"] = tr.step(x, y.to("cuda"), lengths).detach().clone()
    finally:
        TS.forward_train_raw = fwd
    got["state"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.cuda.synchronize()
    return got


def _same(a, b, tag):
    assert torch.equal(a["logits"], b["logits"]), tag
    assert torch.equal(a["loss"], b["loss"]), tag
    for (n, ga), (_, gb) in zip(a["grads"], b["grads"]):
        assert torch.equal(ga, gb), (tag, n)
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), (tag, k)


def _finite(r, tag):
    assert torch.isfinite(r["logits"]).all() and torch.isfinite(r["loss"]).all(), tag
    for n, g in r["grads"]:
        assert torch.isfinite(g).all(), (tag, n)
    for k, v in r["state"].items():
        assert torch.isfinite(v.float()).all(), (tag, k)


# ------------------------------------------------------------------------------------------------ 1. oracle parity
def _parity(name, x3=1, layout="stored"):
    sd, stored, y, lengths, T_max, want, after_w = _case(name)
    ctx = _ctx()
    ctx.set_option("cnn1d_train_x3", x3)
    try:
        got = _step(sd, _x(stored, layout), y, lengths)
    finally:
        ctx.set_option("cnn1d_train_x3", 1)
    log = []
    tag = f"cnn1d ragged set {name} x3={x3} {layout} vs float64 helper"
    d = np.abs(_to_np(got["logits"]) - want["logits"].numpy())
    print(f"[{tag}] logits max err {d.max():.2e}, loss {got['loss'].item():.8f} vs {want['loss']:.8f}")
    try:
        np.testing.assert_allclose(_to_np(got["logits"]), want["logits"].numpy(), atol=2e-4, rtol=1e-5)
        np.testing.assert_allclose(got["loss"].item(), want["loss"], rtol=1e-5)
        _check_grads(got["grads"], {k: v.float() for k, v in want["grads"].items()}, NOISE1D, log=log)
        _check_state(got["state"], after_w, sd, NOISE1D, log=log)
    finally:
        _print_log(tag, log or [("-", 0.0, 0.0, 0)])


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_ragged_step_matches_the_float64_definition(name):
    _parity(name)


@pytest.mark.parametrize("x3", [0, 3])
def test_ragged_step_matches_the_definition_under_every_x3_option(x3):
    """Option 0: the fp32 vector-ALU convolutions and the fp32 matrix-core weight gradient; 3: two bf16 terms per operand."""
    _parity("A", x3=x3)


def test_ragged_step_matches_the_definition_on_a_contiguous_btf_batch():
    """x contiguous as [B, T, F]: frames are not contiguous, layer 1 takes the strided convolution."""
    _parity("A", layout="btf")


# ------------------------------------------------------------------------------------------------ 2. equal lengths = the uniform step
@pytest.mark.parametrize("B,T", [(4, 40), (2, 321)])
@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_equal_lengths_are_the_uniform_step_bit_for_bit(B, T, dropout):
    from dfa_amd.training import train_step as TS
    sd = RO.cnn1d_state(seed=9 + T)
    stored, _ = RO.ragged_batch([T] * B, T, seed=77 + T)
    x = _x(stored)
    g = torch.Generator().manual_seed(3)
    dlogits = (torch.randn(B, generator=g) * 0.1).to("cuda")
    res = []
    for lengths in (None, [T] * B):
        m = _model(sd, dropout)
        m._drop_seed, m._drop_offset = 99, 16          # the same Philox key and offset for both
        (logits,), st = TS.forward_train_raw(m, x, lengths=lengths)
        grads = [torch.full_like(p, float("nan")) for p in m.parameters()]
        TS.backward_raw(m, x, dlogits, grads, st)
        torch.cuda.synchronize()
        stats = [getattr(m.conv[i], n).clone() for i in m._BN_IDX for n in ("running_mean", "running_var")]
        res.append((logits.clone(), grads, stats))
    (lu, gu, su), (lr, gr, sr) = res
    assert torch.isfinite(lu).all() and torch.equal(lu, lr)
    assert len(gu) == 14 and len(su) == 6
    for (n, _), a, b in zip(m.named_parameters(), gu, gr):
        assert torch.isfinite(a).all() and torch.equal(a, b), n
    for a, b in zip(su, sr):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. padding is never used
@pytest.mark.parametrize("name", ["A", "B"])
def test_padding_frames_are_never_used(name):
    sd, _, y, lengths, T_max, _, _ = _case(name)
    res = {}
    for pad in (float("nan"), 3e38, 0.0):
        stored, _ = RO.ragged_batch(lengths, T_max, seed=1000 + T_max, pad=pad)
        res[pad if pad == pad else "nan"] = _step(sd, _x(stored), y, lengths)
    _finite(res[0.0], "zero padding")
    _same(res["nan"], res[0.0], "NaN padding")
    _same(res[3e38], res[0.0], "3e38 padding")


def test_padding_frames_are_never_used_by_the_strided_and_vector_kernels():
    """The same for the kernels the default path does not reach at set A: option 0 (vector-ALU convolution, fp32 matrix-core
    weight gradient) on the stored layout and on a contiguous [B, T, F] batch."""
    sd, _, y, lengths, T_max, _, _ = _case("A")
    ctx = _ctx()
    ctx.set_option("cnn1d_train_x3", 0)
    try:
        for layout in ("stored", "btf"):
            res = []
            for pad in (float("nan"), 0.0):
                stored, _ = RO.ragged_batch(lengths, T_max, seed=1000 + T_max, pad=pad)
                res.append(_step(sd, _x(stored, layout), y, lengths))
            _finite(res[1], layout)
            _same(res[0], res[1], layout)
    finally:
        ctx.set_option("cnn1d_train_x3", 1)


# ------------------------------------------------------------------------------------------------ 4. stale memory
def test_stale_workspace_and_lds_change_nothing():
    sd, stored, y, lengths, T_max, _, _ = _case("A")
    x = _x(stored)
    ctx = _ctx()
    clean = _step(sd, x, y, lengths)

    def nan_workspace(m, xx):
        n = ctx.lib.dfa_cnn1d_train_ragged_workspace_bytes(ctx.handle, xx.shape[0], xx.shape[1], xx.shape[2])
        assert n > 0
        m._train_ws = torch.full((int(n),), 0xFF, dtype=torch.uint8, device="cuda")       # every float a NaN

    _same(_step(sd, x, y, lengths, before=nan_workspace), clean, "NaN-filled workspace")
    for pat in (0xFFFF, 0x7FC0, 0x7F80):
        _same(_step(sd, x, y, lengths, before=lambda m, xx: ctx.set_option("poison_lds", pat)), clean, f"LDS poisoned {pat:#x}")


# ------------------------------------------------------------------------------------------------ 5. errors
def test_refusals_name_their_cause_and_leave_the_context_usable():
    from dfa_amd import _lib
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.training import train_step as TS
    sd, stored, y, lengths, T_max, _, _ = _case("A")
    B = len(lengths)
    x = _x(stored)
    ctx = _ctx()
    lib, h = ctx.lib, ctx.handle
    m = _model(sd)
    dlogits = torch.full((B,), 0.01, device="cuda")
    grads = [torch.empty_like(p) for p in m.parameters()]
    logits = torch.empty(B, device="cuda")

    def good():
        (lg,), st = TS.forward_train_raw(m, x, lengths=lengths)
        TS.backward_raw(m, x, dlogits, grads, st)
        torch.cuda.synchronize()
        assert torch.isfinite(lg).all() and all(torch.isfinite(g).all() for g in grads)
        return st
    st = good()
    ws = st.ws
    err = lambda: lib.dfa_last_error(h).decode()      # noqa: E731

    def fwd_ragged(xx=x, lens=lengths, nbytes=None, dtype=_lib.DTYPE_F32):
        arr = np.asarray(lens, dtype=np.int32)
        return lib.dfa_cnn1d_forward_train_ragged(h, C.c_void_p(xx.data_ptr()), dtype, B, T_max, F, *xx.stride(), C.c_void_p(arr.ctypes.data),
                                                  0.0, 1, 0, 0.1, 0, C.c_void_p(logits.data_ptr()), C.c_void_p(ws.data_ptr()),
                                                  ws.numel() if nbytes is None else nbytes)

    def fwd_uniform():
        return lib.dfa_cnn1d_forward_train(h, C.c_void_p(x.data_ptr()), _lib.DTYPE_F32, B, T_max, F, *x.stride(), 0.0, 1, 0, 0.1, 0,
                                           C.c_void_p(logits.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel())

    def bwd(name):
        return getattr(lib, name)(h, C.c_void_p(x.data_ptr()), _lib.DTYPE_F32, B, T_max, F, *x.stride(), C.c_void_p(dlogits.data_ptr()),
                                  _lib.ptr_array(grads), 14, C.c_void_p(ws.data_ptr()), ws.numel())
    with torch.cuda.device(ctx.index):
        ctx.use_current_stream()
        # the pairs do not mix
        assert fwd_ragged() == _lib.DFA_OK
        assert bwd("dfa_cnn1d_backward") == _lib.E_NOT_PREPARED and "dfa_cnn1d_backward must follow" in err()
        assert bwd("dfa_cnn1d_backward_ragged") == _lib.DFA_OK
        assert fwd_uniform() == _lib.DFA_OK
        assert bwd("dfa_cnn1d_backward_ragged") == _lib.E_NOT_PREPARED and "dfa_cnn1d_forward_train_ragged" in err()
        assert bwd("dfa_cnn1d_backward") == _lib.DFA_OK
        good()
        # an armed augmentation
        _lib.check(h, lib.dfa_cnn1d_set_train_augment(h, 1, T_max, F, 3, None, 0, 0, 0, 0, 0.0, 0, 0))
        assert fwd_ragged() == _lib.E_UNSUPPORTED and "augment" in err()
        good()                                          # (the arm was one-shot: consumed by the refused call)
        # an armed SyncBN hook
        hook = _lib.BnSync.FN(lambda user, buf, count: 0)
        buf = torch.zeros(1024, device="cuda")
        _lib.check(h, lib.dfa_ctx_set_bn_sync(h, C.cast(hook, C.c_void_p), None, 1, C.c_void_p(buf.data_ptr()), buf.numel()))
        try:
            assert fwd_ragged() == _lib.E_UNSUPPORTED and "BatchNorm" in err()
        finally:
            _lib.check(h, lib.dfa_ctx_set_bn_sync(h, None, None, 1, None, 0))
        good()
        # workspace, dtype, lengths
        need = lib.dfa_cnn1d_train_ragged_workspace_bytes(h, B, T_max, F)
        assert need > lib.dfa_cnn1d_train_workspace_bytes(h, B, T_max, F) > 0
        assert fwd_ragged(nbytes=need - 1) == _lib.E_WORKSPACE and "too small" in err()
        assert fwd_ragged(nbytes=lib.dfa_cnn1d_train_workspace_bytes(h, B, T_max, F)) == _lib.E_WORKSPACE
        good()
        xb = x.to(torch.bfloat16)
        assert fwd_ragged(xx=xb, dtype=_lib.DTYPE_BF16) == _lib.E_BAD_DTYPE
        good()
        for bad, msg in (([8, 2] + lengths[2:], "lengths[1]=2"), ([41, 6] + lengths[2:], "lengths[0]=41")):
            assert fwd_ragged(lens=bad) == _lib.E_BAD_SHAPE and msg in err(), (bad, err())
        good()
    # the Python entry points refuse before anything is launched
    with pytest.raises(ValueError, match=r"lengths\[1\]=2"):
        TS.forward_train_raw(m, x, lengths=[8, 2] + lengths[2:])
    tr = TS.NativeTrainer(_model(sd), label_smoothing=EPS)
    with pytest.raises(ValueError, match=r"lengths\[0\]=41"):
        tr.step(x, y.to("cuda"), [41, 6] + lengths[2:])
    with pytest.raises(ValueError):
        TS.forward_train_raw(m, x.to(torch.bfloat16), lengths=lengths)
    from dfa_amd.model import CNN2D
    with pytest.raises(ValueError, match="CNN1D only in this version"):
        TS.NativeTrainer(CNN2D(in_features=F).to("cuda")).step(x, y.to("cuda"), lengths)
    # a capturing stream (everything is prepared and sized: the capture launches nothing)
    good()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):
        with torch.cuda.graph(g):
            TS.forward_train_raw(m, x, lengths=lengths)
    torch.cuda.synchronize()
    good()
    # the autograd bridge has no ragged form
    with pytest.raises(NotImplementedError):
        CNN1D(in_features=F).to("cuda").train()(x, lengths=lengths)


# ------------------------------------------------------------------------------------------------ 6. CLI end to end
def _write_set(path, n, seed, lo=20, hi=60):
    """A separable ragged set in the reference's pickle schema, built as tests/eer_set.py builds its own: class 1 = class 0 plus
    a fixed low-rank pattern of per-utterance strength."""
    import pandas as pd
    g = torch.Generator().manual_seed(seed)
    gp = torch.Generator().manual_seed(4242)            # the pattern is the same for the train and the dev set
    u, v = torch.randn(F, 2, generator=gp), torch.randn(2, hi, generator=gp)
    pattern = (u @ v) / 2.0
    lengths = torch.randint(lo, hi + 1, (n,), generator=g).tolist()
    labels = (torch.arange(n) % 2).long()
    feats = []
    for i, t in enumerate(lengths):
        f = torch.randn(F, t, generator=g) * 3.2 - 0.07
        strength = 1.5 * (1.0 + 0.3 * float(torch.randn((), generator=g)))
        feats.append((f + float(labels[i]) * strength * pattern[:, :t]).clamp_(-61.0, 87.0))
    uttids = [f"utt_{seed}_{i:04d}" for i in range(n)]
    os.makedirs(path, exist_ok=True)
    pd.DataFrame({"uttid": uttids, "features": feats}).to_pickle(os.path.join(path, "features.pkl"))
    pd.DataFrame({"uttid": uttids, "label": labels.numpy().astype(np.int64)}).to_pickle(os.path.join(path, "labels.pkl"))
    return feats, labels.numpy().astype(np.float32)


def test_train_cli_on_a_ragged_set(tmp_path, capsys):
    from dfa_amd import train
    from dfa_amd.evaluation import evaluate_ragged
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.predict import load_weights
    _write_set(str(tmp_path / "train"), 48, seed=1)
    dev_feats, dev_labels = _write_set(str(tmp_path / "dev"), 16, seed=2)
    assert len({f.shape[-1] for f in dev_feats}) > 1

    def run(tag):
        argv = ["--train-features", str(tmp_path / "train" / "features.pkl"), "--train-labels", str(tmp_path / "train" / "labels.pkl"),
                "--dev-features", str(tmp_path / "dev" / "features.pkl"), "--dev-labels", str(tmp_path / "dev" / "labels.pkl"),
                "--model", "cnn1d", "--native", "--epochs", "2", "--batch-size", "8", "--seed", "7", "--dropout", "0.2",
                "--label-smoothing", "0.05", "--checkpoint-dir", str(tmp_path / tag)]
        capsys.readouterr()
        train.main(argv)
        out = capsys.readouterr().out
        rows = re.findall(r"epoch (\d+): train_loss=(\S+) dev_loss=(\S+) dev_eer=(\S+)", out)
        assert [int(r[0]) for r in rows] == [1, 2], out
        return [(float(a), float(b), float(c)) for _, a, b, c in rows], out
    rows, out = run("run1")
    assert all(np.isfinite(v) for r in rows for v in r), out
    best, last = tmp_path / "run1" / "cnn1d_best.pt", tmp_path / "run1" / "cnn1d_last.pt"
    assert best.exists() and last.exists()
    criterion = train.make_criterion(0.05)
    for path, epoch in ((last, 2), (best, None)):
        m = CNN1D(in_features=F, dropout=0.2).to("cuda")
        load_weights(m, str(path), "cuda")
        metrics, scores, labels = evaluate_ragged(m, dev_feats, dev_labels, criterion=criterion, device="cuda", batch_size=8)
        assert len(scores) == len(labels) == 16 and labels == dev_labels.tolist()
        got = (f"{metrics['avg_loss']:.6f}", f"{metrics['eer']:.6f}")
        printed = [(f"{r[1]:.6f}", f"{r[2]:.6f}") for r in rows]
        if epoch is not None:
            assert got == printed[epoch - 1], (got, printed)
        else:                                       # the best checkpoint is one of the two epochs, the one marked *best* last
            assert got in printed, (got, printed)
    rows2, _ = run("run2")
    assert [r[0] for r in rows2] == [r[0] for r in rows]          # the same seed: the identical train loss
    assert rows2 == rows
