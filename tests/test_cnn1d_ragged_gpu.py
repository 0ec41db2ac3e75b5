"""Variable-length (ragged) CNN1D batches on the GPU (dfa_cnn1d_forward_ragged, one launch of cnn1d_ragged_x3_kernel) and the
ragged path of `python -m dfa_amd.predict`.

Write uniform(u) for CNN1D()(u_stored[None].transpose(1, 2)) with u_stored the utterance's own contiguous [F, T_u] tensor:
with default options that runs cnn1d_fused_x3_kernel while T_u fits its LDS.  A slice x[b:b+1, :T_b] of the padded batch is
NOT that (its stride_f is T_max: the uniform forward sends it to the exact-fp32 kernel), so the tests copy.  The promises:
every logit within 1e-4 of the fp32 oracle; bit-identical to uniform(u) for every length the uniform split-bf16 kernel takes;
and for every length bit-identical whatever the batch, the position in it and T_max."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dfa_oracle as O

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4                   # the bar tests/test_cnn1d_gpu.py holds every CNN1D kernel to
# every T mod 4, both sides of 321, of the one-window cap (348 at F = 180), of the exact-fp32 kernel's 384; several segments
LENGTHS = [3, 4, 5, 6, 7, 37, 64, 130, 321, 322, 340, 352, 385, 481, 641, 1000]
PATTERNS = [0xFFFF, 0x7FC0, 0x7F80]                     # as tests/test_lds_poison_gpu.py


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _model(golden):
    from dfa_amd.model_cnn1d import CNN1D
    sd, _ = golden("cnn1d_eval")
    m = CNN1D()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to("cuda").eval(), sd


def _utts(lengths, seed, F=180):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(F, int(T), generator=gen) * 3.2 - 0.07 for T in lengths]


def _pad(utts, pad=0.0, extra=0, order=None):
    """stored [B, F, T_pad] batch (T_pad = longest length rounded up to 4, plus `extra` columns), padding filled with `pad`;
    returns the strided [B, T_max, F] view on the GPU and the lengths"""
    order = list(range(len(utts))) if order is None else order
    lengths = [int(utts[i].shape[1]) for i in order]
    T_max = max(lengths)
    stored = torch.full((len(order), utts[0].shape[0], -(-T_max // 4) * 4 + extra), pad)
    for j, i in enumerate(order):
        stored[j, :, :lengths[j]] = utts[i]
    return stored.to("cuda").transpose(1, 2)[:, :T_max + extra], lengths


def _uniform(model, u):
    return model(u.to("cuda")[None].transpose(1, 2))


def test_ragged_matches_oracle_every_length(golden):
    model, sd = _model(golden)
    utts = _utts(LENGTHS, 7)
    x, lengths = _pad(utts)
    got = model(x, lengths=lengths).cpu().numpy()
    assert np.isfinite(got).all()
    for i, u in enumerate(utts):
        want = O.cnn1d_forward(sd, u.numpy().T[None])
        err = float(np.abs(got[i] - want[0]).max())
        print(f"[cnn1d ragged T={LENGTHS[i]}] logit {got[i, 0]:.6f} oracle {want[0, 0]:.6f} |diff| {err:.2e}")
        assert err <= TOL_F32, (LENGTHS[i], err)


def test_ragged_is_bit_identical_to_the_uniform_kernel(golden):
    model, _ = _model(golden)
    utts = _utts(LENGTHS, 8)
    x, lengths = _pad(utts)
    got = model(x, lengths=lengths)
    for i, u in enumerate(utts):
        if LENGTHS[i] <= 340:
            assert torch.equal(got[i:i + 1], _uniform(model, u)), LENGTHS[i]
    same = _utts([64] * 5, 9)
    xs, ls = _pad(same)
    assert torch.equal(model(xs, lengths=ls), model(torch.stack(same).to("cuda").transpose(1, 2)))
    # a tensor in another layout is copied into the channel-major padded batch by the Python layer: same logits
    assert torch.equal(model(x.contiguous(), lengths=lengths), got)


def test_logit_does_not_depend_on_the_batch(golden):
    model, _ = _model(golden)
    utts = _utts(LENGTHS, 10)
    x, lengths = _pad(utts)
    mixed = model(x, lengths=lengths)
    rev = list(range(len(utts)))[::-1]
    xr, lr = _pad(utts, order=rev)
    reversed_ = model(xr, lengths=lr).flip(0)
    xw, _ = _pad(utts, extra=64)
    wide = model(xw, lengths=lengths)
    assert torch.equal(mixed, reversed_)
    assert torch.equal(mixed, wide)
    for i, u in enumerate(utts):
        xa, la = _pad([u])
        alone = model(xa, lengths=la)
        assert torch.equal(alone, mixed[i:i + 1]), LENGTHS[i]
        # beyond the uniform split-bf16 kernel's reach the uniform forward runs the exact-fp32 or the three-launch kernels
        np.testing.assert_allclose(mixed[i:i + 1].cpu().numpy(), _uniform(model, u).cpu().numpy(), atol=TOL_F32, rtol=0,
                                   err_msg=str(LENGTHS[i]))


@pytest.mark.parametrize("pad", [float("nan"), float("inf"), 3.0e38])
@pytest.mark.parametrize("lengths", [LENGTHS, [481, 350, 6, 130], [7, 5, 3], [349, 64]])
def test_padding_is_never_used(golden, pad, lengths):
    """(the longest utterance of three of the batches has T % 4 != 0: the tail float4 of its rows covers the row's own padding;
    lengths over the one-window cap exercise the interior window edges)"""
    model, _ = _model(golden)
    utts = _utts(lengths, 11)
    x0, ls = _pad(utts, pad=0.0, extra=8)
    x1, _ = _pad(utts, pad=pad, extra=8)
    want = model(x0, lengths=ls)
    got = model(x1, lengths=ls)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_ragged_ignores_stale_lds(golden):
    model, _ = _model(golden)
    ctx = _ctx()
    lengths = [1000, 5, 481, 64, 700, 37, 349, 321]        # one-window and multi-segment utterances, short after long
    x, ls = _pad(_utts(lengths, 12))
    want = model(x, lengths=ls).clone()
    for pat in PATTERNS:
        ctx.set_option("poison_lds", pat)
        got = model(x, lengths=ls)
        assert torch.isfinite(got).all()
        assert torch.equal(got, want), hex(pat)


def test_full_size_batch(golden):
    model, sd = _model(golden)
    lengths = np.random.default_rng(321).integers(161, 482, size=256)
    utts = _utts(lengths, 13)
    x, ls = _pad(utts)
    got = model(x, lengths=ls)
    host = got.cpu().numpy()
    worst = 0.0
    for i, u in enumerate(utts):
        want = O.cnn1d_forward(sd, u.numpy().T[None])
        worst = max(worst, float(np.abs(host[i] - want[0]).max()))
    print(f"[cnn1d ragged B=256] max |ragged - oracle| over 256 utterances {worst:.2e}")
    assert worst <= TOL_F32
    parts = []
    for k in range(0, 256, 32):
        xk, lk = _pad(utts[k:k + 32])
        parts.append(model(xk, lengths=lk))
    assert torch.equal(got, torch.cat(parts))


def test_ragged_errors(golden):
    from dfa_amd import _lib
    model, _ = _model(golden)
    x, _ = _pad(_utts([8, 6], 14))
    with pytest.raises(ValueError, match=r"lengths\[1\]=2"):
        model(x, lengths=[8, 2])
    with pytest.raises(ValueError, match=r"lengths\[0\]=9"):
        model(x, lengths=[9, 6])
    with pytest.raises(ValueError, match="3 lengths for a batch of 2"):
        model(x, lengths=[8, 6, 6])
    with pytest.raises(ValueError, match="integers"):
        model(x, lengths=torch.tensor([8.0, 6.0]))
    model.train()
    with pytest.raises(NotImplementedError):
        model(x, lengths=[8, 6])
    model.eval()
    want = model(x, lengths=[8, 6]).clone()
    # the C ABI validates on its own; none of these launches a kernel
    ctx = _ctx()
    ws = ctx.workspace(ctx.lib.dfa_ragged_workspace_bytes(ctx.handle, _lib.MODEL_CNN1D, 2, 8, 180, _lib.PREC_F32))
    out = torch.zeros(2, device="cuda")

    def call(xt, lens, dtype=_lib.DTYPE_F32, strides=None):
        lens = np.asarray(lens, dtype=np.int32)
        return ctx.lib.dfa_cnn1d_forward_ragged(ctx.handle, C.c_void_p(xt.data_ptr()), dtype, 2, 8, 180, *(strides or xt.stride()),
                                                C.c_void_p(lens.ctypes.data), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), ws.numel())
    for bad, msg in (([8, 2], b"lengths[1]=2"), ([10, 6], b"lengths[0]=10")):
        assert call(x, bad) == _lib.E_BAD_SHAPE and msg in ctx.lib.dfa_last_error(ctx.handle)
    assert call(x.to(torch.bfloat16), [8, 6], dtype=_lib.DTYPE_BF16) == _lib.E_BAD_DTYPE
    xc = x.contiguous()
    assert call(xc, [8, 6]) == _lib.E_UNSUPPORTED and b"stride_t" in ctx.lib.dfa_last_error(ctx.handle)
    ctx.set_option("cnn1d_fused", 0)
    try:
        assert call(x, [8, 6]) == _lib.E_UNSUPPORTED and b"cnn1d_fused" in ctx.lib.dfa_last_error(ctx.handle)
    finally:
        ctx.set_option("cnn1d_fused", 1)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                  # nothing ran
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):
        with torch.cuda.graph(g):
            model(x, lengths=[8, 6])
    torch.cuda.synchronize()
    assert torch.equal(model(x, lengths=[8, 6]), want)    # the stream is usable afterwards


def _features_file(tmp_path, lengths, seed):
    import pandas as pd
    feats = _utts(lengths, seed)
    df = pd.DataFrame({"uttid": [f"utt{i:03d}" for i in range(len(feats))], "features": feats})
    path = str(tmp_path / "features.pkl")
    df.to_pickle(path)
    return path, df, feats


def test_predict_cnn1d_scores_a_ragged_file(golden, tmp_path):
    import pandas as pd
    from dfa_amd import predict
    model, _ = _model(golden)
    path, df, feats = _features_file(tmp_path, np.random.default_rng(5).integers(3, 500, size=37), 21)
    ckpt = str(tmp_path / "cnn1d.pt")
    torch.save(model.state_dict(), ckpt)
    out = str(tmp_path / "prediction.pkl")
    predict.main(["--features", path, "--checkpoint", ckpt, "--model", "cnn1d", "--out", out, "--no-apply-sigmoid"])
    pred = pd.read_pickle(out)
    assert list(pred["uttid"]) == list(df["uttid"])
    for i, u in enumerate(feats):
        xa, la = _pad([u])
        assert pred["predictions"][i] == float(model(xa, lengths=la)[0, 0]), (i, u.shape)
    with pytest.raises(ValueError, match="no-swap-tf"):
        predict.main(["--features", path, "--checkpoint", ckpt, "--model", "cnn1d", "--out", out, "--no-swap-tf"])


def test_predict_cnn2d_scores_a_ragged_file_in_bf16(golden, tmp_path):
    import pandas as pd
    from dfa_amd import predict
    from dfa_amd.model import CNN2D
    sd, _ = golden("cnn2d_eval")
    model = CNN2D(precision="bf16")
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to("cuda").eval()
    # (the CNN1D file's draw, from 4 frames: two (2,1) average pools make 4 the shortest utterance CNN2D takes)
    path, df, feats = _features_file(tmp_path, np.random.default_rng(5).integers(4, 500, size=37), 22)
    ckpt = str(tmp_path / "cnn2d.pt")
    torch.save(model.state_dict(), ckpt)
    out, emb_out = str(tmp_path / "prediction.pkl"), str(tmp_path / "emb.pt")
    argv = ["--features", path, "--checkpoint", ckpt, "--model", "cnn2d", "--out", out, "--no-apply-sigmoid"]
    predict.main(argv + ["--precision", "bf16", "--embeddings-out", emb_out])
    pred = pd.read_pickle(out)
    assert list(pred["uttid"]) == list(df["uttid"])
    embs = torch.load(emb_out)
    assert list(embs["uttid"]) == list(df["uttid"]) and embs["embeddings"].shape == (37, 128 * 180)
    for i, u in enumerate(feats):
        xa, la = _pad([u])
        lg, e = model(xa, return_embedding=True, lengths=la)
        assert pred["predictions"][i] == float(lg[0, 0]), (i, u.shape)
        assert torch.equal(embs["embeddings"][i], e[0].cpu()) and float(embs["logits"][i]) == float(lg[0, 0])
    for prec in ("fp32", "bf16x3"):
        with pytest.raises(ValueError, match="--precision bf16 only"):
            predict.main(argv + ["--precision", prec])


def test_predict_equal_lengths_keep_the_stacked_path(golden, tmp_path):
    import pandas as pd
    from dfa_amd import predict
    model, _ = _model(golden)
    path, df, feats = _features_file(tmp_path, [321] * 9, 23)
    ckpt = str(tmp_path / "cnn1d.pt")
    torch.save(model.state_dict(), ckpt)
    out = str(tmp_path / "prediction.pkl")
    predict.main(["--features", path, "--checkpoint", ckpt, "--model", "cnn1d", "--out", out, "--batch-size", "4"])
    pred = pd.read_pickle(out)
    want = predict.predict_scores(model, torch.stack(feats), batch_size=4, device="cuda", apply_sigmoid=True).cpu().tolist()
    assert list(pred["uttid"]) == list(df["uttid"])
    assert list(pred["predictions"]) == [float(s) for s in want]
