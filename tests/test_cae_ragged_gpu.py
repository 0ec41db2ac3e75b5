"""Variable-length (ragged) auto-encoder scoring on the GPU (dfa_cae_score_ragged, bf16 precision).

Utterance b of a ragged batch must get the score ConvAutoencoder.score gives x[b:b+1, :T_b] alone, bit for bit: the ragged
kernels take their row masks, layer heights, decoder tile partition, tail rows and divisor from T_b, and nothing in the uniform
bf16 path depends on the batch.  The ragged ensemble CLIs (predict_hybrid, hybrid_ensemble, ensemble) are run end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RESIDUES = list(range(16, 48))        # every T mod 16, every parity at each of the four pools, H4 in {1, 2}
MIXED = [321, 70, 64, 481, 161, 16, 333, 17]
PATTERNS = [0xFFFF, 0x7FC0, 0x7F80]   # as tests/test_lds_poison_gpu.py


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _model(golden, precision="bf16"):
    from dfa_amd.model_cae import ConvAutoencoder
    sd, g = golden("cae_eval")
    m = ConvAutoencoder(precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to("cuda").eval(), g


def _stats(seed=5, F=180):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(F, generator=gen) * 0.3).to("cuda"), (torch.rand(F, generator=gen) + 0.5).to("cuda")


def _ragged(lengths, seed, F=180, pad=0.0, dtype=torch.float32, layout="stored", extra=0):
    """the padded [B, T_max (+ extra), F] view of a ragged batch, padding filled with `pad`.  layout "stored": [B][F][T_pad]
    storage seen through the transposed view (what dataloaders.RaggedBatcher yields); "plain": a contiguous [B, T_max, F]."""
    gen = torch.Generator().manual_seed(seed)
    T_max = max(lengths) + extra
    stored = torch.full((len(lengths), F, T_max), pad)
    for i, T in enumerate(lengths):
        stored[i, :, :T] = torch.randn(F, T, generator=gen) * 1.3 - 0.07
    stored = stored.to(dtype).to("cuda")
    return stored.transpose(1, 2) if layout == "stored" else stored.transpose(1, 2).contiguous()


def _alone(model, x, lengths, mean=None, std=None):
    """the uniform score of every utterance alone, at its own length"""
    return torch.cat([model.score(x[i:i + 1, :int(T)], mean, std) for i, T in enumerate(lengths)])


@pytest.mark.parametrize("layout", ["stored", "plain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("zscore", [False, True])
def test_every_residue_is_bit_identical_to_the_utterance_alone(golden, zscore, dtype, layout):
    model, _ = _model(golden)
    mean, std = _stats() if zscore else (None, None)
    x = _ragged(RESIDUES, 3, dtype=dtype, layout=layout)
    got = model.score(x, mean, std, lengths=RESIDUES)
    want = _alone(model, x, RESIDUES, mean, std)
    assert torch.isfinite(got).all()
    bad = [(RESIDUES[i], float(got[i]), float(want[i])) for i in range(len(RESIDUES)) if got[i] != want[i]]
    assert torch.equal(got, want), bad[:8]
    assert torch.equal(model.score(x, mean, std, lengths=torch.tensor(RESIDUES, device="cuda")), want)


def test_mixed_long_batch_position_and_padding_independent(golden):
    model, _ = _model(golden)
    mean, std = _stats()
    x = _ragged(MIXED, 4, dtype=torch.bfloat16)
    want = _alone(model, x, MIXED, mean, std)
    got = model.score(x, mean, std, lengths=MIXED)
    assert torch.equal(got, want), (got - want).abs().max()
    rev = model.score(x.flip(0), mean, std, lengths=MIXED[::-1])
    assert torch.equal(rev.flip(0), want)
    xp = _ragged(MIXED, 4, dtype=torch.bfloat16, extra=37, pad=float("nan"))
    assert xp.shape[1] == max(MIXED) + 37
    assert torch.equal(model.score(xp, mean, std, lengths=MIXED), want)


def test_full_size_batch_equals_small_batches_and_uniform_groups(golden):
    """B = 256, lengths uniform in [161, 481]: equal to eight ragged batches of 32 and to uniform calls on equal-length groups"""
    model, _ = _model(golden)
    mean, std = _stats()
    lengths = np.random.default_rng(2025).integers(161, 482, size=256)
    x = _ragged(lengths.tolist(), 6, dtype=torch.bfloat16)
    got = model.score(x, mean, std, lengths=lengths)
    parts = []
    for i in range(0, 256, 32):
        l = lengths[i:i + 32]
        parts.append(model.score(x[i:i + 32, :int(l.max())], mean, std, lengths=l))
    assert torch.equal(got, torch.cat(parts))
    for T in np.unique(lengths):
        idx = torch.from_numpy(np.nonzero(lengths == T)[0]).to("cuda")
        want = model.score(x.index_select(0, idx)[:, :int(T)], mean, std)
        assert torch.equal(got.index_select(0, idx), want), int(T)


@pytest.mark.parametrize("T", [16, 70, 321])
def test_equal_lengths_ragged_equals_uniform_call(golden, T):
    model, _ = _model(golden)
    mean, std = _stats()
    x = _ragged([T] * 6, 9)
    assert torch.equal(model.score(x, mean, std, lengths=[T] * 6), model.score(x, mean, std))
    assert torch.equal(model.score(x, lengths=np.full(6, T)), model.score(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pad", [float("nan"), float("inf"), 3.0e38])
def test_padding_and_stale_workspace_are_never_read(golden, pad, dtype):
    from dfa_amd import _lib
    model, _ = _model(golden)
    ctx = _ctx()
    mean, std = _stats()
    lengths = RESIDUES[::3] + MIXED
    x0 = _ragged(lengths, 11, pad=0.0, dtype=dtype)
    x1 = _ragged(lengths, 11, pad=pad, dtype=dtype)
    want = model.score(x0, mean, std, lengths=lengths).clone()
    assert torch.equal(want, _alone(model, x0, lengths, mean, std))
    B, T, F = x1.shape
    nbytes = ctx.lib.dfa_cae_ragged_workspace_bytes(ctx.handle, B, T, F, _lib.PREC_BF16)
    for pat in PATTERNS:
        ctx.set_option("poison_lds", pat)
        ws = ctx.workspace(nbytes)
        # every activation and partial sum of the workspace: a NaN / Inf bit pattern
        ws[:ws.numel() // 2 * 2].view(torch.int16).fill_(pat - 0x10000 if pat >= 0x8000 else pat)
        got = model.score(x1, mean, std, lengths=lengths)
        assert ctx.workspace(nbytes).data_ptr() == ws.data_ptr()                # the call ran in the poisoned workspace
        assert torch.isfinite(got).all(), hex(pat)
        assert torch.equal(got, want), (hex(pat), (got - want).abs().max())


def test_golden_utterances_inside_a_mixed_batch_meet_the_bf16_bar(golden):
    """Independent of the uniform kernels: the two golden T = 321 utterances, scored with other lengths around them, against
    the fp32 reference's score at the model's existing bf16 bar (tests/test_cae_gpu.py::test_cae_bf16_mode_close)."""
    model, g = _model(golden)
    gx = torch.from_numpy(g["t321.x"])
    assert gx.shape[0] >= 2 and gx.shape[1] == 321
    lengths = [481, 321, 17, 70, 321, 400, 16]
    x = _ragged(lengths, 21, pad=float("nan"), layout="plain")
    x[1, :321] = gx[0].to("cuda")
    x[4, :321] = gx[1].to("cuda")
    got = model.score(x, lengths=lengths).cpu().numpy()
    print("ragged golden scores", got[[1, 4]], "fp32 reference", g["t321.mse"][:2])
    np.testing.assert_allclose(got[[1, 4]], g["t321.mse"][:2], rtol=2e-2)


def test_ragged_score_is_five_launches(golden):
    model, _ = _model(golden)
    ctx = _ctx()
    x = _ragged(MIXED, 8)
    model.score(x, lengths=MIXED)
    ctx.timing_reset()
    ctx.timing(True)
    model.score(x, lengths=MIXED)
    ctx.timing(False)
    torch.cuda.synchronize()
    counts = [ctx.timing_read(s)[1] for s in range(8, 16)]
    ctx.timing_reset()
    assert counts == [1, 1, 1, 1, 1, 0, 0, 0], counts


def test_ragged_score_errors(golden):
    from dfa_amd import _lib
    model, _ = _model(golden)
    x = _ragged([40, 24], 13)
    with pytest.raises(ValueError, match=r"lengths\[1\]=15"):
        model.score(x, lengths=[40, 15])
    with pytest.raises(ValueError, match=r"lengths\[0\]=41"):
        model.score(x, lengths=[41, 24])
    with pytest.raises(ValueError, match="3 lengths for a batch of 2"):
        model.score(x, lengths=[40, 24, 24])
    # the C ABI validates on its own, and names the index
    ctx = _ctx()
    model.score(x, lengths=[40, 24])
    ws = ctx.workspace(ctx.lib.dfa_cae_ragged_workspace_bytes(ctx.handle, 2, 40, 180, _lib.PREC_BF16))
    out = torch.empty(2, device="cuda")
    for bad, msg in (([40, 15], b"lengths[1]=15"), ([41, 24], b"lengths[0]=41")):
        lens = np.asarray(bad, dtype=np.int32)
        code = ctx.lib.dfa_cae_score_ragged(ctx.handle, C.c_void_p(x.data_ptr()), _lib.DTYPE_F32, 2, 40, 180, *x.stride(),
                                            C.c_void_p(lens.ctypes.data), None, None, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(ws.data_ptr()), ws.numel())
        assert code == _lib.E_BAD_SHAPE and msg in ctx.lib.dfa_last_error(ctx.handle)
    # non-default kernel options: the uniform forward would run other kernels, the identity would not hold
    for opt in ("cae_dec_fused", "cae_enc1_mfma", "cae_enc_dma", "lds_pipe"):
        ctx.set_option(opt, 0)
        try:
            with pytest.raises(ValueError, match="default options"):
                model.score(x, lengths=[40, 24])
        finally:
            ctx.set_option(opt, 1)
    want = model.score(x, lengths=[40, 24])            # prepared, workspace sized: the capture below launches nothing
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):
        with torch.cuda.graph(g):
            model.score(x, lengths=[40, 24])
    torch.cuda.synchronize()
    assert torch.equal(model.score(x, lengths=[40, 24]), want)
    # an fp32-prepared context fails loudly instead of falling back
    fp32, _ = _model(golden, precision="fp32")
    with pytest.raises(ValueError, match="bf16 only"):
        fp32.score(x, lengths=[40, 24])


# ---------------------------------------------------------------------------------------------------------------- CLIs
def _files(golden, tmp_path, lengths, seed):
    import pandas as pd
    from dfa_amd.dataset_cae import FeatureNormalizer
    n = len(lengths)
    g = torch.Generator().manual_seed(seed)
    labels = [i % 2 for i in range(n)]
    feats = [torch.randn(180, int(T), generator=g) * 3.2 - 0.07 + 0.8 * labels[i] for i, T in enumerate(lengths)]
    uttids = [f"utt_{i:04d}" for i in range(n)]
    paths = {"features": str(tmp_path / "features.pkl"), "labels": str(tmp_path / "labels.pkl"), "norm": str(tmp_path / "normalizer.pt")}
    pd.DataFrame({"uttid": uttids, "features": [f.clone() for f in feats]}).to_pickle(paths["features"])
    pd.DataFrame({"uttid": uttids, "label": labels}).to_pickle(paths["labels"])
    norm = FeatureNormalizer().fit([f.transpose(0, 1) for f in feats])
    norm.save(paths["norm"])
    for name in ("cnn2d", "cnn1d", "cae"):
        sd, _ = golden(f"{name}_eval")
        paths[name] = str(tmp_path / f"{name}.pt")
        torch.save({"model_state": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, paths[name])
    return paths, feats, uttids, labels, norm


def _per_utterance(paths, feats, norm, precision="bf16"):
    """every model on every utterance alone: CNN2D and the auto-encoder through their uniform calls; CNN1D through a ragged
    batch of one (its logit depends on the utterance alone, whatever its length; the uniform CNN1D forward runs other kernels
    for layouts and lengths its one-window kernel does not take)"""
    from dfa_amd.model import CNN2D
    from dfa_amd.model_cae import ConvAutoencoder
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.predict import load_weights
    m2 = load_weights(CNN2D(in_features=180, dropout=0.2, precision=precision).to("cuda"), paths["cnn2d"]).eval()
    m1 = load_weights(CNN1D(in_features=180, dropout=0.2).to("cuda"), paths["cnn1d"]).eval()
    mc = load_weights(ConvAutoencoder(precision=precision).to("cuda"), paths["cae"]).eval()
    mean, std = norm.mean.to("cuda"), norm.std.to("cuda")
    out = {"cnn2d": [], "cnn1d": [], "cae": []}
    with torch.no_grad():
        for f in feats:
            x = f.float().to("cuda")[None].transpose(1, 2)
            out["cnn2d"].append(torch.sigmoid(m2(x).squeeze(-1)))
            T = f.shape[-1]
            own = torch.zeros(1, 180, -(-T // 4) * 4)
            own[0, :, :T] = f.float()
            out["cnn1d"].append(torch.sigmoid(m1(own.to("cuda").transpose(1, 2), lengths=[T]).squeeze(-1)))
            out["cae"].append(mc.score(x, mean, std))
    return {k: torch.cat(v).double().cpu().numpy() for k, v in out.items()}


def test_ragged_clis_end_to_end(golden, tmp_path):
    import pandas as pd
    from dfa_amd import ensemble as ens_cli, fusion, hybrid_ensemble as he_cli, predict_hybrid as ph_cli
    lengths = [400, 16, 321, 47, 170, 31, 333, 64, 17, 250, 96]
    paths, feats, uttids, labels, norm = _files(golden, tmp_path, lengths, 41)
    want = _per_utterance(paths, feats, norm)
    # --- predict_hybrid: the reference schema, input order, scores of per-utterance model calls
    out = str(tmp_path / "prediction_hybrid.pkl")
    common = ["--sup-checkpoint", paths["cnn2d"], "--cae-checkpoint", paths["cae"], "--cae-normalizer", paths["norm"]]
    pred = ph_cli.main(common + ["--test-features", paths["features"], "--alpha", "0.7", "--out", out, "--batch-size", "4",
                                 "--precision", "bf16"])
    got = pd.read_pickle(out)
    assert list(got.columns) == ["uttid", "predictions"] and got["predictions"].dtype == np.float64
    assert got["uttid"].tolist() == uttids and pred["predictions"].equals(got["predictions"])
    np.testing.assert_array_equal(got["predictions"].values, fusion.hybrid_scores(want["cnn2d"], want["cae"], 0.7))
    # --- the same file at fp32: the new argument check, before any model is built (the checkpoints do not even exist)
    with pytest.raises(ValueError, match="--precision bf16 only"):
        ph_cli.main(["--sup-checkpoint", "/nonexistent/a.pt", "--cae-checkpoint", "/nonexistent/b.pt", "--cae-normalizer", "/nonexistent/c.pt",
                     "--test-features", paths["features"], "--out", str(tmp_path / "never.pkl")])
    with pytest.raises(ValueError, match="--precision bf16 only"):
        he_cli.main(["--sup-checkpoint", "/nonexistent/a.pt", "--cae-checkpoint", "/nonexistent/b.pt", "--cae-normalizer", "/nonexistent/c.pt",
                     "--dev-features", paths["features"], "--dev-labels", paths["labels"]])
    with pytest.raises(ValueError, match="--precision bf16 only"):
        ens_cli.main(["--checkpoints", "cnn2d:/nonexistent/a.pt", "cnn1d:/nonexistent/b.pt", "--dev-features", paths["features"],
                      "--dev-labels", paths["labels"]])
    # --- hybrid_ensemble (three members, fixed alpha written to --out) and ensemble
    hout = str(tmp_path / "prediction_he.pkl")
    he_cli.main(common + ["--cnn1d-checkpoint", paths["cnn1d"], "--dev-features", paths["features"], "--dev-labels", paths["labels"],
                          "--batch-size", "5", "--precision", "bf16", "--alpha", "0.6", "--out", hout])
    hgot = pd.read_pickle(hout)
    sup = fusion.ensemble_mean([want["cnn2d"], want["cnn1d"]])
    assert hgot["uttid"].tolist() == uttids
    np.testing.assert_array_equal(hgot["predictions"].values, fusion.hybrid_scores(sup, want["cae"], 0.6))
    res = ens_cli.main(["--checkpoints", f"cnn2d:{paths['cnn2d']}", f"cnn1d:{paths['cnn1d']}", "--dev-features", paths["features"],
                        "--dev-labels", paths["labels"], "--batch-size", "3", "--precision", "bf16"])
    np.testing.assert_array_equal(res["scores"], sup)
    # cnn1d alone takes a ragged file at any precision
    res1 = ens_cli.main(["--checkpoints", f"cnn1d:{paths['cnn1d']}", "--dev-features", paths["features"], "--dev-labels", paths["labels"]])
    np.testing.assert_array_equal(res1["scores"], want["cnn1d"])


def test_equal_length_file_keeps_the_stacked_path(golden, tmp_path):
    """an equal-length file: byte for byte what the stacked path (score_models on the stacked tensor) gives, fp32 included"""
    import pandas as pd
    from dfa_amd import fusion, hybrid_ensemble as he, predict_hybrid as ph_cli
    from dfa_amd.dataset_cae import FeatureNormalizer
    from dfa_amd.model import CNN2D
    from dfa_amd.model_cae import ConvAutoencoder
    paths, feats, uttids, labels, norm = _files(golden, tmp_path, [321] * 9, 43)
    out = str(tmp_path / "prediction_hybrid.pkl")
    calls = []
    real = he.score_models_ragged
    he.score_models_ragged = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        ph_cli.main(["--sup-checkpoint", paths["cnn2d"], "--cae-checkpoint", paths["cae"], "--cae-normalizer", paths["norm"],
                     "--test-features", paths["features"], "--alpha", "0.7", "--out", out, "--batch-size", "4"])
    finally:
        he.score_models_ragged = real
    assert not calls
    df = pd.read_pickle(paths["features"])
    sup = he._load(CNN2D, paths["cnn2d"], "cuda", in_features=180, dropout=0.2, precision="fp32")
    cae = he._load(ConvAutoencoder, paths["cae"], "cuda", precision="fp32")
    local = he.score_models(he._stack(df), sup, None, cae, FeatureNormalizer.load(paths["norm"]), 4, "cuda", 0, 1)
    want = fusion.hybrid_scores(local["cnn2d"], local["cae"], 0.7).astype(np.float64)
    assert pd.read_pickle(out)["predictions"].values.tobytes() == want.tobytes()
