"""Variable-length (ragged) CNN2D batches on the GPU (dfa_cnn2d_forward_ragged, bf16 precision).

Utterance b of a ragged batch must get what the uniform forward gives x[b:b+1, :T_b] alone, bit for bit: the ragged kernels
take their loop bounds, row masks, canonical time-mean chunks and 1/H2 from T_b, and the uniform path is bit-invariant to the
batch size and to the time split (test_parity_r2_gpu.py::test_time_axis_split_is_bit_invariant)."""
import numpy as np
import pytest
import torch

from oracle import dfa_oracle as O

pytestmark = pytest.mark.gpu

TOL_BF16_EMU_REL = 1e-3          # as tests/test_parity_r2_gpu.py: bf16 mode against the rounding-faithful oracle
LENGTHS = [4, 5, 6, 7, 37, 64, 130, 321, 322, 641]     # every T mod 4, both sides of the dataset's 321
PATTERNS = [0xFFFF, 0x7FC0, 0x7F80]                     # as tests/test_lds_poison_gpu.py


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _model(golden, precision="bf16"):
    from dfa_amd.model import CNN2D
    sd, _ = golden("cnn2d_eval")
    m = CNN2D(precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to("cuda").eval(), sd


def _ragged(lengths, seed, F=180, pad=0.0, dtype=torch.float32):
    """stored [B, F, T_max] features (the reference's layout), padding columns filled with `pad`; returns the strided
    [B, T_max, F] view and the per-utterance stored arrays"""
    gen = torch.Generator().manual_seed(seed)
    T_max = max(lengths)
    stored = torch.full((len(lengths), F, T_max), pad)
    parts = []
    for i, T in enumerate(lengths):
        u = torch.randn(F, T, generator=gen) * 3.2 - 0.07
        stored[i, :, :T] = u
        parts.append(u.numpy())
    return stored.to(dtype).to("cuda").transpose(1, 2), parts


def _uniform_each(model, x, lengths):
    """the uniform forward of every utterance alone, at its own length"""
    outs = [model(x[i:i + 1, :T], return_embedding=True) for i, T in enumerate(lengths)]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def test_ragged_matches_rounding_faithful_oracle_per_utterance(golden):
    model, sd = _model(golden)
    x, parts = _ragged(LENGTHS, 7)
    logits, emb = model(x, return_embedding=True, lengths=LENGTHS)
    for i, u in enumerate(parts):
        want, inter = O.cnn2d_forward(sd, u.T[None], return_intermediates=True, emulate="bf16")
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(logits[i:i + 1].cpu().numpy(), want, atol=TOL_BF16_EMU_REL * scale, rtol=0, err_msg=str(LENGTHS[i]))
        e = inter["embedding"]
        np.testing.assert_allclose(emb[i:i + 1].cpu().numpy(), e, atol=2e-3 * max(1.0, float(np.abs(e).max())), rtol=0,
                                   err_msg=str(LENGTHS[i]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_is_bit_identical_to_the_uniform_path(golden, dtype):
    model, _ = _model(golden)
    ctx = _ctx()
    x, _ = _ragged(LENGTHS, 8, dtype=dtype)
    try:
        ctx.set_option("time_split", 0)
        want_l, want_e = _uniform_each(model, x, LENGTHS)
        for split in (-1, 0, 2, 5):
            ctx.set_option("time_split", split)
            l, e = model(x, return_embedding=True, lengths=LENGTHS)
            assert torch.equal(l, want_l), (split, float((l - want_l).abs().max()))
            assert torch.equal(e, want_e), (split, float((e - want_e).abs().max()))
            assert torch.equal(model(x, lengths=torch.tensor(LENGTHS, device="cuda")), want_l), split
    finally:
        ctx.set_option("time_split", -1)


def test_equal_lengths_ragged_equals_uniform_call(golden):
    model, _ = _model(golden)
    x, _ = _ragged([321] * 6, 9)
    want = model(x, return_embedding=True)
    got = model(x, return_embedding=True, lengths=np.full(6, 321))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_ragged_full_size_batch_bit_identical_per_length_group(golden):
    """B = 256, lengths uniform in [161, 481] (mean 321): no time split, longest-first order dealt over the 8 XCDs."""
    model, _ = _model(golden)
    rng = np.random.default_rng(2024)
    lengths = rng.integers(161, 482, size=256).tolist()
    x, _ = _ragged(lengths, 10, dtype=torch.bfloat16)
    l, e = model(x, return_embedding=True, lengths=lengths)
    arr = np.asarray(lengths)
    for T in np.unique(arr):
        idx = torch.from_numpy(np.nonzero(arr == T)[0]).to("cuda")
        wl, we = model(x.index_select(0, idx)[:, :int(T)], return_embedding=True)
        assert torch.equal(l.index_select(0, idx), wl), int(T)
        assert torch.equal(e.index_select(0, idx), we), int(T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pad", [float("nan"), 3.0e38, -1.0e4])
def test_padding_rows_are_never_read(golden, pad, dtype):
    model, _ = _model(golden)
    x0, _ = _ragged(LENGTHS, 11, pad=0.0, dtype=dtype)
    x1, _ = _ragged(LENGTHS, 11, pad=pad, dtype=dtype)
    want = model(x0, return_embedding=True, lengths=LENGTHS)
    got = model(x1, return_embedding=True, lengths=LENGTHS)
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_ragged_ignores_stale_lds(golden):
    model, _ = _model(golden)
    ctx = _ctx()
    x, _ = _ragged(LENGTHS, 12, dtype=torch.bfloat16)
    try:
        for split in (-1, 0):
            ctx.set_option("time_split", split)
            want = [t.clone() for t in model(x, return_embedding=True, lengths=LENGTHS)]
            for pat in PATTERNS:
                ctx.set_option("poison_lds", pat)
                got = model(x, return_embedding=True, lengths=LENGTHS)
                assert torch.isfinite(got[0]).all()
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (split, hex(pat))
    finally:
        ctx.set_option("time_split", -1)


def test_ragged_errors(golden):
    import ctypes as C
    from dfa_amd import _lib
    model, _ = _model(golden)
    x, _ = _ragged([8, 6], 13)
    with pytest.raises(ValueError, match=r"lengths\[1\]=3"):
        model(x, lengths=[8, 3])
    with pytest.raises(ValueError, match=r"lengths\[0\]=9"):
        model(x, lengths=[9, 6])
    with pytest.raises(ValueError, match="3 lengths for a batch of 2"):
        model(x, lengths=[8, 6, 6])
    model.train()
    with pytest.raises(NotImplementedError):
        model(x, lengths=[8, 6])
    model.eval()
    # the C ABI validates on its own, and names the index
    ctx = _ctx()
    ws = ctx.workspace(ctx.lib.dfa_ragged_workspace_bytes(ctx.handle, _lib.MODEL_CNN2D, 2, 8, 180, _lib.PREC_BF16))
    out = torch.empty(2, device="cuda")
    for bad, msg in (([8, 2], b"lengths[1]=2"), ([10, 6], b"lengths[0]=10")):
        lens = np.asarray(bad, dtype=np.int32)
        code = ctx.lib.dfa_cnn2d_forward_ragged(ctx.handle, C.c_void_p(x.data_ptr()), _lib.DTYPE_F32, 2, 8, 180, *x.stride(),
                                                C.c_void_p(lens.ctypes.data), C.c_void_p(out.data_ptr()), None,
                                                C.c_void_p(ws.data_ptr()), ws.numel())
        assert code == _lib.E_BAD_SHAPE and msg in ctx.lib.dfa_last_error(ctx.handle)
    # non-default kernel options (the uniform forward would run other kernels) and graph capture are refused
    for opt in ("fuse_conv1", "block3_m16"):
        ctx.set_option(opt, 0)
        try:
            with pytest.raises(ValueError, match="default options"):
                model(x, lengths=[8, 6])
        finally:
            ctx.set_option(opt, 1)
    model(x, lengths=[8, 6])                    # prepared, workspace sized: the capture below launches nothing
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):
        with torch.cuda.graph(g):
            model(x, lengths=[8, 6])
    torch.cuda.synchronize()
    # precisions without ragged kernels fail loudly instead of falling back
    with pytest.raises(ValueError, match="bf16 only"):
        model.set_precision("fp32")(x, lengths=[8, 6])


def test_ragged_batcher_end_to_end(golden):
    """features.pkl-style list of [F, T_i] tensors -> RaggedBatcher -> ragged forward -> input order; equals the uniform
    forward of each utterance alone"""
    from dfa_amd.dataloaders import RaggedBatcher
    model, _ = _model(golden)
    gen = torch.Generator().manual_seed(17)
    feats = [torch.randn(180, int(t), generator=gen) for t in np.random.default_rng(5).integers(4, 500, size=37)]
    b = RaggedBatcher(feats, None, batch_size=8, device="cuda", dtype=torch.bfloat16)
    got = b.restore([model(x, lengths=lengths) for x, _, lengths in b])
    want = torch.cat([model(f.to(torch.bfloat16).to("cuda")[None].transpose(1, 2)) for f in feats])
    assert torch.equal(got, want)
