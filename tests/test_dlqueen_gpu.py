"""DeepfakeDetector (Conv1d + StatsPool) eval forward on the GPU (dfa_dlq_forward: three matrix-core layer launches over a tile
list + the pool / head kernel) and `python -m dfa_amd.dlqueen_model`.

Promises: (1) parity with the float64 statement of the model (tests/dlqueen_oracle.py, pinned to the reference by
tests/test_dlqueen_cpu.py) within 2^-17 * S for logits, S = max |logit64| of the fixture, and 2^-17 * max |pooled64| for the
pooled vectors, rtol 0 -- 2^-17 is the representation error of one hi + lo bf16 operand; the kernels carry three bf16 terms per
operand (fp32 grade), for which a float64 emulation of the arithmetic gives 1.8e-7 * S and the reference's own fp32 forward is
7.3e-7 * S from float64; (2) logit[b] is bit for bit a function of (x[b, :, :len], len, min(T - len, 2)): not of the batch, the
position in it, T, the padding's contents, the workspace's contents or what LDS held.

Every case prints its measured maxima before it asserts (run with -s); tools/gpu_dlqueen_bench.py --parity prints the padded
batch's.  Measured on an MI355X: padded batch 1.16e-6 S (pooled 4.1e-7 of max), alone 1.16e-6 S (2.9e-7), one frame of padding
1.03e-6 S (3.8e-7)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dlqueen_oracle as DO

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -17
N = 64                                                   # the kernel's frame tile (asserted against the module below)
PATTERNS = [0xFFFF, 0x7FC0, 0x7F80]                      # as tests/test_lds_poison_gpu.py


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


@pytest.fixture(scope="module")
def fx(golden):
    from dfa_amd import dlqueen_model as M
    assert M.TILE_FRAMES == N
    _, g = golden("dlqueen_eval")
    sd = DO.fixture_state_dict(g, M.DeepfakeDetector)
    m = M.DeepfakeDetector(180)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda").eval(), g, sd, DO.split_utts(g)


def _batch(utts, T=None, fill=0.0, order=None):
    order = list(range(len(utts))) if order is None else order
    x, lengths = DO.pad_batch([utts[i] for i in order], T, fill=fill)
    base = x._base if x._base is not None else x
    return base.to("cuda")[:, :, :x.shape[2]], lengths


def _check(got_logits, got_pooled, want_logits, want_pooled, S, what):
    el = float(np.abs(got_logits.double().cpu().numpy() - want_logits).max())
    pm = float(np.abs(want_pooled).max())
    ep = float(np.abs(got_pooled.double().cpu().numpy() - want_pooled).max())
    print(f"{what}: logits max|gpu - f64| = {el:.3e} = {el / S:.3e} S (bound {TOL:.3e} S); pooled {ep:.3e} = {ep / pm:.3e} of max {pm:.3f}")
    assert el <= TOL * S, (what, el / S)
    assert ep <= TOL * pm, (what, ep / pm)


def test_parity_with_the_fixture(fx):
    model, g, _, utts = fx
    S = float(g["S"])
    x, lengths = _batch(utts)
    assert x.shape == (13, 180, 321)
    lg, pooled = model(x, lengths, return_pooled=True)
    assert lg.shape == (13,) and pooled.shape == (13, 512) and lg.dtype == torch.float32
    _check(lg, pooled, g["batch.logits64"], g["batch.pooled64"], S, "batch padded to 321")
    assert torch.equal(model(x, lengths), lg)
    for tag, extra in (("alone", 0), ("pad1", 1)):
        outs = [model(*_batch([u], u.shape[-1] + extra), return_pooled=True) for u in utts]
        _check(torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), g[tag + ".logits64"], g[tag + ".pooled64"], S, tag)
    assert torch.equal(pooled[0, 256:], torch.full((256,), 1e-3, device="cuda"))       # len = 1: the clamp, exactly


def test_parity_around_the_frame_tile(fx):
    model, g, sd, _ = fx
    S = float(g["S"])
    gen = torch.Generator().manual_seed(21)
    for n in (N - 1, N, N + 1, 2 * N + 1):
        u = ((3.2 * torch.randn(180, n, generator=gen) - 0.07).clamp(-61.0, 87.0)).numpy()
        for pad in (0, 1, 2, 3):
            x, lengths = DO.pad_batch([u], n + pad)
            want_l, want_p = DO.forward(sd, x, lengths)
            lg, pooled = model(*_batch([u], n + pad), return_pooled=True)
            _check(lg, pooled, want_l, want_p, S, f"len {n} padding {pad}")


def test_logit_is_a_function_of_the_utterance_alone(fx):
    model, _, _, utts = fx
    ctx = _ctx()
    alone = [model(*_batch([u], u.shape[-1] + 2), return_pooled=True) for u in utts]
    want_l, want_p = torch.cat([a[0] for a in alone]), torch.cat([a[1] for a in alone])
    T = 323                                               # every utterance has >= 2 frames of padding

    def same(x, lengths, order=None, what=""):
        lg, pooled = model(x, lengths, return_pooled=True)
        idx = torch.arange(13) if order is None else torch.tensor(order)
        assert torch.isfinite(lg).all(), what
        assert torch.equal(lg, want_l[idx.to("cuda")]) and torch.equal(pooled, want_p[idx.to("cuda")]), what

    x, lengths = _batch(utts, T)
    same(x, lengths, what="mixed batch")
    rev = list(range(12, -1, -1))
    same(*_batch(utts, T, order=rev), order=rev, what="reversed")
    same(*_batch(utts, T + 64), what="T_max + 64")
    for fill in (float("nan"), float("inf"), 3e38):
        same(*_batch(utts, T, fill=fill), what=f"padding {fill}")
    ws = ctx.workspace(ctx.lib.dfa_dlq_workspace_bytes(ctx.handle, 13, T, 180))
    ws.fill_(0xFF)                                        # NaN in every activation slot
    same(x, lengths, what="workspace of NaN bytes")
    for pat in PATTERNS:
        ctx.set_option("poison_lds", pat)
        same(x, lengths, what=f"poison_lds {pat:#x}")
    a = model(*_batch(utts[:6], T))
    b = model(*_batch(utts[6:], T))
    assert torch.equal(torch.cat([a, b]), want_l)         # B = 13 == B = 6 then B = 7


def test_other_layouts_and_dtypes_are_copied(fx):
    model, g, sd, utts = fx
    S = float(g["S"])
    sub = [torch.from_numpy(u).bfloat16().float().numpy() for u in utts[3:11]]      # bf16-representable values
    x, lengths = _batch(sub)
    want = model(x, lengths)
    want_l, want_p = DO.forward(sd, *DO.pad_batch(sub))
    btc = x.transpose(1, 2).contiguous().transpose(1, 2)  # a (B, T, C) tensor seen as (B, C, T): stride_t = C
    assert btc.stride(2) == 180
    lg, pooled = model(btc, lengths, return_pooled=True)
    assert torch.equal(lg, want)
    _check(lg, pooled, want_l, want_p, S, "(B, T, C)-strided view")
    lg, pooled = model(x.to(torch.bfloat16), lengths, return_pooled=True)
    assert torch.equal(lg, want)
    _check(lg, pooled, want_l, want_p, S, "bf16 input")
    odd = x[:, :, :63]                                    # rows that end off a 16-byte boundary, lengths cut to fit
    lens = [min(n, 63) for n in lengths]
    assert torch.equal(model(odd, lens), model(odd.contiguous(), lens))


def test_refusals_name_their_cause_and_leave_the_context_usable(fx):
    from dfa_amd import _lib
    from dfa_amd.dlqueen_model import DeepfakeDetector
    model, _, _, utts = fx
    ctx = _ctx()
    x, lengths = _batch(utts[4:8], 36)                    # lengths 5, 31, 32, 33
    want = model(x, lengths).clone()
    with pytest.raises(ValueError, match=r"lengths\[1\]=0"):
        model(x, [5, 0, 32, 33])
    with pytest.raises(ValueError, match=r"lengths\[2\]=37"):
        model(x, [5, 31, 37, 33])
    with pytest.raises(ValueError, match="3 lengths for a batch of 4"):
        model(x, [5, 31, 32])
    with pytest.raises(ValueError, match="hidden=256"):
        DeepfakeDetector(180, hidden=128).to("cuda").eval()(x, lengths)
    with pytest.raises(ValueError, match="in_ch=182"):
        DeepfakeDetector(182).to("cuda").eval()(torch.zeros(1, 182, 8, device="cuda"), [8])
    assert torch.equal(model(x, lengths), want)           # the fixture's model binds its weights again

    # the C ABI directly
    need = ctx.lib.dfa_dlq_workspace_bytes(ctx.handle, 4, 36, 180)
    ws = ctx.workspace(need + 256)
    out = torch.zeros(4, device="cuda")
    host = np.asarray(lengths, dtype=np.int32)

    def call(ws_ptr, ws_bytes, lens=host):
        sb, sc, _ = x.stride()
        return ctx.lib.dfa_dlq_forward(ctx.handle, C.c_void_p(x.data_ptr()), 4, 36, 180, sb, sc, C.c_void_p(lens.ctypes.data),
                                       C.c_void_p(out.data_ptr()), None, C.c_void_p(ws_ptr), ws_bytes)

    err = lambda: ctx.lib.dfa_last_error(ctx.handle)     # noqa: E731
    assert call(ws.data_ptr(), need - 1) == _lib.E_WORKSPACE and b"too small" in err()
    assert call(ws.data_ptr() + 16, need) == _lib.E_WORKSPACE and b"aligned" in err()
    assert call(ws.data_ptr(), need, np.array([5, 31, 0, 33], dtype=np.int32)) == _lib.E_BAD_SHAPE and b"lengths[2]=0" in err()
    sb, sc, _ = x.stride()
    assert ctx.lib.dfa_dlq_forward(ctx.handle, C.c_void_p(x.data_ptr() + 4), 4, 36, 180, sb, sc, C.c_void_p(host.ctypes.data),
                                   C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), need) == _lib.E_UNSUPPORTED
    assert b"16-byte" in err()
    # forward before prepare: set_params alone invalidates the preparation
    arr = _lib.ptr_array([t.detach() for t in model._abi_tensors()])
    assert ctx.lib.dfa_dlq_set_params(ctx.handle, arr, 22, 180, 256) == _lib.DFA_OK
    assert call(ws.data_ptr(), need) == _lib.E_NOT_PREPARED and b"dfa_dlq_prepare" in err()
    assert ctx.lib.dfa_dlq_set_params(ctx.handle, arr, 21, 180, 256) == _lib.E_BAD_SHAPE
    assert ctx.lib.dfa_dlq_prepare(ctx.handle) == _lib.DFA_OK
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                  # nothing ran
    assert call(ws.data_ptr(), need) == _lib.DFA_OK
    assert torch.equal(out, want)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):
        with torch.cuda.graph(g):
            model(x, lengths)
    torch.cuda.synchronize()
    assert torch.equal(model(x, lengths), want)           # the stream is usable afterwards


def test_cli_end_to_end(fx, tmp_path, capsys):
    import pandas as pd
    from dfa_amd import dlqueen_model as M
    model, _, sd, _ = fx
    gen = torch.Generator().manual_seed(8)
    lens = [int(v) for v in torch.randint(1, 140, (24,), generator=gen)]
    feats = [(3.2 * torch.randn(180, n, generator=gen) - 0.07) for n in lens]
    uttids = [f"utt_{i:03d}" for i in range(24)]
    split = tmp_path / "data" / "dev"
    os.makedirs(split)
    pd.DataFrame({"uttid": uttids, "features": feats}).to_pickle(split / "features.pkl")
    pd.DataFrame({"uttid": uttids[::-1], "label": [(i * 7) % 3 == 0 for i in range(24)][::-1]}).astype({"label": int}).to_pickle(split / "labels.pkl")
    ckpt, out = str(tmp_path / "best_model.pth"), str(tmp_path / "prediction.pkl")
    torch.save(sd, ckpt)
    argv = ["--data_dir", str(tmp_path / "data"), "--test_split", "dev", "--ckpt_path", ckpt, "--prediction_pkl", out, "--batch_size", "7"]
    M.main(argv)
    text = capsys.readouterr().out
    pred = pd.read_pickle(out)
    assert list(pred.columns) == ["uttid", "predictions"] and pred["uttid"].tolist() == uttids
    assert pred["predictions"].dtype == np.float64
    direct = M.run_inference(model, feats, batch_size=7)
    np.testing.assert_array_equal(pred["predictions"].to_numpy(), direct.double().cpu().numpy())
    # each score is the utterance's own logit in its padding class: batches of 7, longest first, padded to the batch's longest
    order = np.argsort(-np.array(lens), kind="stable")
    by_hand = torch.empty(24, device="cuda")
    for lo in range(0, 24, 7):
        idx = order[lo:lo + 7]
        for i in idx:
            by_hand[i] = model(*_batch([feats[i].numpy()], lens[i] + min(lens[idx[0]] - lens[i], 2)))[0]
    assert torch.equal(by_hand, direct)
    from dfa_amd.evaluation import calculate_eer
    labels = [int((i * 7) % 3 == 0) for i in range(24)]
    eer, _ = calculate_eer(direct.double().cpu().numpy(), np.array(labels))
    assert f"EER on split 'dev': {eer:.6f}" in text
    M.main(argv + ["--use_prob", "--file-order"])
    prob = pd.read_pickle(out)["predictions"].to_numpy()
    in_order = M.run_inference(model, feats, batch_size=7, file_order=True)
    np.testing.assert_array_equal(prob, torch.sigmoid(in_order).double().cpu().numpy())
    assert ((prob > 0) & (prob < 1)).all()
