"""GPU tests of the k = (5, 3, 3) CNN1D variant's eval forward (cnn1d_fused_x3_k5_kernel / cnn1d_ragged_x3_k5_kernel, the
five-tap conv1d.hip kernel of the three-launch path) against the float64 oracle of tests/cnn1d_k5_oracle.py.

Bounds: every logit within 1e-4 of the oracle -- the bar tests/test_cnn1d_gpu.py holds every three-tap CNN1D kernel to (TOL_F32);
a ragged logit is bit-identical to the uniform forward of that utterance alone wherever the uniform one-kernel form takes the
length, as tests/test_cnn1d_ragged_gpu.py holds for three taps, and within 1e-4 of it beyond."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import cnn1d_k5_oracle as KO
import utt_norm_oracle as UO

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4                    # tests/test_cnn1d_gpu.py
K5 = (5, 3, 3)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_CKPT = os.path.join(GOLDEN, "ref_cnn1d_k533_checkpoint.pt")


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _model(sd, kernels=K5):
    from dfa_amd.model_cnn1d import CNN1D
    m = CNN1D(in_features=int(np.asarray(sd["conv.0.weight"]).shape[1]), kernels=kernels)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to("cuda").eval()


def _max_t(F):
    """the longest T the one-kernel form takes, as the library computes it (the bound of cnn1d_fused_x3_supports)"""
    from dfa_amd import _lib
    return _lib.load().dfa_cnn1d_fused_max_t(F, 5)


@functools.lru_cache(maxsize=None)
def _state(F):
    """asymmetric across taps: a reversed or shifted tap order moves every logit"""
    return KO.asymmetric_state(F, K5, seed=F)


@functools.lru_cache(maxsize=None)
def _model_f(F):
    return _model(_state(F))


def _slot_counts(ctx, fn):
    ctx.timing_reset()
    ctx.timing(True)
    out = fn()
    ctx.timing(False)
    torch.cuda.synchronize()
    counts = [ctx.timing_read(s)[1] for s in (4, 5, 6, 7)]
    ctx.timing_reset()
    return out, counts


def _t_cases(F):
    cap = _max_t(F)
    return [3, 4, 5, 31, 32, 33, 64, 65, 257, 321, cap, cap + 1]


@pytest.mark.parametrize("F", [180, 20, 4])
@pytest.mark.parametrize("ti", range(12))
def test_uniform_forward_matches_oracle_in_every_form(F, ti):
    """B = 3 at T in {3, 4, 5, 31, 32, 33, 64, 65, 257, 321, the one-kernel form's limit, limit + 1}: the default form (ONE launch
    for the stored layout up to the limit, the three launches past it), the three-launch path forced, and a contiguous [B, T, F]
    input (the fallback layout) -- all within 1e-4 of the float64 oracle and of each other.  F = 20: a short second slab (4 of its
    16 channels); F = 4: one real k-step, an odd count padded to even with a zero slab."""
    T = _t_cases(F)[ti]
    sd, m, ctx = _state(F), _model_f(F), _ctx()
    stored = np.stack(KO.utterances([T] * 3, 1000 * F + T, F))
    want = KO.forward(sd, stored.swapaxes(1, 2))
    x = torch.from_numpy(stored).to("cuda").transpose(1, 2)
    got, counts = _slot_counts(ctx, lambda: m(x).cpu().numpy())
    assert counts == ([1, 0, 0, 0] if T <= _max_t(F) else [1, 1, 1, 1]), (T, counts)
    try:
        ctx.set_option("cnn1d_fused", 0)
        three, counts3 = _slot_counts(ctx, lambda: m(x).cpu().numpy())
    finally:
        ctx.set_option("cnn1d_fused", 1)
    assert counts3 == [1, 1, 1, 1]
    btf, counts_c = _slot_counts(ctx, lambda: m(x.contiguous()).cpu().numpy())
    assert counts_c == [1, 1, 1, 1]              # (the exact-fp32 one-kernel form refuses five taps: the three launches)
    errs = [float(np.abs(v - want).max()) for v in (got, three, btf)]
    print(f"[cnn1d k5 T={T} F={F}] max |logit| {np.abs(want).max():.2f}; |one kernel - oracle| {errs[0]:.2e}, |three launches - oracle| "
          f"{errs[1]:.2e}, |contiguous - oracle| {errs[2]:.2e}, |one kernel - three launches| {np.abs(got - three).max():.2e}")
    assert np.isfinite(got).all()
    assert max(errs) <= TOL_F32, errs
    assert float(np.abs(got - three).max()) <= TOL_F32
    np.testing.assert_array_equal(btf, three)     # the same kernels through other strides


def test_reference_fixture_logits(golden):
    sd, g = golden("cnn1d_k533_eval")
    m = _model(sd)
    got = m(torch.from_numpy(g["x"]).to("cuda")).cpu().numpy()                                       # [B, T, F] contiguous
    got_s = m(torch.from_numpy(g["x"].swapaxes(1, 2).copy()).to("cuda").transpose(1, 2)).cpu().numpy()   # the stored layout: one kernel
    np.testing.assert_allclose(got, g["logits"], atol=TOL_F32, rtol=0)
    np.testing.assert_allclose(got_s, g["logits"], atol=TOL_F32, rtol=0)


def test_one_launch_and_batch_independence():
    m, ctx = _model_f(180), _ctx()
    x = torch.from_numpy(np.stack(KO.utterances([321] * 7, 11))).to("cuda").transpose(1, 2)
    full, counts = _slot_counts(ctx, lambda: m(x))
    assert counts == [1, 0, 0, 0], counts
    for i in (0, 3, 6):
        assert torch.equal(m(x[i:i + 1]), full[i:i + 1])


# ------------------------------------------------------------------------------------------------ ragged
RAGGED = [3, 4, 5, 33, 321, 500]          # 500 > the 384-frame window: two segments


def _pad(utts, pad=float("nan"), order=None):
    order = list(range(len(utts))) if order is None else order
    lengths = [int(utts[i].shape[1]) for i in order]
    T_max = max(lengths)
    stored = torch.full((len(order), utts[0].shape[0], -(-T_max // 4) * 4), pad)
    for j, i in enumerate(order):
        stored[j, :, :lengths[j]] = torch.from_numpy(utts[i])
    return stored.to("cuda").transpose(1, 2)[:, :T_max], lengths


def test_ragged_forward_nan_padding_every_utterance_alone():
    from dfa_amd import _lib
    sd, m = _state(180), _model_f(180)
    assert _lib.load().dfa_cnn1d_ragged_segments_k(500, 180, 5, None, None, None, None, 0) == 2
    utts = KO.utterances(RAGGED, 77)
    x, lengths = _pad(utts)
    got, counts = _slot_counts(_ctx(), lambda: m(x, lengths=lengths))
    assert counts == [1, 0, 0, 0], counts
    assert torch.isfinite(got).all()
    want = KO.forward_ragged(sd, utts)
    for i, u in enumerate(utts):
        alone = m(torch.from_numpy(u).to("cuda")[None].transpose(1, 2))
        err = float(np.abs(got[i].cpu().numpy() - want[i]).max())
        print(f"[cnn1d k5 ragged T={RAGGED[i]}] logit {float(got[i, 0]):.6f} oracle {want[i, 0]:.6f} |diff| {err:.2e}")
        assert err <= TOL_F32, (RAGGED[i], err)
        if RAGGED[i] <= _max_t(180):
            assert torch.equal(got[i:i + 1], alone), RAGGED[i]           # one window: the uniform kernel's own arithmetic
        else:
            np.testing.assert_allclose(got[i:i + 1].cpu().numpy(), alone.cpu().numpy(), atol=TOL_F32, rtol=0)
    perm = [4, 0, 5, 2, 1, 3]
    xp, lp = _pad(utts, order=perm)
    assert torch.equal(m(xp, lengths=lp), got[perm])
    x0, _ = _pad(utts, pad=0.0)
    assert torch.equal(m(x0, lengths=lengths), got)                       # the padding is never used


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(golden):
    from dfa_amd import _lib
    ctx = _ctx()
    lib, h = ctx.lib, ctx.handle
    m5 = _model_f(180)
    x = torch.from_numpy(np.stack(KO.utterances([33] * 2, 5))).to("cuda").transpose(1, 2)
    want5 = m5(x).clone()
    # an unsupported set: refused with a message, the context keeps its (5, 3, 3) model
    assert lib.dfa_cnn1d_set_kernels(h, 3, 5, 3) == _lib.E_UNSUPPORTED
    msg = lib.dfa_last_error(h)
    assert b"(3, 5, 3)" in msg and b"(5, 3, 3)" in msg
    assert torch.equal(m5(x), want5)
    # the five-tap RAGGED training forward: refused before anything is launched, logits untouched (the uniform step exists:
    # tests/test_cnn1d_k5_train_gpu.py)
    ws = ctx.workspace(lib.dfa_cnn1d_train_workspace_bytes(h, 2, 33, 180) + 4096)
    out = torch.full((2,), 7.0, device="cuda")
    head = (h, C.c_void_p(x.data_ptr()), _lib.DTYPE_F32, 2, 33, 180, *x.stride())
    tail = (0.0, 1, 0, 0.1, 1, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel())
    lens = np.asarray([33, 20], dtype=np.int32)
    assert lib.dfa_cnn1d_forward_train_ragged(*head, C.c_void_p(lens.ctypes.data), *tail) == _lib.E_UNSUPPORTED
    assert b"(3, 3, 3)" in lib.dfa_last_error(h) and b"(5, 3, 3)" in lib.dfa_last_error(h)
    assert lib.dfa_cnn1d_train_ragged_workspace_bytes(h, 2, 33, 180) == 0
    assert lib.dfa_cnn1d_train_plan(h, 2, 33, 180, 1, None, 0) == _lib.E_UNSUPPORTED and b"(5, 3, 3)" in lib.dfa_last_error(h)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((2,), 7.0, device="cuda"))
    # after a (5, 3, 3) model, a (3, 3, 3) model on the same context still reproduces cnn1d_eval.npz -- and the other way round
    sd3, g3 = golden("cnn1d_eval")
    m3 = _model(sd3, (3, 3, 3))
    stored = torch.from_numpy(g3["t64.x_stored"]).to("cuda")
    np.testing.assert_allclose(m3(stored.transpose(1, 2)).cpu().numpy(), g3["t64.logits"], atol=TOL_F32, rtol=0)
    assert torch.equal(m5(x), want5)
    np.testing.assert_allclose(m3(stored.transpose(1, 2)).cpu().numpy(), g3["t64.logits"], atol=TOL_F32, rtol=0)


def test_kernels_flag_with_cnn2d_is_refused(tmp_path):
    from dfa_amd import predict
    missing = str(tmp_path / "nothing.pkl")
    with pytest.raises(ValueError, match="--model cnn1d"):
        predict.main(["--features", missing, "--checkpoint", missing, "--model", "cnn2d", "--out", missing, "--kernels", "5,3,3"])


# ------------------------------------------------------------------------------------------------ end to end
def test_predict_scores_the_reference_written_checkpoint(golden, tmp_path):
    """no --kernels, no --norm: both come from the file src/compare_kernels.py:178-184 writes (kernels (5, 3, 3), norm_mode cmn).
    Bound on a score: the logit's 1e-4 through the sigmoid (slope <= 1/4), doubled for the float32 CMN in front of the model (its
    own bound, tests/utt_norm_oracle.row_bound, is ~1e-6 of a feature): 5e-5."""
    import pandas as pd
    from dfa_amd import predict
    sd, _ = golden("cnn1d_k533_eval")
    utts = KO.utterances([321] * 5, 99)
    path, out = str(tmp_path / "features.pkl"), str(tmp_path / "prediction.pkl")
    pd.DataFrame({"uttid": [f"utt{i}" for i in range(5)], "features": [torch.from_numpy(u) for u in utts]}).to_pickle(path)
    predict.main(["--features", path, "--checkpoint", REF_CKPT, "--model", "cnn1d", "--out", out])
    pred = pd.read_pickle(out)
    assert list(pred["uttid"]) == [f"utt{i}" for i in range(5)]
    logits = KO.forward(sd, np.stack([UO.normalize(u, "cmn").T for u in utts]))[:, 0]
    want = 1.0 / (1.0 + np.exp(-logits))
    err = np.abs(np.asarray(pred["predictions"], dtype=np.float64) - want)
    print(f"[cnn1d k5 predict] scores {list(pred['predictions'])} max |score - oracle| {err.max():.2e}")
    assert err.max() <= 5e-5
