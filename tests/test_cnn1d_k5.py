"""CPU tests of the k = (5, 3, 3) CNN1D variant (the reference's CNN1D_Variant, src/compare_kernels.py:38-67): the module
surface, the checkpoint key, the float64 oracle against the reference's own results, the `--kernels` flag and the segment plan
of the five-tap ragged kernel.  Nothing here launches a kernel."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import cnn1d_k5_oracle as KO
from dfa_amd import _lib
from dfa_amd.model_cnn1d import CNN1D, resolve_kernels
from dfa_amd.training import checkpoint_blob

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_CKPT = os.path.join(GOLDEN, "ref_cnn1d_k533_checkpoint.pt")


def test_variant_exists_with_the_reference_layout(golden):
    sd, _ = golden("cnn1d_k533_eval")
    m = CNN1D(kernels=(5, 3, 3))
    mine = m.state_dict()
    assert list(mine.keys()) == list(sd.keys())               # same keys in the same order as CNN1D_Variant(kernels=(5, 3, 3))
    for k, v in sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    assert tuple(mine["conv.0.weight"].shape) == (32, 180, 5)
    assert m.kernels == (5, 3, 3) and CNN1D().kernels == (3, 3, 3)
    assert tuple(CNN1D().state_dict()["conv.0.weight"].shape) == (32, 180, 3)
    assert [n for n, _ in m.named_parameters()] == list(KO.GRAD_KEYS)


def test_seeded_init_is_bit_identical_to_the_reference(golden):
    """make_golden_cnn1d_k533.py built the reference's variant under torch.manual_seed(533) and left its conv parameters alone"""
    sd, g = golden("cnn1d_k533_eval")
    torch.manual_seed(533)
    mine = CNN1D(dropout=0.0, kernels=(5, 3, 3)).state_dict()
    for k in ("conv.0.weight", "conv.0.bias", "conv.4.weight", "conv.4.bias", "conv.8.weight", "conv.8.bias", "classifier.bias"):
        np.testing.assert_array_equal(mine[k].numpy(), sd[k], err_msg=k)
    np.testing.assert_array_equal(mine["classifier.weight"].numpy(), g["init.classifier.weight"])


@pytest.mark.parametrize("kernels", [(3, 5, 3), (7, 3, 3), (5, 3)])
def test_other_kernel_sets_are_refused_by_name(kernels):
    with pytest.raises(ValueError, match=r"\(3, 3, 3\).*\(5, 3, 3\)"):
        CNN1D(kernels=kernels)


def test_oracle_reproduces_the_reference(golden):
    """pins tests/cnn1d_k5_oracle.py to the reference's float32 module: eval logits, train-mode logits, loss, all 14 gradients"""
    sd, g = golden("cnn1d_k533_eval")
    assert KO.kernels_of(sd) == (5, 3, 3)
    np.testing.assert_allclose(KO.forward(sd, g["x"]), g["logits"], atol=1e-4, rtol=0)
    _, t = golden("cnn1d_k533_train")
    logits, loss, grads = KO.train_step(sd, t["x"], t["y"])
    np.testing.assert_allclose(logits, t["logits"], atol=1e-4, rtol=0)
    assert abs(loss - float(t["loss"])) <= 1e-5
    for k in KO.GRAD_KEYS:
        # (a conv bias in front of a BatchNorm has gradient zero up to rounding: measured on its weight's scale)
        ref = k.replace(".bias", ".weight") if k.startswith("conv.") and int(k.split(".")[1]) in KO.CONV_IDX else k
        scale = float(np.abs(grads[ref]).max())
        assert float(np.abs(t["grad." + k] - grads[k]).max()) <= 1e-3 * scale + 1e-7, k
    # ragged form = every utterance alone
    utts = KO.utterances([5, 9], 3)
    np.testing.assert_array_equal(KO.forward_ragged(sd, utts)[1:], KO.forward(sd, utts[1].T[None].astype(np.float64)))


def test_checkpoint_key_round_trip(capsys):
    args = types.SimpleNamespace(model="cnn1d")
    for kernels in ((3, 3, 3), (5, 3, 3)):
        m = CNN1D(kernels=kernels)
        blob = checkpoint_blob(m, torch.optim.SGD(m.parameters(), lr=0.1), 1, args)
        assert ("kernels" in blob) == (kernels != (3, 3, 3))      # (3, 3, 3) writes no key: the file is what it was
        assert resolve_kernels(None, blob) == kernels
        assert resolve_kernels(None, blob["model_state"]) == (3, 3, 3)     # a bare state dict
    assert capsys.readouterr().err == ""
    assert resolve_kernels((5, 3, 3), blob) == (5, 3, 3) and capsys.readouterr().err == ""
    assert resolve_kernels((3, 3, 3), blob) == (3, 3, 3)          # an explicit flag wins, and says so
    assert "warning: --kernels 3,3,3" in capsys.readouterr().err
    assert resolve_kernels((5, 3, 3), {}) == (5, 3, 3)
    assert "warning: --kernels 5,3,3" in capsys.readouterr().err
    with pytest.raises(ValueError, match=r"\(5, 3, 3\)"):
        resolve_kernels(None, {"kernels": (3, 5, 3)})


def test_reference_written_checkpoint_loads(golden):
    from dfa_amd.normalization import resolve_norm
    from dfa_amd.predict import build_model, load_weights, read_checkpoint
    sd, _ = golden("cnn1d_k533_eval")
    blob = read_checkpoint(REF_CKPT, "cpu")
    assert set(blob) == {"model_state", "kernels", "norm_mode", "best_epoch", "best_dev_eer"}     # src/compare_kernels.py:178-184
    kernels = resolve_kernels(None, blob)
    assert kernels == (5, 3, 3) and resolve_norm(None, blob) == "cmn"
    m = load_weights(build_model("cnn1d", kernels=kernels), REF_CKPT, "cpu", blob=blob)
    for k, v in m.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), sd[k], err_msg=k)
    with pytest.raises(RuntimeError, match="size mismatch"):
        load_weights(build_model("cnn1d"), REF_CKPT, "cpu", blob=blob)


def test_kernels_flag_is_cnn1d_only_and_checked_first(tmp_path):
    from dfa_amd import predict
    assert predict.check_kernels_arg("cnn1d", "5,3,3") == (5, 3, 3) and predict.check_kernels_arg("cnn2d", None) is None
    with pytest.raises(ValueError, match="--model cnn1d"):
        predict.check_kernels_arg("cnn2d", "5,3,3")
    with pytest.raises(ValueError, match="3,3,3 and 5,3,3"):
        predict.check_kernels_arg("cnn1d", "3,5,3")
    with pytest.raises(ValueError, match="3,3,3 and 5,3,3"):
        predict.check_kernels_arg("cnn1d", "5;3")
    # refused before the features file or the checkpoint is opened: neither exists
    missing = str(tmp_path / "nothing.pkl")
    with pytest.raises(ValueError, match="--model cnn1d"):
        predict.main(["--features", missing, "--checkpoint", missing, "--model", "cnn2d", "--out", missing, "--kernels", "5,3,3"])


def test_ragged_training_of_the_variant_is_refused_by_name():
    """the variant trains on uniform batches; a ragged batch or a ragged training file is refused up front, by name"""
    from dfa_amd import train
    from dfa_amd.training.train_step import forward_train_raw
    m = CNN1D(kernels=(5, 3, 3)).train()
    with pytest.raises(ValueError, match=r"kernels=\(3, 3, 3\)"):
        forward_train_raw(m, torch.zeros(2, 33, 180), lengths=[33, 20])
    args = types.SimpleNamespace(model="cnn1d", swap_tf=True, sync_bn=False, native=True, kernels="5,3,3")
    with pytest.raises(ValueError, match="--kernels 5,3,3"):
        train.check_ragged_train_args(args)
    args.kernels = None
    train.check_ragged_train_args(args)
    assert train.parse_args(["--kernels", "5,3,3", "--model", "cnn1d"]).kernels == "5,3,3" and train.parse_args([]).kernels is None


def _plan(T, F, k1):
    lib = _lib.load()
    n = lib.dfa_cnn1d_ragged_segments_k(T, F, k1, None, None, None, None, 0)
    arr = [(C.c_int * max(n, 1))() for _ in range(4)]
    assert lib.dfa_cnn1d_ragged_segments_k(T, F, k1, *arr, n) == n
    return [tuple(a[i] for a in arr) for i in range(n)]


def test_five_tap_segment_plan():
    """for T in 3..700 the owned ranges tile [0, T) exactly once; every window holds its owned frames plus 4 frames of halo to
    either side, or runs to the utterance's end; starts on a multiple of 4 (the 16-byte row loads); and fits the launch's LDS"""
    lib = _lib.load()
    for F in (180, 20):
        cap = lib.dfa_cnn1d_fused_max_t(F, 5)
        assert 3 <= cap <= 384
        for T in range(3, 701):
            plan = _plan(T, F, 5)
            assert plan, T
            nxt = 0
            for start, length, lo, hi in plan:
                assert lo == nxt and hi > lo, (T, plan)
                nxt = hi
                assert start % 4 == 0 and start == max(0, lo - 4) and start + length == min(T, hi + 4), (T, plan)
                assert 3 <= length <= 384
            assert nxt == T, (T, plan)
        assert len(_plan(384, 180, 5)) == 1 and len(_plan(385, 180, 5)) == 2 and len(_plan(700, 180, 5)) == 2
        assert 0 < lib.dfa_cnn1d_ragged_lds_bytes_k(700, F, 5) <= 160 * 1024
    # k1 = 3 is the old pair, any other k1 nothing
    for T in (2, 3, 321, 349, 700, 1000):
        n = lib.dfa_cnn1d_ragged_segments(T, 180, None, None, None, None, 0)
        assert lib.dfa_cnn1d_ragged_segments_k(T, 180, 3, None, None, None, None, 0) == n
        assert lib.dfa_cnn1d_ragged_lds_bytes_k(T, 180, 3) == lib.dfa_cnn1d_ragged_lds_bytes(T, 180)
    assert lib.dfa_cnn1d_ragged_segments_k(321, 180, 7, None, None, None, None, 0) == 0
    assert lib.dfa_cnn1d_ragged_lds_bytes_k(321, 180, 7) == 0 and lib.dfa_cnn1d_fused_max_t(180, 7) == 0
    assert 321 <= lib.dfa_cnn1d_fused_max_t(180, 3) < lib.dfa_cnn1d_fused_max_t(180, 5) == 384     # (streamed weights leave more LDS)
