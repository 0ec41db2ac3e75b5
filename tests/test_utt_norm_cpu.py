"""Per-utterance CMN / CVMN normalisation, the part that needs no GPU: the float64 oracle against the
reference's own output (tests/golden/utt_norm.npz, written by tests/golden/make_golden_utt_norm.py), the reference's float32
error against the bound the GPU tests use, the C ABI's symbols, resolve_norm, --norm on the four CLIs, and norm_mode in a
checkpoint."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dfa_amd  # noqa: F401
from dfa_amd import _lib, normalization as N

import utt_norm_oracle as UO
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "utt_norm.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_oracle_matches_the_reference_fixture(fixture):
    for T in UO.FIXTURE_LENGTHS:
        x = fixture[f"x_{T}"]
        assert x.dtype == np.float32 and x.shape == (180, T)
        assert np.array_equal(_bits(x), _bits(UO.utterance(180, T))), f"the recipe no longer draws the fixture's utterance T={T}"
        for mode in UO.MODES:
            err = np.abs(fixture[f"{mode}_{T}"].astype(np.float64) - UO.normalize(x, mode)).max(axis=1)
            bound = UO.row_bound(x, mode)
            print(f"T={T} {mode}: max err / bound = {(err / bound).max():.3f}")
            assert (err <= bound).all(), (T, mode, float((err / bound).max()))


def test_normalize_utterance_is_the_reference_bit_for_bit(fixture):
    for T in UO.FIXTURE_LENGTHS:
        x = torch.from_numpy(fixture[f"x_{T}"])
        assert torch.equal(N.normalize_utterance(x, "raw"), x)
        for mode in UO.MODES:
            got = N.normalize_utterance(x, mode).numpy()
            assert np.array_equal(_bits(got), _bits(fixture[f"{mode}_{T}"])), (T, mode)
    with pytest.raises(ValueError):
        N.normalize_utterance(torch.zeros(3, 4), "zscore")


def test_reference_float32_stays_inside_the_bound():
    """the bound of the GPU tests is not tighter than the reference's own float32 arithmetic, at every length and channel count"""
    worst_unit, worst_bound = 0.0, 0.0
    for Cc in UO.CHANNELS:
        for T in UO.LENGTHS:
            x = UO.utterance(Cc, T)
            for mode in UO.MODES:
                y64, bound = UO.expected(Cc, T, mode)
                err = np.abs(UO.reference32(x, mode).astype(np.float64) - y64).max(axis=1)
                worst_unit = max(worst_unit, float((err / UO.first_term(x, mode)).max()))
                worst_bound = max(worst_bound, float((err / bound).max()))
                assert (err <= bound).all(), (Cc, T, mode, float((err / bound).max()))
    print(f"reference float32: at most {worst_unit:.2f} x 2^-24 max|x| / s, {worst_bound:.3f} of the bound")
    assert worst_bound > 0.01          # ... nor vacuous: the reference uses a visible part of it


def test_oracle_definition():
    x = np.array([[1.0, 2.0, 4.0], [5.0, 5.0, 5.0]], dtype=np.float32)
    assert np.allclose(UO.normalize(x, "cmn"), [[-4 / 3, -1 / 3, 5 / 3], [0, 0, 0]])
    s = np.sqrt(((np.array([1.0, 2.0, 4.0]) - 7 / 3) ** 2).sum() / 2)
    assert np.allclose(UO.normalize(x, "cvmn")[0], (np.array([1.0, 2.0, 4.0]) - 7 / 3) / s)
    assert np.array_equal(UO.normalize(x, "cvmn")[1], np.zeros(3))       # the clamp: 0 / 1e-8


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in ("dfa_utt_norm_workspace_bytes", "dfa_utt_norm", "dfa_utt_norm_packed"):
        assert hasattr(lib, name) and name in bound, name
    assert bound["dfa_utt_norm_workspace_bytes"] == (C.c_size_t, [C.c_int])
    res, args = bound["dfa_utt_norm"]
    assert res is C.c_int and len(args) == 13 and args[1] is C.c_int and args[7:10] == [C.c_int64] * 3 and args[12] is C.c_size_t
    res, args = bound["dfa_utt_norm_packed"]
    assert res is C.c_int and len(args) == 10 and args[3] is C.c_int64 and args[6:8] == [C.c_int, C.c_int] and args[9] is C.c_size_t
    assert (_lib.NORM_CMN, _lib.NORM_CVMN) == (1, 2)
    assert lib.dfa_utt_norm_workspace_bytes(0) == 0 and lib.dfa_utt_norm_workspace_bytes(-3) == 0
    assert lib.dfa_utt_norm_workspace_bytes(1) == 256 and lib.dfa_utt_norm_workspace_bytes(100) == 1792     # 4 B words, to 256 bytes
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dfa_hip.h")).read()
    assert f"#define DFA_UTT_NORM_HELD_FRAMES {_lib.UTT_NORM_HELD_FRAMES}\n" in header and UO.HELD_FRAMES == _lib.UTT_NORM_HELD_FRAMES
    assert f"#define DFA_UTT_NORM_MAX_PACKED {_lib.UTT_NORM_MAX_PACKED}\n" in header
    assert lib.dfa_utt_norm(None, 1, None, None, 1, 1, 1, 1, 1, 1, None, None, 0) == _lib.E_NULL_PTR
    assert lib.dfa_utt_norm_packed(None, 1, None, 0, None, None, 1, 1, None, 0) == _lib.E_NULL_PTR


def test_modes_and_the_gpu_only_entry_points():
    assert N.MODES == ("raw", "cmn", "cvmn")
    x = torch.zeros(2, 5, 4)
    assert N.normalize_batch(x, "raw") is x and N.normalize_stored(x, "raw") is x
    assert N.normalize_packed_(x.reshape(-1), [0], [5], 4, "raw").data_ptr() == x.data_ptr()
    with pytest.raises(RuntimeError, match="GPU"):
        N.normalize_batch(x, "cmn")
    with pytest.raises(ValueError):
        N.normalize_batch(x, "zscore")


def test_resolve_norm(capsys):
    assert N.resolve_norm(None, {}) == "raw"
    assert N.resolve_norm(None, {"model_state": {}}) == "raw"
    assert N.resolve_norm(None, {"norm_mode": "cvmn"}) == "cvmn"
    assert N.resolve_norm(None, {"norm_mode": "cmn", "model_state": {}}) == "cmn"
    assert N.resolve_norm(None, None) == "raw"                       # a file that holds no dict
    assert N.resolve_norm("cvmn", {"norm_mode": "cvmn"}) == "cvmn"
    assert N.resolve_norm("raw", {}) == "raw"
    assert capsys.readouterr().err == ""
    assert N.resolve_norm("cmn", {"norm_mode": "cvmn"}) == "cmn"      # the explicit flag wins, and says so
    err = capsys.readouterr().err
    assert "cmn" in err and "cvmn" in err
    assert N.resolve_norm("raw", {"norm_mode": "cvmn"}) == "raw"
    assert "cvmn" in capsys.readouterr().err
    assert N.resolve_norm("cvmn", {}) == "cvmn"
    assert "raw" in capsys.readouterr().err
    with pytest.raises(ValueError):
        N.resolve_norm(None, {"norm_mode": "zscore"})
    with pytest.raises(ValueError):
        N.resolve_norm("zscore", {})


def _parsers():
    from dfa_amd import dlqueen_model, predict, train, train_dlqueen
    need = ["--features", "f.pkl", "--checkpoint", "c.pt", "--model", "cnn1d", "--out", "o.pkl"]
    return {"train": (train.parse_args, []), "predict": (predict.parse_args, need), "train_dlqueen": (train_dlqueen.parse_args, []),
            "dlqueen_model": (dlqueen_model.parse_args, [])}


@pytest.mark.parametrize("cli", ["train", "predict", "train_dlqueen", "dlqueen_model"])
def test_norm_flag_parses_with_default_raw(cli):
    parse, need = _parsers()[cli]
    args = parse(need)
    assert args.norm == "raw" and args.norm_explicit is False and N.explicit_norm(args) is None
    for mode in N.MODES:
        args = parse(need + ["--norm", mode])
        assert args.norm == mode and args.norm_explicit is True and N.explicit_norm(args) == mode
    with pytest.raises(SystemExit):
        parse(need + ["--norm", "zscore"])


def test_checkpoint_carries_norm_mode_only_when_not_raw(tmp_path):
    from dfa_amd.train_dlqueen import dlq_checkpoint
    from dfa_amd.training import checkpoint_blob, load_checkpoint, save_checkpoint
    model = torch.nn.Linear(3, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    args = argparse.Namespace(model="cnn1d", batch_size=4, lr=0.1)
    raw = checkpoint_blob(model, opt, 2, args)
    assert "norm_mode" not in raw and set(raw) == {"model_state", "optimizer_state", "epoch", "config"}
    assert "norm_mode" not in checkpoint_blob(model, opt, 2, args, norm_mode="raw")
    for mode in ("cmn", "cvmn"):
        blob = checkpoint_blob(model, opt, 2, args, norm_mode=mode)
        assert blob["norm_mode"] == mode and set(blob) == set(raw) | {"norm_mode"}
        path = str(tmp_path / f"{mode}.pt")
        save_checkpoint(model, opt, 2, args, path, norm_mode=mode)
        back = load_checkpoint(path, model=torch.nn.Linear(3, 1))         # still loads as a checkpoint of the reference's layout
        assert back["norm_mode"] == mode and N.resolve_norm(None, back) == mode
    save_checkpoint(model, opt, 2, args, str(tmp_path / "raw.pt"))
    assert "norm_mode" not in load_checkpoint(str(tmp_path / "raw.pt"))
    # the DeepfakeDetector's file: the bare state_dict as before, wrapped only to carry a mode
    assert set(dlq_checkpoint(model)) == set(model.state_dict())
    wrapped = dlq_checkpoint(model, "cvmn")
    assert set(wrapped) == {"model_state", "norm_mode"} and wrapped["norm_mode"] == "cvmn"
    assert N.resolve_norm(None, dlq_checkpoint(model)) == "raw" and N.resolve_norm(None, wrapped) == "cvmn"
