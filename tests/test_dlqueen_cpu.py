"""CPU side of the DeepfakeDetector (Conv1d + StatsPool) eval forward: the float64 statement of the model
(tests/dlqueen_oracle.py) is pinned to what the reference itself computed (tests/golden/dlqueen_eval.npz, written by
tests/golden/make_golden_dlqueen.py), the padded-batch rule is checked on it, and the host-side pieces -- state_dict layout,
seeded initialisation, refusals, CLI arguments, order restoration, the C ABI table -- are checked without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import dlqueen_oracle as DO
from dfa_amd import _lib, dlqueen_model as M
from dfa_amd.dlqueen_model import DeepfakeDetector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dfa_dlq_set_params", "dfa_dlq_prepare", "dfa_dlq_workspace_bytes", "dfa_dlq_forward")


@pytest.fixture(scope="module")
def fx(golden):
    _, g = golden("dlqueen_eval")
    return g, DO.fixture_state_dict(g, DeepfakeDetector), DO.split_utts(g)


def test_oracle_equals_the_reference_in_all_three_padding_classes(fx):
    g, sd, utts = fx
    x, lengths = DO.pad_batch(utts)
    assert x.shape == (13, 180, 321) and sum(lengths) == 754
    lg, pooled = DO.forward(sd, x, lengths)
    np.testing.assert_allclose(lg, g["batch.logits64"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(pooled, g["batch.pooled64"], rtol=0, atol=1e-10)
    for tag, extra in (("alone", 0), ("pad1", 1)):
        for i, u in enumerate(utts):
            xi, li = DO.pad_batch([u], u.shape[-1] + extra)
            lg, pooled = DO.forward(sd, xi, li)
            np.testing.assert_allclose(lg, g[tag + ".logits64"][i:i + 1], rtol=0, atol=1e-10, err_msg=f"{tag} {i}")
            np.testing.assert_allclose(pooled, g[tag + ".pooled64"][i:i + 1], rtol=0, atol=1e-10, err_msg=f"{tag} {i}")
    S = float(g["S"])
    assert S >= 1.0 and S == float(np.abs(g["batch.logits64"]).max())
    assert g["batch.logits64"].min() < 0 < g["batch.logits64"].max()


def test_padded_batch_rule_on_the_oracle(fx):
    """the logit depends on the padding through min(T - len, 2) only, and does depend on it"""
    g, sd, utts = fx
    S = float(g["S"])
    for i in (5, 8):                                   # len 31, 63
        u = utts[i]
        n = u.shape[-1]
        by_pad = {p: DO.forward(sd, *DO.pad_batch([u], n + p))[0][0] for p in (0, 1, 2, 3, 10)}
        assert abs(by_pad[2] - by_pad[10]) <= 1e-12 and abs(by_pad[2] - by_pad[3]) <= 1e-12      # (equal up to float64 summation order)
        assert abs(by_pad[0] - by_pad[2]) > 1e-5 * S and abs(by_pad[1] - by_pad[2]) > 1e-5 * S
        # what stands in the padding does not matter
        xn, ln = DO.pad_batch([u], n + 3, fill=float("nan"))
        assert abs(DO.forward(sd, xn, ln)[0][0] - by_pad[3]) <= 1e-12
    _, pooled = DO.forward(sd, *DO.pad_batch([utts[0]], 4))     # len = 1: the variance clamp
    np.testing.assert_array_equal(pooled[0, 256:], np.full(256, np.sqrt(1e-6)))
    np.testing.assert_allclose(pooled[0, 256:], 1e-3, rtol=1e-15)


def test_state_dict_keys_shapes_and_order_equal_the_reference(fx):
    g, _, _ = fx
    mine = DeepfakeDetector(180).state_dict()
    assert list(mine.keys()) == [str(k) for k in g["keys"]]
    for k, v in mine.items():
        assert tuple(v.shape) == tuple(int(d) for d in g["shape." + k]), k
    assert mine["enc.net.1.num_batches_tracked"].dtype == torch.long


def test_strict_load_of_the_reference_state_dict(fx):
    _, sd, _ = fx
    m = DeepfakeDetector(180)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_seeded_default_init_equals_the_reference(fx):
    g, _, _ = fx
    torch.manual_seed(DO.INIT_SEED)
    sd = DeepfakeDetector(180).state_dict()
    checked = 0
    for k, v in sd.items():
        if "head32." + k in g:
            np.testing.assert_array_equal(v.reshape(-1)[:32].numpy(), g["head32." + k], err_msg=k)
            assert DO.exact_sums(v.double().reshape(-1).tolist()) == (float(g["sum." + k]), float(g["abssum." + k])), k
            checked += 1
    assert checked == 8                                # three convolutions and head.0, weight and bias


def test_train_mode_and_cpu_input_are_refused():
    m = DeepfakeDetector(180)
    with pytest.raises(NotImplementedError, match="eval-only"):
        m.train()(torch.zeros(1, 180, 8), [8])
    with pytest.raises(RuntimeError, match="GPU only"):
        m.eval()(torch.zeros(1, 180, 8), [8])
    with pytest.raises(ValueError, match=r"\(B, C, T\)"):
        m.eval()(torch.zeros(180, 8), [8])


def test_cli_arguments(capsys):
    a = M.parse_args(["--data_dir", "d", "--test_split", "dev", "--ckpt_path", "c.pth", "--prediction_pkl", "p.pkl", "--batch_size", "7",
                      "--hidden", "256", "--dropout", "0.1", "--use_prob", "--device", "cuda:0", "--file-order"])
    assert (a.data_dir, a.test_split, a.ckpt_path, a.prediction_pkl, a.batch_size, a.hidden, a.dropout, a.use_prob, a.device, a.file_order,
            a.epochs) == ("d", "dev", "c.pth", "p.pkl", 7, 256, 0.1, True, "cuda:0", True, 0)
    d = M.parse_args([])
    assert (d.epochs, d.batch_size, d.hidden, d.dropout, d.use_prob, d.file_order, d.test_split) == (0, 32, 256, 0.3, False, False, "test2")
    with pytest.raises(SystemExit) as e:
        M.parse_args(["--epochs", "1"])
    assert e.value.code != 0
    assert "eval-only" in capsys.readouterr().err


class _Stub(torch.nn.Module):
    """logit = the utterance's first valid value + its length + 1000 * min(T - len, 2): shows order and padding class"""

    def forward(self, x, lengths):
        n = torch.as_tensor(np.asarray(lengths), dtype=torch.float32)
        pad = torch.clamp(x.shape[2] - n, max=2.0)
        return x[:, 0, 0].float() + n + 1000.0 * pad


@pytest.mark.parametrize("file_order", [False, True])
def test_run_inference_restores_input_order(file_order):
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(1, 40, size=23)]
    feats = [torch.full((8, n), float(i) / 64) for i, n in enumerate(lens)]
    out = M.run_inference(_Stub(), feats, batch_size=5, device="cpu", file_order=file_order)
    assert out.shape == (23,)
    base = out.numpy() % 1000.0
    np.testing.assert_allclose(base, np.array([i / 64 + n for i, n in enumerate(lens)], dtype=np.float32), rtol=0, atol=1e-4)
    if file_order:                                     # the reference's batches: consecutive files, padded to the batch's longest
        want = [min(max(lens[i // 5 * 5:i // 5 * 5 + 5]) - n, 2) for i, n in enumerate(lens)]
        np.testing.assert_array_equal(np.round((out.numpy() - base) / 1000.0), want)
    prob = M.run_inference(_Stub(), feats, batch_size=5, device="cpu", use_prob=True, file_order=file_order)
    np.testing.assert_allclose(prob.numpy(), torch.sigmoid(out).numpy())


def test_library_exports_the_new_symbols_and_the_tile_size():
    lib = _lib.load()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound, name
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    assert int(re.search(r"#define DFA_DLQ_TILE_FRAMES (\d+)", header).group(1)) == M.TILE_FRAMES
    assert int(re.search(r"#define DFA_DLQ_NPARAMS (\d+)", header).group(1)) == len(DeepfakeDetector(8)._abi_tensors()) == 22
    assert lib.dfa_dlq_workspace_bytes(None, 0, 10, 180) == 0
    n = lib.dfa_dlq_workspace_bytes(None, 3, 100, 180)
    assert n % 256 == 0 and n >= 2 * 3 * 100 * 1536
