"""Host side of the DeepfakeDetector's resident training set: draw_spans against spec_augment, the
packed-set plan, the new symbols of the C ABI and the CLI flag.  Every comparison is exact."""
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8, 1), (8, 3), (5, 20), (180, 321))
CONFIGS = ((30, 2, 24, 2), (2, 2, 3, 1), (0, 2, 24, 2), (30, 0, 0, 0), (400, 3, 400, 3))


def apply_spans(x, spans, n_t):
    """the kernel's defining expression on one [C, T] sample, as slice assignments"""
    for k, (s0, w) in enumerate(spans.tolist()):
        if k < n_t:
            x[:, s0:s0 + w] = 0.0
        else:
            x[s0:s0 + w, :] = 0.0
    return x


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_draw_spans_equals_spec_augment(shape, cfg):
    from dfa_amd import train_dlqueen as TD
    Cc, T = shape
    n_t, n_f = TD.span_counts(*cfg)
    base = torch.arange(1, Cc * T + 1, dtype=torch.float32).reshape(Cc, T)          # nonzero everywhere
    whole_axis = 0
    for seed in range(200):
        ra, rb = random.Random(seed), random.Random(seed)
        want = TD.spec_augment(base.clone(), ra, *cfg)
        spans = TD.draw_spans(rb, Cc, T, *cfg)
        assert spans.dtype == np.int32 and spans.shape == (n_t + n_f, 2)
        assert (spans >= 0).all() and (spans[:n_t].sum(1) <= T).all() and (spans[n_t:].sum(1) <= Cc).all()
        assert torch.equal(apply_spans(base.clone(), spans, n_t), want), (seed, spans)
        assert ra.random() == rb.random(), seed                                     # both generators left in the same state
        whole_axis += int((spans[:n_t, 1] == T).any() or (spans[n_t:, 1] == Cc).any())
    if cfg == (400, 3, 400, 3):
        assert whole_axis > 0                     # the maxima are clamped by the dimension: whole-axis masks occur


def test_plan_packed_set():
    from dfa_amd.dataloaders import plan_packed_set
    for Cc in (5, 180):
        lens = [1, 2, 3, 4, 5]
        off, total = plan_packed_set(lens, Cc)
        assert off.dtype == np.int64 and off.tolist() == [0, 4 * Cc, 8 * Cc, 12 * Cc, 16 * Cc] and total == 24 * Cc
    off, total = plan_packed_set([], 180)
    assert off.shape == (0,) and total == 0
    g = np.random.default_rng(0)
    lens = g.integers(161, 322, size=60000)                  # plan only: nothing is allocated
    off, total = plan_packed_set(lens, 180)
    pitch = (lens + 3) // 4 * 4
    assert total > 2 ** 31 and total == int((180 * pitch).sum()) and off.dtype == np.int64
    assert (off % 4 == 0).all() and off[0] == 0 and (np.diff(off) > 0).all()
    assert np.array_equal(off[1:], off[:-1] + 180 * pitch[:-1]) and off[-1] + 180 * pitch[-1] == total     # back to back: no overlap, no gap
    for bad in ([3, 0], [-1]):
        with pytest.raises(ValueError):
            plan_packed_set(bad, 180)


def test_gather_symbols_declared_and_bound():
    from dfa_amd import _lib
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    declared = set(re.findall(r"\b(dfa_[a-z0-9_]+)\s*\(", header))
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in ("dfa_dlq_gather_batch", "dfa_dlq_gather_workspace_bytes"):
        assert name in declared and name in bound
    assert len(bound["dfa_dlq_gather_batch"][1]) == 16 and len(bound["dfa_dlq_gather_workspace_bytes"][1]) == 3
    lib = _lib.load()
    assert lib.dfa_dlq_gather_workspace_bytes(16, 2, 2) == 768           # (4 * 16 + 2 * 16 * 4) words = 768 bytes
    assert lib.dfa_dlq_gather_workspace_bytes(5, 2, 1) == 256            # (4 * 5 + 2 * 5 * 3) words = 200 bytes, rounded to 256
    assert lib.dfa_dlq_gather_workspace_bytes(1, 0, 0) == 256
    assert lib.dfa_dlq_gather_workspace_bytes(0, 0, 0) == 0 and lib.dfa_dlq_gather_workspace_bytes(4, 9, 8) == 0


def test_resident_flag_parses_and_leaves_the_rest(capsys):
    from dfa_amd import train_dlqueen as TD
    plain = vars(TD.parse_args([]))
    assert plain.pop("resident") is False
    res = vars(TD.parse_args(["--resident"]))
    assert res.pop("resident") is True
    assert res == plain                                       # every existing field as it is without the flag
    a = TD.parse_args(["--resident", "--specaug", "--time_mask_n", "8", "--freq_mask_n", "8"])
    assert a.resident and a.time_mask_n + a.freq_mask_n == 16
    with pytest.raises(SystemExit):
        TD.parse_args(["--resident", "--specaug", "--time_mask_n", "9", "--freq_mask_n", "8"])
    assert "16" in capsys.readouterr().err
    assert TD.parse_args(["--specaug", "--time_mask_n", "9", "--freq_mask_n", "8"]).resident is False   # the host loop has no such limit
