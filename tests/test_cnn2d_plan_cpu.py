"""dfa_cnn2d_forward_plan (deep-fake-audio-classifier_amd/csrc/cnn2d_api.hip) against the dispatch rule as it stood before the
eval API was split by model, when the rule was spread over the planner and the two forwards of csrc/api.hip.

tests/golden/cnn2d_forward_plan.npz is that rule, recorded: a throwaway host program included that commit's api.hip in its own
translation unit (so plan_cnn2d, seg_iters_for and chunk3_for were callable), carried the lines of dfa_cnn2d_forward and
dfa_cnn2d_forward_ragged that form fused12, fused123, the seg_iters values, nseg3 and split3 verbatim, took the conv123 form from
that commit's conv123_plan, and printed one row per case.  `inputs` [13, N]: B, T, F, precision, ragged, the seven options in the
order of _lib.CNN2D_PLAN_OPTIONS, the CU count; `fields` [19, N]: the order of _lib.CNN2D_PLAN_FIELDS.  The grid: B in {1, 2, 5,
32, 85, 86, 170, 171, 256, 512, 1024} x T in {4, 5, 33, 52, 130, 321, 323, 700} x F in {5, 30, 31, 65, 180, 225}; every precision
with time_split in {-1, 0, 2, 4} at the default flags and 256 CUs; for bf16 at time_split = -1 also each of the six flags at 0
on its own, 304 and 7 CUs, and the ragged plan.  It crosses B * strips = 510 / 516, F = 30 / 31 (where the two strip widths
disagree), niter <= period, the 4-chunk cap and the carry form's conditions.

Host arithmetic only: the entry is called without a context, so no device is needed."""
import os

import numpy as np
import pytest

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnn2d_forward_plan.npz")
DEFAULTS = (-1, 1, 1, 1, 1, 1, 1)


@pytest.fixture(scope="module")
def abi():
    from dfa_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def table():
    z = np.load(DATA)
    return z["inputs"].T.tolist(), z["fields"].T.tolist()


def test_the_table_covers_the_grid(abi, table):
    L, _ = abi
    inputs, fields = table
    assert len(inputs) == len(fields) == 11 * 8 * 6 * (3 * 4 + 6 + 2 + 1)
    assert len(inputs[0]) == 5 + len(L.CNN2D_PLAN_OPTIONS) + 1 and len(fields[0]) == len(L.CNN2D_PLAN_FIELDS)
    assert len({tuple(r) for r in inputs}) == len(inputs)
    units = {r[0] * -(-r[2] // 30) for r in inputs}
    assert {510, 516} <= units


def test_the_plan_equals_the_recorded_rule_in_every_field(abi, table):
    L, lib = abi
    inputs, fields = table
    names = L.CNN2D_PLAN_FIELDS
    for row, want in zip(inputs, fields):
        B, T, F, prec, ragged = row[:5]
        opts, cus = tuple(row[5:12]), row[12]
        got = L.cnn2d_forward_plan(None, B, T, F, prec, ragged, opts, cus)
        assert list(got) == want, (row, [(n, g, w) for n, g, w in zip(names, got, want) if g != w])
        p = dict(zip(names, got))
        if opts == DEFAULTS:      # a null options pointer means the defaults; the planners give this plan's total
            assert L.cnn2d_forward_plan(None, B, T, F, prec, ragged, None, cus) == got, row
            planner = lib.dfa_ragged_workspace_bytes if ragged else lib.dfa_workspace_bytes
            assert planner(None, L.MODEL_CNN2D, B, T, F, prec) == p["total"], row
        # a split block 3 has a chunk slab for each of its chunks behind slab 0, and there are never more than four chunks
        if p["seg3"] != 0 or p["split3"]:
            assert p["slabs"] > 1 and p["nseg3"] <= p["slabs"] - 1, (row, p)
        assert 1 <= p["nseg3"] <= 4, (row, p)
        assert p["total"] == p["tab_off"] + -(-p["tab_words"] * 4 // 256) * 256, (row, p)


def test_the_table_has_every_kind_of_plan(table, abi):
    """(so that "equal in every field" above is a statement about every path, form and split, not about one of them)"""
    L, _ = abi
    _, fields = table
    col = {n: {r[i] for r in fields} for i, n in enumerate(L.CNN2D_PLAN_FIELDS)}
    assert col["path"] == {0, 1, 2} and col["form"] == {0, 1, 2, 3} and col["phase"] == {0, 1}
    assert col["slabs"] == {1, 5} and col["nseg3"] == {1, 2, 4} and col["split3"] == {0, 1}   # (T = 130: 2 chunks, 321 / 323 / 700: 4)
    assert len(col["seg12"]) > 3 and len(col["seg3"]) > 3 and col["chunk3"] == {0, 12, 24}


def test_bad_shapes_and_short_arrays(abi):
    L, lib = abi
    import ctypes as C
    for B, T, F in ((0, 33, 180), (2, 0, 180), (2, 33, 0)):
        assert lib.dfa_cnn2d_forward_plan(None, B, T, F, L.PREC_BF16, 0, None, 256, None, 0) == 0
    out = (C.c_longlong * 4)(-7, -7, -7, -7)
    assert lib.dfa_cnn2d_forward_plan(None, 2, 33, 180, L.PREC_BF16, 0, None, 256, out, 3) == len(L.CNN2D_PLAN_FIELDS)
    assert list(out) == [16, 8, 0, -7]
    assert lib.dfa_cnn2d_forward_plan(None, 2, 33, 180, L.PREC_BF16, 0, None, 256, None, 0) == len(L.CNN2D_PLAN_FIELDS)
