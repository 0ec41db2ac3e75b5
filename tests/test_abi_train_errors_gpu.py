"""The refusals of the C ABI's training entry points are behaviour too: the trainers turn the codes into exceptions and callers
read the text.  Every case of tests/abi_train_error_cases.py is replayed on one context and compared -- return code and
dfa_last_error text, pointers as PTR -- with tests/golden/abi_train_errors.json, recorded by
tests/golden/make_golden_abi_errors.py train before the training host layer's helpers were gathered into csrc/train_host.h."""
import json
import os

import pytest

import abi_train_error_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_train_errors.json")


def test_abi_train_refusals_match_the_recorded_ones():
    with open(GOLDEN) as f:
        want = [tuple(r) for r in json.load(f)]
    assert [r[0] for r in want] == abi_train_error_cases.CASE_IDS    # the list and the file cannot drift
    got = [tuple(r) for r in abi_train_error_cases.record()]
    assert all(rc != 0 for _, rc, _ in got), [r for r in got if r[1] == 0]
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, "\n".join(f"got {g}\nwant {w}" for g, w in diff)
