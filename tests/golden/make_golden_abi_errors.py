#!/usr/bin/env python3
"""Records how the C ABI refuses every case of tests/abi_error_cases.py: run ONCE on an MI355X, at the commit whose behaviour is
to be kept, after the library has been built:      python tests/golden/make_golden_abi_errors.py [train] [OUT.json]

Writes tests/golden/abi_errors.json (or OUT.json) -- data only: a list of [case id, return code, dfa_last_error text], every
0x... pointer in the text replaced by PTR.  tests/test_abi_errors_gpu.py replays the same list and compares.  With `train` it
records tests/abi_train_error_cases.py into tests/golden/abi_train_errors.json, for tests/test_abi_train_errors_gpu.py."""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))     # the repository root (dfa_amd)

import abi_error_cases  # noqa: E402
import abi_train_error_cases  # noqa: E402


def main():
    args = sys.argv[1:]
    train = args[:1] == ["train"]
    cases = abi_train_error_cases if train else abi_error_cases
    path = args[train] if len(args) > train else os.path.join(OUT, "abi_train_errors.json" if train else "abi_errors.json")
    rows = cases.record()
    accepted = [r for r in rows if r[1] == 0]
    assert not accepted, f"cases the library did not refuse: {accepted}"
    with open(path, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    for r in rows:
        print(r)
    print(f"wrote {path}: {len(rows)} cases")


if __name__ == "__main__":
    main()
