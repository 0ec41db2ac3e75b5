#!/usr/bin/env python3
"""Records how the C ABI refuses every case of tests/abi_error_cases.py: run ONCE on an MI355X, at the commit whose behaviour is
to be kept, after the library has been built:      python tests/golden/make_golden_abi_errors.py [OUT.json]

Writes tests/golden/abi_errors.json (or OUT.json) -- data only: a list of [case id, return code, dfa_last_error text], every
0x... pointer in the text replaced by PTR.  tests/test_abi_errors_gpu.py replays the same list and compares."""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))     # the repository root (dfa_amd)

import abi_error_cases  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(OUT, "abi_errors.json")
    rows = abi_error_cases.record()
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
