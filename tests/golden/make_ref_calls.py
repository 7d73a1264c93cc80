#!/usr/bin/env python3
"""Record the REAL reference's result of every call tests/test_oracle_vs_ref.py makes into tests/golden/ref_calls.json.

Run where the reference tree exists and `make -C oracle` has compiled it into oracle/_ref/libhmj_ref.so:
    python tests/golden/make_ref_calls.py
It replays the tests with a recording reference (so the C restatement is checked against the live reference on the
way).  Each entry maps a call -- method name + digest of its arguments -- to the digest of the reference's result
(oracle/pyoracle.py: digest, RecordedReference); the inputs themselves come from the tests' seeded generators.
Fixtures are data only -- no reference source text is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.pyoracle import Oracle, RecordedReference, Reference  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402

live = Reference()
assert live.available, "build oracle/_ref first: make -C oracle ref"
o, rec = Oracle(), RecordedReference({}, live=live, record=True)
for n in T.SORT_SIZES:
    T.test_sorts_match_reference(o, rec, n)
for nr, ns, dom in T.JOIN_CASES:
    T.test_joins_match_reference(o, rec, nr, ns, dom)
T.test_unique_keys_all_formulations_agree(o, rec)
T.test_ordered_output_independent_of_threads(rec, o)

with open(os.path.join(HERE, "ref_calls.json"), "w") as f:
    json.dump({"_about": "digests of the compiled reference's results on the calls of tests/test_oracle_vs_ref.py; "
                         "see make_ref_calls.py", "calls": dict(sorted(rec.calls.items()))}, f, indent=0)
    f.write("\n")
print("wrote ref_calls.json with %d calls" % len(rec.calls))
