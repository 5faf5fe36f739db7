"""What the launch manager does for the launch-form matrix (tools/debug/record_forms.py: ~580 fresh ctxs through the C ABI -- every form,
source and destination format, refusal, batch and pair_submit case) against tests/golden/launch_forms_parent.json, the same matrix recorded on
an MI355X at the commit before the pipeline planner: the status and error text of every call, the format of a ctx-owned output and the SHA-256
of the output bytes are equal, case by case.  The record is never regenerated here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_forms_equal_the_parent_record(gpu):
    spec = importlib.util.spec_from_file_location("record_forms", os.path.join(ROOT, "tools", "debug", "record_forms.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_forms_parent.json")))
    cases = R.cases()
    assert {c["id"] for c in cases} == set(want)
    bad = []
    for c in cases:
        got = json.loads(json.dumps(R.run_case(c)))   # (tuples -> lists, as the record holds them)
        if got != want[c["id"]]:
            bad.append((c["id"], {k: (got.get(k), want[c["id"]].get(k)) for k in set(got) | set(want[c["id"]]) if got.get(k) != want[c["id"]].get(k)}))
    assert not bad, "%d of %d cases differ from the parent's record; first: %r" % (len(bad), len(cases), bad[:5])
