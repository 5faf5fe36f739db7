"""What cfg.pair_submit does for sequences of submissions (tools/debug/record_sequences.py: every eye sequence of length 1 to 6 with
caller-owned and with ctx-owned outputs, and the scripted cases -- a batch call between the eyes, size changes, reset and set_config with a
recorded eye, unpairable second eyes, shared side-by-side textures, no stage selected) against tests/golden/submit_sequences_parent.json, the
same matrix recorded on an MI355X at the commit before the submission sequencer (csrc/submit_sequence.cpp): status, error text,
ovrfsr_pair_pending and the image handed back are equal call by call, the SHA-256 of every output image case by case.  The record is never
regenerated here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_submit_sequences_equal_the_parent_record(gpu):
    spec = importlib.util.spec_from_file_location("record_sequences", os.path.join(ROOT, "tools", "debug", "record_sequences.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "submit_sequences_parent.json")))
    cases = R.cases()
    assert {c["id"] for c in cases} == set(want)
    assert sum(c["id"].startswith("plain/") for c in cases) == 2 * 126 and sum(c["id"].startswith("scripted/") for c in cases) >= 12
    bad = []
    for c in cases:
        got = json.loads(json.dumps(R.run_case(c)))   # (tuples -> lists, as the record holds them)
        if got != want[c["id"]]:
            bad.append((c["id"], got, want[c["id"]]))
    assert not bad, "%d of %d cases differ from the parent's record; first: %r" % (len(bad), len(cases), bad[:3])
