"""The launch-form matrix (tools/debug/record_forms.py::cases()) against the CPU ORACLE, case by case: every case the record
(tests/golden/launch_forms_parent.json) accepts runs on a fresh ctx through the C ABI and its output arrays are compared with
tests/forms_model.expected(case) under the case's contract class (tests/forms_model.py; the header's "Arithmetic the kernels run in").
tests/test_gpu_launch_forms.py shows that nothing moved since the record was taken; this file shows that what was recorded is right.

  * whole-frame bits cases (strict build, exact stores, product EASU-only into UNORM8): the oracle's bytes;
  * the other classes: their bound, and inside them the bits sub-assertions -- groups outside the radius in RGBA8 forms and NIS DirectCopy
    groups are the oracle's bytes; fused = -1 stores what fused = 0 stores wherever auto does not pick the fused kernel; precision 3
    stores what precision 2 stores;
  * every product-arithmetic case (precision 0 and 3) a second time on synth.random_u8 content in the source's format: the structured
    generator is smooth and meets few near-ties, random content is what trips the guards.  No hash exists for these runs, only the oracle.

Product-build distances (max LSB or max abs, share of differing values, per case and content) go to reports/launch_forms_oracle.json
(OVRFSR_REPORT_DIR names another directory); they are recorded, not asserted beyond the class.  The committed copy of the measuring run
is profiles/launch_forms_oracle.json."""
import json
import os

import pytest

from tests import forms_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.record_forms()
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_forms_parent.json")))
ACCEPTED = [c for c in R.cases() if RECORD[c["id"]]["sha256"] and c["id"] not in M.UNMODELLED]
_REPORT = {}     # case id -> {content: [distance records]}
_HASHES = {}     # case id -> SHA-256 of the structured-content output, for the form-pair assertions


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _REPORT:
        return
    out_dir = os.environ.get("OVRFSR_REPORT_DIR") or os.path.join(ROOT, "reports")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "launch_forms_oracle.json"), "w") as f:
        json.dump({"note": "the launch-form matrix, product arithmetic (precision 0 and 3) against the CPU oracle; written by "
                           "tests/test_gpu_launch_forms_oracle.py.  max_lsb: UNORM8 / 10-bit outputs, max_abs: half / float outputs; "
                           "differing: share of the output's values whose words differ from the oracle's",
                   "classes": {cid: M.contract(M.BY_ID()[cid]) for cid in sorted(_REPORT)},
                   "cases": {cid: _REPORT[cid] for cid in sorted(_REPORT)}}, f, indent=0, sort_keys=True)
        f.write("\n")


_DEVICE_ERROR = []   # an exception out of a case (run_case synchronises the device on its way out) ends the file: nothing more is launched


def _run(case, content):
    if _DEVICE_ERROR:
        pytest.fail("not run: an earlier case raised on the device: %s" % _DEVICE_ERROR[0])
    try:
        got = R.run_case(case, content=content, arrays=True)
    except Exception as e:
        _DEVICE_ERROR.append("%s (%s): %r" % (case["id"], content, e))
        raise
    assert all(rc == 0 for rc, _ in got["calls"]) and got["arrays"] is not None, (case["id"], content, got["calls"])
    return got


@pytest.mark.parametrize("cid", [c["id"] for c in ACCEPTED])
def test_case_is_the_oracles(gpu, cid):
    case = M.BY_ID()[cid]
    product = case["cfg"].get("precision", 0) != M.STRICT
    for content in (R.CONTENTS if product else R.CONTENTS[:1]):
        got = _run(case, content)
        if content == "structured":
            assert got["owned_format"] == RECORD[cid]["owned_format"], cid
            _HASHES[cid] = got["sha256"]
        dist = M.check(case, got["arrays"], content)
        print("launch forms oracle:", cid, content, M.contract(case), json.dumps(dist))
        if product:
            _REPORT.setdefault(cid, {})[content] = dist


def test_form_and_precision_pairs_store_the_same_bytes(gpu):
    """mask-sorted (fused = -1) = two-pass (fused = 0) wherever auto does not pick the fused kernel; precision 3 = precision 2 -- over the
    cases of this session that ran (the whole matrix in a full run)"""
    pairs = 0
    for cid, sha in _HASHES.items():
        for a, b in (("-f-1-", "-f0-"), ("/p3-", "/p2-")):
            other = cid.replace(a, b)
            if a not in cid or other not in _HASHES or (a == "-f-1-" and M.auto_is_fused(M.BY_ID()[cid])):
                continue
            pairs += 1
            assert sha == _HASHES[other], (cid, other)
    if len(_HASHES) == len(ACCEPTED):
        assert pairs >= 150, pairs
