"""The reference's own outputs in the CPU tests without the reference: where oracle/_ref is built (oracle/build_ref.py) the tests call it and
compare bit for bit, as they always did; where it is not, they compare against SHA-256 digests of those same outputs (and the few reference
tables they feed back in), committed in tests/golden/ref_digests.json.  With oracle/_ref present every live value is also checked against
its stored digest, so a stale fixture fails rather than hides.

Regenerate (oracle/_ref built):  OVRFSR_RECORD_REF_DIGESTS=1 python -m pytest -q tests/test_oracle.py tests/test_oracle_nis.py tests/test_constants.py"""
import atexit
import hashlib
import json
import os

import numpy as np

from oracle import oracle as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")
RECORD = os.environ.get("OVRFSR_RECORD_REF_DIGESTS") == "1"
_STORE = json.load(open(PATH)) if os.path.exists(PATH) else {}


def live():
    return O.have_ref()


def _bits(a, nan_equal):
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint32 if a.itemsize == 4 else np.uint8).copy()
    if nan_equal:
        bits[np.isnan(a)] = 0x7fc00000   # every NaN alike (two NaNs compare equal whatever their sign and payload)
    return bits


def digest(a, nan_equal=False):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(("%s %s;" % (a.dtype.str, a.shape)).encode())
    h.update(_bits(a, nan_equal).tobytes())
    return h.hexdigest()


def same_as_reference(key, got, ref_fn, nan_equal=False):
    """True when `got` (an oracle output) equals, bit for bit, what ref_fn() -- a call of the reference's own code -- returns: live where
    oracle/_ref exists, else through the stored digest of that output."""
    if live():
        want = np.ascontiguousarray(ref_fn())
        d = digest(want, nan_equal)
        if RECORD:
            _STORE[key] = d
        else:
            assert _STORE.get(key) == d, "tests/golden/ref_digests.json is stale for %s (regenerate it: tests/refgold.py)" % key
        return np.array_equal(_bits(got, nan_equal), _bits(want, nan_equal)) and np.asarray(got).shape == want.shape
    assert key in _STORE, "no stored digest for %s (tests/golden/ref_digests.json)" % key
    return digest(got, nan_equal) == _STORE[key]


def reference_value(key, ref_fn):
    """A small array the reference computes (NIS coefficient tables, scaler constant blocks) that a test feeds back into the oracle: live
    where oracle/_ref exists (and checked against the stored copy), else the stored copy."""
    if live():
        v = np.ascontiguousarray(ref_fn())
        rec = {"dtype": v.dtype.str, "shape": list(v.shape), "hex": v.tobytes().hex()}
        if RECORD:
            _STORE[key] = rec
        else:
            assert _STORE.get(key) == rec, "tests/golden/ref_digests.json is stale for %s (regenerate it: tests/refgold.py)" % key
        return v
    rec = _STORE[key]
    return np.frombuffer(bytes.fromhex(rec["hex"]), dtype=np.dtype(rec["dtype"])).reshape(rec["shape"]).copy()


def ref_nis_coefs():
    """the reference's NIS coefficient tables (scale, usm), as O.ref_nis_coefs()"""
    both = reference_value("nis_coefs", lambda: np.stack(O.ref_nis_coefs()))
    return both[0], both[1]


def ref_nis_scaler_config(sharpness, inW, inH, outW, outH):
    """the reference's NIS constant block (ok, block), as O.ref_nis_scaler_config(); keyed by its arguments"""
    def call():
        ok, buf = O.ref_nis_scaler_config(sharpness, inW, inH, outW, outH)
        return np.concatenate([np.array([int(ok)], np.uint32), buf])
    v = reference_value("nis_scaler_config/%r/%d/%d/%d/%d" % (float(sharpness), inW, inH, outW, outH), call)
    return bool(v[0]), v[1:].copy()


def _save():
    if RECORD and _STORE:
        with open(PATH, "w") as f:
            json.dump(dict(sorted(_STORE.items())), f, indent=0, sort_keys=True)
            f.write("\n")


atexit.register(_save)
