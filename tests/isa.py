"""The machine-code record of the kernels, in one place for the tests that hold a change to "these kernels moved, no others did":
tools/isa_fingerprint.py (per-kernel MD5 of the disassembly), the fingerprint of the library as built, and the records under profiles/.
profiles/isa_fingerprint.json is the record of the current library; the *_before.json files are the parent builds of earlier changes."""
import functools
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openvr_fsr_amd", "libopenvr_fsr_amd.so")


@functools.lru_cache(maxsize=None)
def load_tool():
    spec = importlib.util.spec_from_file_location("isa_fingerprint", os.path.join(ROOT, "tools", "isa_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fingerprint_of_built_library():
    return load_tool().fingerprint(LIB)


def fingerprint_of_built_library():
    """{kernel name: {"md5": ..., "n": instructions}} of the built library, disassembled once per process; a copy the caller may keep"""
    return dict(_fingerprint_of_built_library())


def record(name):
    return json.load(open(os.path.join(ROOT, "profiles", name)))
