"""CPU (no GPU): bts_eval_frame_gt -- the evaluation frame with rgb_gt written by the hand-over launch -- is additive to ABI 9: declared in
include/bts_render.h, bound in _lib.py with three arguments, exported by the built library; the version stays 9."""
import ctypes as C
import os
import re

import pytest

from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bts_render.h")


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def test_bts_eval_frame_gt_is_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+bts_eval_frame_gt\s*\(([^)]*)\)\s*;", src)
    assert m, "bts_eval_frame_gt is not declared in include/bts_render.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 3 and params[0].startswith("const BtsEvalFrame*") and params[1].startswith("float*") and params[2].startswith("void*")
    assert re.search(r"\bint\s+bts_eval_frame\s*\(\s*const BtsEvalFrame\*\s*\w+\s*,\s*void\*\s*\w+\s*\)\s*;", src), "bts_eval_frame must stay"
    res, args = _lib.SYMBOLS["bts_eval_frame_gt"]
    assert res is C.c_int and len(args) == 3 and args[0] is C.POINTER(_lib.BtsEvalFrame) and args[1] is C.c_void_p and args[2] is C.c_void_p
    assert hasattr(lib, "bts_eval_frame_gt") and hasattr(lib, "bts_eval_frame")
    assert lib.bts_eval_frame_gt.argtypes == args


def test_the_abi_version_is_still_9(lib):
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9


def test_a_null_frame_is_refused_by_both_entry_points(lib):
    assert lib.bts_eval_frame_gt(None, None, None) == -1 and b"NULL frame" in lib.bts_last_error()
    assert lib.bts_eval_frame(None, None) == -1
