"""CPU (no GPU): the host's test for the pinned set (PinnedSet::matches of bts_field_kernel.h through the exported bts_render_pinned) --
true for the render launch of the shipped KITTI eval configuration, false for every near miss, so that such a launch keeps the general
kernel."""
import ctypes as C
import re
from pathlib import Path

import pytest

from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library
from tests._pinned_helpers import frame_launch, pinned


@pytest.fixture(scope="module", autouse=True)
def lib():
    build_library()
    return _lib.load()


def test_the_shipped_eval_configuration_is_the_pinned_set():
    assert pinned() == 1
    # sizes, the batch and the second compiled shape without blocks stay run-time values
    assert pinned(n=2) == 1 and pinned(H=192, W=640) == 1 and pinned(v=1) == 1 and pinned(C_=32, d_hidden=32) == 1
    assert pinned(hard_alpha_cap=2) == 1 and pinned(lindisp=7) == 1      # (the kernels test these against zero)


NEAR_MISSES = [
    dict(K=48), dict(K=56), dict(K=65), dict(K=128), dict(hard_alpha_cap=0), dict(learn_empty=0), dict(weights=False), dict(alphas=False),
    dict(invalid=False), dict(enc_view=-1), dict(nv=2), dict(nv=2, enc_view=1), dict(nv=0, enc_view=-1), dict(lindisp=0), dict(code_mode=1),
    dict(inv_z=0), dict(empty_empty=1), dict(feat_shift=1), dict(white_bkgd=1), dict(z_samp=True), dict(z_samp_out=True), dict(sigma_noise=True),
    dict(rgb_samps=True), dict(sigma_raw=True), dict(trans=True), dict(invalid_wsum=True),
    dict(K=32, v=2),      # short rays share a wave iteration: not a one-ray launch
]


@pytest.mark.parametrize("miss", NEAR_MISSES, ids=lambda m: ",".join(f"{k}={v}" for k, v in m.items()))
def test_a_near_miss_is_not(miss):
    assert pinned(**miss) == 0


def test_null_arguments(lib):
    cfg, t, a = frame_launch()
    assert lib.bts_render_pinned(None, C.byref(t), C.byref(a)) == -1
    assert lib.bts_render_pinned(C.byref(cfg), None, C.byref(a)) == -1
    assert lib.bts_render_pinned(C.byref(cfg), C.byref(t), None) == -1


def test_declared_bound_and_exported(lib):
    src = (Path(__file__).resolve().parents[1] / "include" / "bts_render.h").read_text()
    assert re.search(r"\bint32_t\s+bts_render_pinned\s*\(\s*const BtsFieldCfg\*\s*cfg,\s*const BtsFieldTensors\*\s*t,\s*const BtsRenderArgs\*\s*a\)\s*;", src)
    m = re.search(r"\bint\s+bts_eval_frame_prep_unpinned\s*\(([^)]*)\)\s*;", src)
    p = re.search(r"\bint\s+bts_eval_frame_prep\s*\(([^)]*)\)\s*;", src)
    assert m and p and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", p.group(1))     # the same arguments as bts_eval_frame_prep
    assert _lib.SYMBOLS["bts_eval_frame_prep_unpinned"] == _lib.SYMBOLS["bts_eval_frame_prep"]
    assert hasattr(lib, "bts_render_pinned") and hasattr(lib, "bts_eval_frame_prep_unpinned")
    assert re.search(r"#define BTS_ABI_VERSION 9\b", src)       # additive: the ABI and the structs are what they were
