"""CPU (no GPU): bts_eval_frame_prep -- the evaluation frame whose projection launch also packs and stages the MLP, fed with the MLP's parameter tensors
instead of a packed vector -- is additive to ABI 9: declared in include/bts_render.h, bound in _lib.py, exported by the built library;
its argument checks refuse what its siblings refuse, with their texts, before anything is launched."""
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


def _frame(**kw):
    """a BtsEvalFrame whose every pointer is a (never dereferenced) non-NULL value: the checks run on the host and nothing is launched
    when one of them refuses"""
    fr = _lib.BtsEvalFrame()
    fr.cfg = _lib.BtsFieldCfg(n=1, H=16, W=24, C=64, d_hidden=64, n_blocks=0, nv=1, num_freqs=6, code_mode=0, inv_z=1, learn_empty=1, empty_empty=0,
                              freq_factor=1.5, d_min=3.0, d_max=80.0, feat_shift=0, enc_render_view=0, tile_blocks=0)
    fr.v, fr.id_encoder, fr.K, fr.lindisp, fr.hard_alpha_cap, fr.norm_dir = 2, 0, 64, 1, 1, 1
    fr.z_near, fr.z_far, fr.img_scale, fr.img_shift = 3.0, 80.0, 0.5, 0.5
    for k in ("images", "Ks", "poses_c2w", "feat_nchw", "empty_feature", "jitter", "cams", "imgs_nhwc4", "proj_nhwc", "inv_K", "rays", "rgb", "depth",
              "depth_z", "weights", "alphas", "invalid"):
        setattr(fr, k, 0x1000)
    for k, v in kw.items():
        if k.startswith("cfg_"):
            setattr(fr.cfg, k[4:], v)
        else:
            setattr(fr, k, v)
    return fr


def _tensors(n=4):
    mt = _lib.BtsMlpTensors()
    mt.n_tensors = n
    for i in range(min(n, _lib.BTS_MLP_MAX_TENSORS)):
        mt.tensor[i] = 0x1000
    return mt


def _call(lib, fr, mt=None, packed=0x1000, image=0x1000):
    rc = lib.bts_eval_frame_prep(None if fr is None else C.byref(fr), None, None, None if mt is None else C.byref(mt), packed, image, None)
    return rc, lib.bts_last_error().decode()


def test_bts_eval_frame_prep_is_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+bts_eval_frame_prep\s*\(([^)]*)\)\s*;", src)
    assert m, "bts_eval_frame_prep is not declared in include/bts_render.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.rsplit(" ", 1)[0] for p in params] == ["const BtsEvalFrame*", "float*", "uint32_t*", "const BtsMlpTensors*", "float*", "float*", "void*"]
    res, args = _lib.SYMBOLS["bts_eval_frame_prep"]
    assert res is C.c_int and len(args) == 7 and args[0] is C.POINTER(_lib.BtsEvalFrame) and args[3] is C.POINTER(_lib.BtsMlpTensors)
    assert hasattr(lib, "bts_eval_frame_prep") and lib.bts_eval_frame_prep.argtypes == args
    assert re.search(r"\bint64_t\s+bts_mlp_image_floats\s*\(\s*const BtsFieldCfg\*\s*\w+\s*\)\s*;", src) and hasattr(lib, "bts_mlp_image_floats")
    # the siblings stay, and so does the version
    for name in ("bts_eval_frame", "bts_eval_frame_gt", "bts_eval_frame_sched"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src) and hasattr(lib, name)
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    # the struct of the parameter list as the header lays it out
    m = re.search(r"#define\s+BTS_MLP_MAX_TENSORS\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.BTS_MLP_MAX_TENSORS
    assert C.sizeof(_lib.BtsMlpTensors) == 8 * _lib.BTS_MLP_MAX_TENSORS + 8


def test_the_image_size_follows_the_compiled_shapes(lib):
    def floats(C_, HD, NB):
        cfg = _lib.BtsFieldCfg(C=C_, d_hidden=HD, n_blocks=NB, num_freqs=6)
        return int(lib.bts_mlp_image_floats(C.byref(cfg)))
    # Lds<C, HD, NB, true> (40 k-major rows of lin_in, the blocks, lin_out, the projected empty feature) + LdsH (raw rows, split-f16 weights, block biases,
    # empty feature, scale, split-f16 block weights), each a multiple of four floats at these shapes
    for C_, HD, NB in ((64, 64, 0), (32, 32, 1), (32, 32, 0)):
        fp32 = 40 * HD + NB * (2 * HD * HD + 2 * HD) + HD + HD
        f16 = 4 * HD + 2 * 3 * (HD // 32) * 256 + NB * 2 * HD + HD + 4 + NB * 2 * 2 * 512
        assert floats(C_, HD, NB) == fp32 + f16, (C_, HD, NB)
    assert floats(64, 64, 0) * 4 == 24336
    assert floats(48, 64, 0) == 0 and floats(64, 64, 1) == 0 and int(lib.bts_mlp_image_floats(None)) == 0


def test_null_and_odd_arguments_are_refused_with_the_siblings_texts(lib):
    rc, msg = _call(lib, None)
    assert rc == -1 and msg == "bts_eval_frame_prep: NULL frame"
    # the same frames through bts_eval_frame_sched give the same text behind the sibling's name
    cases = [
        (dict(K=0), -1, "non-positive size or more than 8 render views (n=1, v=2, K=0)"),
        (dict(cfg_nv=9), -1, "non-positive size or more than 8 render views (n=1, v=2, K=64)"),
        (dict(cfg_C=48), -2, "configuration outside the compiled envelope (C=48 d_hidden=64 n_blocks=0)"),
        (dict(cfg_n_blocks=1), -2, "configuration outside the compiled envelope (C=64 d_hidden=64 n_blocks=1)"),
        (dict(id_encoder=2), -1, "a frame id outside [0, v=2) or enc_render_view out of range"),
        (dict(cfg_enc_render_view=1), -1, "a frame id outside [0, v=2) or enc_render_view out of range"),
        (dict(jitter=None), -1, "NULL input / output / scratch pointer"),
        (dict(proj_nhwc=None), -1, "NULL input / output / scratch pointer"),
        (dict(empty_feature=None), -1, "NULL input / output / scratch pointer"),
        (dict(cfg_H=1 << 15, cfg_W=1 << 15), -2, "too many rays in one call (2147483648)"),
    ]
    for kw, code, text in cases:
        rc, msg = _call(lib, _frame(**kw), _tensors())
        assert rc == code and msg == "bts_eval_frame_prep: " + text, (kw, rc, msg)
        sib = _frame(mlp_params=0x1000, **kw)
        rc2 = lib.bts_eval_frame_sched(C.byref(sib), None, None, None)
        assert rc2 == code and lib.bts_last_error().decode() == "bts_eval_frame: " + text, kw
    # mlp_params is what the siblings need and this entry point does not read
    sib = _frame()
    assert lib.bts_eval_frame_sched(C.byref(sib), None, None, None) == -1 and b"NULL input / output / scratch pointer" in lib.bts_last_error()
    # its own arguments: the parameter list, its length, its entries, the packed scratch, the image's alignment
    for mt, packed, image, text in ((None, 0x1000, 0x1000, "NULL input / output / scratch pointer"),
                                    (_tensors(), None, 0x1000, "NULL input / output / scratch pointer"),
                                    (_tensors(8), 0x1000, 0x1000, "n_tensors=8, the MLP has 4 parameter tensors (4 + 4 * n_blocks)"),
                                    (_tensors(3), 0x1000, 0x1000, "n_tensors=3, the MLP has 4 parameter tensors (4 + 4 * n_blocks)"),
                                    (_tensors(), 0x1000, 0x1004, "mlp_image must be 16-byte aligned (the render's work-groups copy it with 16-byte loads)")):
        rc, msg = _call(lib, _frame(), mt, packed, image)
        assert rc == -1 and msg == "bts_eval_frame_prep: " + text, (rc, msg)
    mt = _tensors()
    mt.tensor[2] = None
    rc, msg = _call(lib, _frame(), mt)
    assert rc == -1 and msg == "bts_eval_frame_prep: NULL input / output / scratch pointer"
