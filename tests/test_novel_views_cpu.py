"""CPU (no GPU, no kernel launches): the numpy restatement of csrc/bts_frames.hip (tests/_novel_views_oracle.py) reproduces the golden
fixture the reference wrote (tests/golden/novel_views.npz) byte for byte; the colour table resolves from a name and from an array; the
new symbols, the struct layout and the host-side error paths; FusedNovelViews says why a configuration is outside its envelope."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native, novel_views as NV
from behindthescenes_amd.build import build_library

from tests import _novel_views_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "novel_views.npz")
COLOUR_CASES = ("s", "a", "b", "c", "k", "m")
TABLES = ("magma", "plasma", "extremes")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("case", COLOUR_CASES)
def test_restatement_reproduces_the_golden_colours(gold, case):
    x = gold[f"col_{case}_x"]
    n = 0
    for name in TABLES:
        for norm in (0, 1):
            key = f"col_{case}_{name}_{norm}"
            if key + "_f64" not in gold:
                assert name == "extremes" and case not in ("a", "b")
                continue
            imgs = x if x.ndim == 3 else x[None]
            f64 = np.stack([NO.colorize(i, gold[f"lut_{name}"], norm=bool(norm)) for i in imgs])
            u8 = np.stack([NO.colorize_u8(i, gold[f"lut_{name}"], norm=bool(norm)) for i in imgs])
            want64, want8 = gold[key + "_f64"], gold[key + "_u8"]
            assert same_bits(f64 if x.ndim == 3 else f64[0], want64), key     # exact float64
            assert same_bits(u8 if x.ndim == 3 else u8[0], want8), key        # exact bytes
            n += 1
    assert n >= 4


def test_the_fixture_holds_the_cases_the_kernels_can_get_wrong(gold):
    a, lut = gold["col_a_x"], gold["lut_magma"]
    assert np.isnan(a).sum() == 1 and (a == 1).any() and (a == 0).any() and (a < 0).any()
    assert (a == np.nextafter(np.float32(1), np.float32(2))).any() and (a == np.float32(255.5 / 256)).any()
    assert lut.shape == (259, 4) and gold["lut_plasma"].shape == (259, 4)
    # a NaN anywhere makes the whole normalised image the bad colour; a constant image is 0 / 0
    assert (gold["col_a_extremes_1_f64"] == gold["lut_extremes"][258, :3]).all()
    assert (gold["col_k_magma_1_f64"] == lut[258, :3]).all() and (gold["col_s_magma_1_f64"] == lut[258, :3]).all()
    # the batch case: three ranges, each normalised on its own
    m = gold["col_m_x"]
    assert m.shape == (3, 7, 9) and m[1].min() > m[0].max() and m[2].max() < m[0].min()
    meta = json.loads(str(gold["meta"]))
    assert meta["matplotlib"] and all(v > 0 for v in meta["mutants"].values()) and set(meta["mutants"]) == {"fold", "nan_bad", "threshold64",
                                                                                                            "max_after"}
    for case in ("p", "q"):
        w = gold[f"fin_{case}_wsum"]
        t = np.float32(0.8)
        assert w.dtype == np.float32 and all((w == v).any() for v in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))))
        assert np.abs(gold[f"fin_{case}_wsum64"] - w).max() < 1e-6
    d, w = gold["fin_p_depth"], gold["fin_p_wsum"]
    assert w.reshape(-1)[d.argmax()] > np.float32(0.8)          # the maximum depth sits on an invalid pixel


@pytest.mark.parametrize("case,black_invalid", [("p", 0), ("p", 1), ("q", 0), ("q", 1)])
def test_restatement_reproduces_the_golden_frames_and_the_mutants_do_not(gold, case, black_invalid):
    g = {k: gold[f"fin_{case}_{k}"] for k in ("rgb", "depth", "wsum", "range")}
    d_min, d_max = (float(v) for v in g["range"])
    out = NO.finish(g["rgb"], g["depth"], g["wsum"], d_min, d_max, gold["lut_magma"], bool(black_invalid))
    canvas = np.concatenate((out["img_u8"], out["depth_u8"]), axis=0)
    assert same_bits(canvas, gold[f"fin_{case}_{black_invalid}_canvas"])
    assert same_bits(out["rgb"], gold[f"fin_{case}_{black_invalid}_rgb"]) and same_bits(out["depth"], gold[f"fin_{case}_{black_invalid}_depth"])
    if black_invalid:
        for k in ("threshold64", "max_after") if case == "p" else ("threshold64",):
            m = NO.finish(g["rgb"], g["depth"], g["wsum"], d_min, d_max, gold["lut_magma"], True, **{k: True})
            assert not np.array_equal(np.concatenate((m["img_u8"], m["depth_u8"]), axis=0), canvas), k
    m = NO.finish(g["rgb"], g["depth"], g["wsum"], d_min, d_max, gold["lut_magma"], bool(black_invalid), u8_fp32=True)
    assert np.array_equal(m["img_u8"], out["img_u8"])           # x 255 in fp32 is the same byte for every float32 in [0, 1]


def test_colour_mutants_change_the_golden(gold):
    x, lut = gold["col_a_x"], gold["lut_extremes"]
    want = gold["col_a_extremes_0_u8"]
    assert np.array_equal(NO.colorize_u8(x, lut), want)
    assert not np.array_equal(NO.colorize_u8(x, lut, fold=False), want) and not np.array_equal(NO.colorize_u8(x, lut, nan_bad=False), want)


def test_table_resolution_from_a_name_and_from_an_array(gold):
    matplotlib = pytest.importorskip("matplotlib")
    N, lut, lut_u8 = NV.cmap_table("magma")
    assert N == 256 and lut.shape == (259, 3) and lut.dtype == np.float64 and lut_u8.shape == (259, 3) and lut_u8.dtype == np.uint8
    if matplotlib.__version__ == json.loads(str(gold["meta"]))["matplotlib"]:
        assert same_bits(lut, np.ascontiguousarray(gold["lut_magma"][:, :3]))
    assert NV.cmap_table("magma") is NV.cmap_table("magma")                         # cached per name
    for table in (gold["lut_plasma"], gold["lut_plasma"][:, :3], torch.from_numpy(gold["lut_plasma"])):
        N2, lut2, u2 = NV.cmap_table(table)
        assert N2 == 256 and same_bits(lut2, np.ascontiguousarray(gold["lut_plasma"][:, :3]))
        assert np.array_equal(u2, NO.lut_u8(gold["lut_plasma"]))
    N3, lut3, _ = NV.cmap_table(np.linspace(0, 1, 7 * 3).reshape(7, 3))
    assert N3 == 4
    for bad in (np.zeros((3, 3)), np.zeros((8, 2)), np.zeros(12), "no_such_colour_map"):
        with pytest.raises(bts.BtsNativeError):
            NV.cmap_table(bad)


def test_symbols_and_the_struct_layout(lib):
    for name in ("bts_colorize", "bts_pack_u8", "bts_novel_views"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "bts_render.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(BtsNovelViews), offsetof(BtsNovelViews, lut_N), offsetof(BtsNovelViews, poses_c2w),
         offsetof(BtsNovelViews, frame_max), offsetof(BtsNovelViews, canvas), offsetof(BtsNovelViews, Hc), offsetof(BtsNovelViews, depth_col0),
         BTS_FRAMES_PARTIALS, BTS_CMAP_MAX_N);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    T = _lib.BtsNovelViews
    assert out == [C.sizeof(T), T.lut_N.offset, T.poses_c2w.offset, T.frame_max.offset, T.canvas.offset, T.Hc.offset, T.depth_col0.offset,
                   _lib.BTS_FRAMES_PARTIALS, _lib.BTS_CMAP_MAX_N]


def test_host_only_error_paths(lib):
    P = 16      # a non-NULL pointer value: everything below is refused before anything is enqueued
    assert lib.bts_colorize(None, 1, 4, 4, 0, 256, P, None, None, P, None, 0, 0, 0, 0, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_colorize(P, 1, 4, 4, 0, 256, None, None, None, P, None, 0, 0, 0, 0, None) == -1      # float64 output without its table
    assert lib.bts_colorize(P, 1, 4, 4, 1, 256, P, None, None, P, None, 0, 0, 0, 0, None) == -1          # norm without scratch
    assert lib.bts_colorize(P, 1, 4, 4, 0, 0, P, None, None, P, None, 0, 0, 0, 0, None) == -1 and b"table" in lib.bts_last_error()
    assert lib.bts_colorize(P, 1, 4, 4, 0, 256, None, P, None, None, P, 4, 7, 1, 0, None) == -1 and b"leaves the canvas" in lib.bts_last_error()
    assert lib.bts_pack_u8(P, 48, 12, 3, 1, 1, 4, 4, 1.0, 0.0, P, 8, 8, 5, 0, None) == -1 and b"leaves the canvas" in lib.bts_last_error()
    assert lib.bts_pack_u8(P, 48, 12, 3, 1, 1, 4, 4, 1.0, 0.0, None, 8, 8, 0, 0, None) == -1
    assert lib.bts_novel_views(None, None, None, None) == -1
    a = _lib.BtsNovelViews(P=1, h=4, w=4, K=8, rgb=P, depth=P, invalid_wsum=P, black_invalid=1, finish_only=1, img_row0=-1, depth_row0=-1)
    assert lib.bts_novel_views(None, None, C.byref(a), None) == -1 and b"frame_max" in lib.bts_last_error()
    a.black_invalid, a.canvas, a.Hc, a.Wc, a.img_row0, a.depth_row0 = 0, P, 8, 4, 0, 5
    assert lib.bts_novel_views(None, None, C.byref(a), None) == -1 and b"depth panel" in lib.bts_last_error()
    a.depth_row0 = 4
    assert lib.bts_novel_views(None, None, C.byref(a), None) == -1 and b"lut_u8" in lib.bts_last_error()
    # the render half: one encoded sample, one colour view, the projected map
    a.finish_only, a.canvas = 0, None
    tens = _lib.BtsFieldTensors(*([P] * 9))
    for n, nv in ((2, 1), (1, 2)):
        cfg = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=n, H=8, W=8, nv=nv)
        assert lib.bts_novel_views(C.byref(cfg), C.byref(tens), C.byref(a), None) == -2 and b"ONE" in lib.bts_last_error()
    cfg = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=8, W=8, nv=1)
    raw = _lib.BtsFieldTensors(P, None, P, P, P, P, P, P, P)
    assert lib.bts_novel_views(C.byref(cfg), C.byref(raw), C.byref(a), None) == -2 and b"proj_nhwc" in lib.bts_last_error()
    assert lib.bts_novel_views(C.byref(cfg), C.byref(tens), C.byref(a), None) == -1 and b"jitter" in lib.bts_last_error()


def test_cpu_tensors_and_bad_shapes_are_refused(gold):
    lut = gold["lut_magma"]
    with pytest.raises(bts.BtsNativeError, match="GPU"):
        NV.color_tensor(torch.zeros(4, 4), lut)                     # no fallback
    with pytest.raises(bts.BtsNativeError):
        NV.color_tensor(np.zeros((4, 4), dtype=np.float32), lut)
    canvas = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(bts.BtsNativeError, match="GPU"):
        NV.colorize_u8(torch.zeros(4, 4), lut, False, canvas)
    with pytest.raises(bts.BtsNativeError, match="GPU"):
        NV.pack_u8(torch.zeros(1, 3, 4, 4), canvas, channels_first=True)
    with pytest.raises(bts.BtsNativeError):
        native._req_canvas(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), 1, 4, 4, 0, 0, "image")


def _wrapped(n_fine=0, **kw):
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=False, code_mode="z",
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="feature_map", size=(8, 16), d_out=64),
                mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=64), mlp_fine=dict(type="empty"))
    net = bts.BTSNet(conf).eval()
    r = bts.NeRFRenderer.from_conf(dict(n_coarse=8, n_fine=n_fine, lindisp=True, hard_alpha_cap=True, **kw)).eval()
    return r.bind_parallel(net)


def test_fused_novel_views_says_why_not():
    smp = bts.ImageRaySampler(3.0, 80.0, 8, 16, norm_dir=False)
    w = _wrapped()
    nv = bts.FusedNovelViews(w, smp, cmap=np.zeros((259, 3)))
    assert "encode" in nv.why_not()                                 # no field state yet
    w.net._has_latents, w.net._grid_c_src = True, torch.zeros(1, 2, 3, 8, 16)
    assert "nv = 2" in nv.why_not()
    with pytest.raises(bts.BtsNativeError, match="nv = 2"):
        nv.frames(torch.eye(4)[None], torch.eye(3), 3.0, 80.0)
    with pytest.raises(bts.BtsNativeError, match="nv = 2"):
        bts.render_poses(w, smp, torch.eye(4).view(1, 1, 4, 4), torch.eye(3).view(1, 1, 3, 3))
    w.net._grid_c_src = torch.zeros(1, 1, 3, 8, 16)
    assert nv.why_not() is None
    with pytest.raises(bts.BtsNativeError, match="GPU"):            # the envelope is fine, the tensors are not
        nv.frames(torch.eye(4)[None], torch.eye(3), 3.0, 80.0)
    fine = _wrapped(n_fine=4)
    fine.net._has_latents, fine.net._grid_c_src = True, torch.zeros(1, 1, 3, 8, 16)
    assert "fine pass" in bts.FusedNovelViews(fine, smp, cmap=np.zeros((259, 3))).why_not()
    with pytest.raises(bts.BtsNativeError, match="fine pass"):
        bts.FusedNovelViews(fine, smp, cmap=np.zeros((259, 3))).frames(torch.eye(4)[None], torch.eye(3), 3.0, 80.0)
    assert "white" in bts.FusedNovelViews(_wrapped(white_bkgd=True), smp, cmap=np.zeros((259, 3))).why_not()
    assert "schedule" in bts.FusedNovelViews(_wrapped(sched=[[1], [8], [0]]), smp, cmap=np.zeros((259, 3))).why_not()
    with pytest.raises(bts.BtsNativeError):
        bts.FusedNovelViews(w, smp, cmap=np.zeros((259, 3)), poses_per_call=0)
    with pytest.raises(bts.BtsNativeError, match="layout"):
        nv.frames(torch.eye(4)[None], torch.eye(3), 3.0, 80.0, layout="depth_over_image")


@pytest.mark.needs_reference
def test_fixture_is_what_the_generator_writes(gold):
    """the committed fixture is the generator's output on the reference tree (same matplotlib version: its tables are the fixture's)"""
    matplotlib = pytest.importorskip("matplotlib")
    if matplotlib.__version__ != json.loads(str(gold["meta"]))["matplotlib"]:
        pytest.skip("another matplotlib version than the fixture was written with")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_novel_views", os.path.join(ROOT, "tests", "golden", "gen_golden_novel_views.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    arrays = gen.generate()
    assert set(arrays) == set(gold)
    for k, v in arrays.items():
        assert (str(v) == str(gold[k])) if k == "meta" else same_bits(np.asarray(v), gold[k]), k
    assert os.path.getsize(GOLDEN) < 300 * 1000
