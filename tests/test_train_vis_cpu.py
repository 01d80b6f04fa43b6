"""CPU (no GPU, no kernel launches): the torch restatement of csrc/bts_train_vis.hip (tests/_train_vis_oracle.py) reproduces the fields
and panels the reference's ``visualize`` wrote into tests/golden/train_vis.npz bit for bit, and each of its mutants leaves the GPU
test's bar; the new struct's layout against the C compiler, the new symbols with ABI 9, every entry check with its code and message
before anything is launched; ``vis_panels`` refuses what it cannot run; ``visualize`` logs the reference's tags in its order."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, train_vis as TV
from behindthescenes_amd.build import build_library

from tests import _train_vis_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_vis.npz")
CASES = ("a", "b", "c", "d", "z")
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def meta(gold):
    return json.loads(str(gold["meta"]))


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def inputs(gold, meta, case):
    stored = {k: gold[f"{case}_{k}"] for k in ("imgs", "rgb", "alphas", "invalid", "depth")}
    return TO.decode(stored, meta["cases"][case]["v"], agree=TO.Z_AGREE if case == "z" else None)


def run_oracle(x, meta, **kw):
    return TO.evaluate(x["imgs"], x["rgb"], x["depth"], x["alphas"], x["invalid"], meta["z_near"], meta["z_far"], **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(gold, meta, case):
    info = meta["cases"][case]
    x = inputs(gold, meta, case)
    before = {k: v.copy() for k, v in x.items()}
    mine = run_oracle(x, meta)
    assert all(same_bits(before[k], x[k]) for k in x)                  # the restatement does not edit its inputs either
    T, S, N, lut = info["T"], info["S"], gold["lut_plasma"].shape[0] - 3, gold["lut_plasma"]
    assert T == min(info["v"], 6) and mine["input_im"].shape == (T, 3, info["h"], info["w"])
    for k in ["recon_im", "f_mse", "f_profile", "f_entropy", "f_alpha_sum", "f_invalid"] + [f"f_depth_{s}" for s in range(S)]:
        assert same_bits(mine[k], gold[f"{case}_{k}"]), (case, k)      # exact float32
    assert mine["f_profile"].shape == (3 * T, info["K"], info["w"])
    for tag, f in TO.coloured(S).items():
        idx = gold[f"{case}_{tag}_idx"]
        assert np.array_equal(TO.colour_indices(mine[f], N), idx), (case, tag)
        panel = TO.panel_from_indices(idx, lut)
        assert panel.dtype == np.float64 and panel.shape == idx.shape[:-2] + (3,) + idx.shape[-2:]
    # the fp64 evaluation lies where the generator measured it
    exact = run_oracle(x, meta, dtype=torch.float64)
    for k, d in info["D"].items():
        with np.errstate(invalid="ignore"):
            gap = np.abs(mine[k].astype(np.float64) - exact[k])
        assert (np.nanmax(gap) if np.isfinite(gap).any() else 0.0) == d, (case, k)


def test_the_fixture_holds_the_cases_the_kernels_can_get_wrong(gold, meta):
    c = meta["cases"]
    assert (c["a"]["K"], c["b"]["K"], c["c"]["K"], c["d"]["K"]) == (8, 48, 64, 96) and c["b"]["v"] == 7 and c["b"]["T"] == 6
    assert c["c"]["w"] > 64 and c["b"]["S"] == 2 and c["b"]["nv"] == 3 and c["d"]["T"] == 1
    assert all(s <= 0.02 for info in c.values() for s in info["share"].values())
    N = gold["lut_plasma"].shape[0] - 3
    assert (gold["z_depth_profile_idx"] == N + 2).all()                                      # 0 / 0: the bad colour everywhere
    assert gold["z_recon_depth_0_idx"][TO.Z_DEPTH_ZERO] == N - 1 and gold["z_recon_depth_0_idx"][TO.Z_DEPTH_NAN] == N + 2
    assert gold["z_f_entropy"][TO.Z_ALPHAS_ZERO] == pytest.approx(np.log(2), abs=1e-6)
    assert gold["z_f_invalid"][TO.Z_ALL_INVALID] == 1.0 and gold["z_invalids_idx"][TO.Z_ALL_INVALID] == N - 1
    assert gold["z_f_mse"][TO.Z_AGREE] == 0.0 and gold["z_recon_mse_idx"][TO.Z_AGREE] == 0
    for case in ("a", "b", "c"):                                                             # both clamps of the depth are hit
        idx = gold[f"{case}_recon_depth_0_idx"]
        assert (idx == N - 1).any() and (gold[f"{case}_f_depth_0"] == 0).any()
    assert (inputs(gold, meta, "b")["alphas"] < 0).any()                                     # clamp_min has something to clamp
    assert os.path.getsize(GOLDEN) <= 1 << 20


def test_every_mutant_leaves_the_bar(gold, meta):
    worst = {m: 0.0 for m in TO.MUTANTS}
    for case in CASES:
        x = inputs(gold, meta, case)
        exact = run_oracle(x, meta, dtype=torch.float64)
        for m in TO.MUTANTS:
            mut = run_oracle(x, meta, mutant=m)
            for k, d in meta["cases"][case]["D"].items():
                if k == "recon_im":
                    continue
                bar = max(4 * d, EPS32)
                with np.errstate(invalid="ignore"):
                    diff = np.abs(mut[k].astype(np.float64) - exact[k])
                diff = np.where(np.isnan(mut[k]) & np.isnan(exact[k]), 0.0, np.where(np.isnan(diff), np.inf, diff))
                worst[m] = max(worst[m], float(diff.max() / bar))
    assert all(v > 1.0 for v in worst.values()), worst
    assert set(meta["mutants"]) == set(TO.MUTANTS) and all(v > 1.0 for v in meta["mutants"].values())
    with pytest.raises(AssertionError):
        run_oracle(inputs(gold, meta, "a"), meta, mutant="no_such_mutant")


def test_the_new_struct_matches_the_c_layout():
    T = _lib.BtsTrainVis
    fields = [f[0] for f in T._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu", sizeof(BtsTrainVis));\n' + \
        "".join(f'  printf(" %zu", offsetof(BtsTrainVis, {f}));\n' for f in fields) + \
        '  printf(" %d %d", BTS_ABI_VERSION, BTS_TRAIN_VIS_MAX_FRAMES);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(T)] + [getattr(T, f).offset for f in fields] + [9, _lib.BTS_TRAIN_VIS_MAX_FRAMES]
    assert T.imgs.size == 6 * C.sizeof(C.c_void_p) and T.depth.size == _lib.BTS_MAX_SCALES * C.sizeof(C.c_void_p)


def test_symbols_export_and_the_abi_version_stays(lib):
    for name in ("bts_train_vis", "bts_train_vis_workspace"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    assert "vis_panels" in bts.__all__ and "visualize" in bts.__all__ and bts.vis_panels is TV.vis_panels


def test_workspace_size(lib):
    ws = lib.bts_train_vis_workspace
    assert ws(6, 192, 640, 64) > 0 and ws(1, 4, 9, 96) > 0 and ws(6, 192, 1280, 64) >= ws(6, 192, 640, 64) >= ws(1, 192, 640, 64)
    for bad in ((0, 8, 8, 8), (7, 8, 8, 8), (2, 8, 8, 1), (2, 8, 8, 257), (2, 0, 8, 8), (2, 8, 8193, 8)):
        assert ws(*bad) == 0, bad


def _args(**over):
    P = 16      # a non-NULL pointer value: everything below is refused before anything is enqueued
    a = _lib.BtsTrainVis(T=2, v=2, h=8, w=12, K=8, nv=1, S=1, lut_N=256, z_near=3.0, z_far=80.0, rgb=P, alphas=P, invalid=P, lut=P,
                         workspace=P, workspace_bytes=1 << 20)
    a.imgs[0] = a.imgs[1] = P
    a.depth[0] = P
    for k in ("input_im", "recon_im", "recon_depth", "depth_profile", "ray_entropy", "alpha_sum", "recon_mse", "invalids"):
        setattr(a, k, P)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_argument_errors_are_codes_with_messages(lib):
    def refused(a, code, *words):
        assert lib.bts_train_vis(C.byref(a) if a is not None else None, None) == code
        msg = lib.bts_last_error()
        assert msg.startswith(b"bts_train_vis") and all(w in msg for w in words), msg
    refused(None, -1, b"NULL")
    for T in (0, 7):
        refused(_args(T=T, v=8), -1, b"T=")
    refused(_args(T=2, v=1), -1, b"T=", b"v = 1")
    for K in (1, 257):
        refused(_args(K=K), -1, b"K=")
    for nv in (0, _lib.BTS_MAX_VIEWS + 1):
        refused(_args(nv=nv), -1, b"nv=")
    for S in (0, _lib.BTS_MAX_SCALES + 1):
        refused(_args(S=S), -1, b"S=")
    refused(_args(h=0), -1, b"h=0")
    refused(_args(w=8193), -1, b"w=8193")
    refused(_args(lut_N=0), -1, b"table", b"lut_N=0")
    refused(_args(lut=None), -1, b"table")
    a = _args()
    a.imgs[1] = None
    refused(a, -1, b"imgs[1]")
    a = _args()
    a.depth[0] = None
    refused(a, -1, b"depth[0]")
    for k in ("rgb", "alphas", "invalid"):
        refused(_args(**{k: None}), -1, b"NULL", b"inputs")
    for k in ("input_im", "depth_profile", "invalids"):
        refused(_args(**{k: None}), -1, b"NULL", b"output")
    refused(_args(workspace=None), -4, b"workspace")
    refused(_args(workspace_bytes=8), -4, b"workspace")
    refused(_args(workspace=24), -4, b"16-byte")
    # the optional pointers may be NULL: the fields, the device pair of z_near / z_far, imgs past T, depth past S (nothing above tripped)
    assert _args().f_depth is None and _args().z_near_far is None


def _data(device="cpu", v=2, h=4, w=6, K=8, nv=1, S=1, n_imgs=None):
    part = dict(alphas=torch.rand(1, v, h, w, K, device=device), invalid=torch.zeros(1, v, h, w, K, nv, device=device))
    fine = [dict(rgb=torch.rand(1, v, h, w, nv, 3, device=device), depth=torch.rand(1, v, h, w, device=device) + 3) for _ in range(S)]
    return dict(imgs=[torch.rand(1, 3, h, w, device=device) for _ in range(v if n_imgs is None else n_imgs)], coarse=[part], fine=fine,
                z_near=3.0, z_far=80.0)


def test_vis_panels_refuses_what_it_cannot_run():
    lut = np.linspace(0, 1, 259 * 3).reshape(259, 3)
    with pytest.raises(bts.BtsNativeError, match="GPU"):
        TV.vis_panels(_data(), cmap=lut)                               # no fallback
    lean = _data()
    del lean["coarse"][0]["alphas"]
    with pytest.raises(KeyError, match="want_alphas"):
        TV.vis_panels(lean, cmap=lut)
    lean["coarse"][0]["alphas"] = None
    with pytest.raises(KeyError, match="want_alphas"):
        TV.vis_panels(lean, cmap=lut)
    with pytest.raises(bts.BtsNativeError):
        TV.vis_panels(dict(_data(), coarse=[dict(alphas=np.zeros((1, 2, 4, 6, 8)), invalid=np.zeros((1, 2, 4, 6, 8, 1)))]), cmap=lut)


def test_visualize_logs_the_reference_tags_in_its_order(gold, meta, monkeypatch):
    case, seen, calls = "b", {}, []
    info = meta["cases"][case]
    x = inputs(gold, meta, case)

    def oracle_panels(data, cmap="plasma", fields=False):
        seen["data"], seen["cmap"], seen["fields"] = data, cmap, fields
        f = run_oracle(x, meta)
        out = dict(input_im=torch.from_numpy(f["input_im"]), recon_im=torch.from_numpy(f["recon_im"]))
        for tag, p in TO.panels(f, gold["lut_plasma"], info["S"]).items():
            out[tag] = torch.from_numpy(p.astype(np.float32))
        return dict(reversed(list(out.items())))                       # the order of the dict must not matter
    monkeypatch.setattr(TV, "vis_panels", oracle_panels)

    def make_grid(panel, nrow):
        calls.append(("grid", tuple(panel.shape), nrow))
        return panel

    class Writer:
        def add_image(self, tag, img, global_step):
            assert isinstance(img, torch.Tensor) and img.device.type == "cpu"
            calls.append(("image", tag, tuple(img.shape), global_step))

    class Holder:
        pass
    engine, logger = Holder(), Holder()
    engine.state = Holder()
    engine.state.output = dict(output="the trainer's dict")
    logger.writer = Writer()
    TV.visualize(engine, logger, 11, "val", make_grid=make_grid)
    assert seen == dict(data="the trainer's dict", cmap="plasma", fields=False)
    T, h, w, K = info["T"], info["h"], info["w"], info["K"]
    tags = ["input_im", "recon_im", "recon_depth_0", "recon_depth_1", "depth_profile", "ray_entropy", "alpha_sum", "recon_mse", "invalids"]
    shapes = [(3 * T, 3, K, w) if t == "depth_profile" else (T, 3, h, w) for t in tags]
    # every grid first (trainer.py:489-496), then every image (:498-506), both in the reference's order
    want = [("grid", s, int(T ** .5)) for s in shapes] + [("image", f"val/{t}", s, 11) for t, s in zip(tags, shapes)]
    assert calls == want and int(T ** .5) == 2


@pytest.mark.needs_reference
def test_fixture_is_what_the_generator_writes(gold):
    """the committed fixture is the generator's output on the reference tree (same matplotlib version: its table is the fixture's)"""
    matplotlib = pytest.importorskip("matplotlib")
    if matplotlib.__version__ != json.loads(str(gold["meta"]))["matplotlib"]:
        pytest.skip("another matplotlib version than the fixture was written with")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_train_vis", os.path.join(ROOT, "tests", "golden", "gen_golden_train_vis.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    arrays = gen.generate()
    assert set(arrays) == set(gold)
    for k, v in arrays.items():
        assert (str(v) == str(gold[k])) if k == "meta" else same_bits(np.asarray(v), gold[k]), k
