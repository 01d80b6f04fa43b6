"""Writes tests/golden/train_vis.npz FROM THE REAL REFERENCE, on CPU tensors: the trainer's ``visualize`` (models/bts/trainer.py:430-506;
the module itself cannot be imported -- ignite, hydra, the datasets -- so the function's source is compiled from the file) is run with

  * the reference's own ``utils.plotting.color_tensor``, wrapped so that every scalar field it is handed is recorded,
  * a ``make_grid`` stand-in that records its argument and returns it,
  * a writer that records ``add_image``,

on a dict shaped like the trainer's output.  The fixture below was written with matplotlib 3.10.8 (the version is in its ``meta``).

    python tests/golden/gen_golden_train_vis.py

Stored per case: the inputs, the six recorded fields (float32, bit for bit), ``recon_im``, and every colour panel as the table's row
index per pixel plus the table -- asserted here to reproduce the reference's float64 panel bit for bit (``table[index]``).  To stay
under 1 MiB the dense inputs are stored as byte codes that ``tests/_train_vis_oracle.py``'s restatement decodes the way this file does
(``decode``): image (c / 127.5 - 1), colour (c / 255), alpha ((c / 255)^2, code 1 = -0.01: the clamp_min), invalid (c / 255: one level
per ray and view from a first invalid sample on -- the run structure of a real render, with a soft level so that the mean does not sit
on a colour step).  Only the first T = min(v, 6) frames are stored: case b's seventh frame is a copy of frame 0 for the reference and is
never read by it.

Cases (the smallest shapes at which the kernels can still go wrong):
  a  v = 2, 8 x 12, K = 8, nv = 1, S = 1      eight pixels per wave; T = 2
  b  v = 7, 13 x 37, K = 48, nv = 3, S = 2    T = 6 < v; K padded to 64; ragged in every direction
  c  v = 3, 5 x 70, K = 64, nv = 2, S = 1     one pixel per wave; w spans two transpose tiles
  d  v = 1, 4 x 9, K = 96, nv = 1, S = 1      the strided K loop; T = 1
  z  the shape of a with specials: the three profile rows all zero (the whole profile 0 / 0, the bad colour), a depth of 0, a NaN
     depth, a pixel with all-zero alphas (entropy ln 2), a pixel invalid in every sample and view (1.0 folds to N - 1), a pixel
     where input and reconstruction agree

Asserted here, on the reference alone, with the numbers in ``meta``: the fp32 restatement reproduces the recorded fields; D_f = per
case and field the largest distance of the reference's fp32 field from the fp64 evaluation; per panel at most 2 % of the pixels lie
within the band (2 x the GPU test's bar max(4 D_f, 2^-23), i.e. 8 D_f) of a colour step; every mutant of the restatement leaves the bar
on at least one case."""
import ast
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle.ref_shim import REFERENCE_ROOT, reference_available
from tests import _train_vis_oracle as TO

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_vis.npz")
CASES = dict(a=dict(v=2, h=8, w=12, K=8, nv=1, S=1), b=dict(v=7, h=13, w=37, K=48, nv=3, S=2), c=dict(v=3, h=5, w=70, K=64, nv=2, S=1),
             d=dict(v=1, h=4, w=9, K=96, nv=1, S=1), z=dict(v=2, h=8, w=12, K=8, nv=1, S=1))
Z_NEAR, Z_FAR = 3.0, 80.0
EPS32 = float(np.finfo(np.float32).eps)
MAX_SHARE = 0.02


def reference_visualize():
    """-> run(data) -> (fields recorded by color_tensor, make_grid's arguments, add_image's (tag, image, step) list)"""
    assert reference_available(), f"reference tree not found at {REFERENCE_ROOT}"
    sys.dont_write_bytecode = True
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    from utils.plotting import color_tensor
    src = open(os.path.join(REFERENCE_ROOT, "models", "bts", "trainer.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "visualize")
    rec = dict(fields=[], grids=[], images=[])

    def recording_color_tensor(tensor, cmap, norm=False):
        assert cmap == "plasma" and not norm
        rec["fields"].append(np.ascontiguousarray(tensor.detach().clone().numpy()))
        return color_tensor(tensor, cmap, norm)

    def make_grid(x, nrow):
        rec["grids"].append((x.detach().clone().numpy(), nrow))
        return x

    class Writer:
        def add_image(self, tag, img, global_step):
            rec["images"].append((tag, img.numpy(), global_step))

    class Holder:
        pass
    ns = dict(torch=torch, math=math, color_tensor=recording_color_tensor, make_grid=make_grid, Engine=object, TensorboardLogger=object)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "trainer.py", "exec"), ns)

    def run(data):
        for v in rec.values():
            v.clear()
        engine, logger = Holder(), Holder()
        engine.state = Holder()
        engine.state.output = dict(output=data)
        logger.writer = Writer()
        ns["visualize"](engine, logger, 7, "vis")
        return list(rec["fields"]), list(rec["grids"]), list(rec["images"])
    return run


def codes(case):
    """the stored inputs of a case: byte codes (first T frames) and the float32 depths"""
    c = CASES[case]
    v, h, w, K, nv, S = (c[k] for k in ("v", "h", "w", "K", "nv", "S"))
    T = min(v, 6)
    rng = np.random.default_rng(dict(a=31, b=32, c=33, d=34, z=35)[case])
    imgs = rng.integers(0, 256, (T, 3, h, w), dtype=np.uint8)
    rgb = rng.integers(0, 256, (T, h, w, nv, 3), dtype=np.uint8)
    alphas = rng.integers(1, 256, (T, h, w, K), dtype=np.uint8)       # (code 0, exactly 0, is case z's)
    for f in range(T):          # every frame its own maximum (ONE profile maximum differs from one per frame), none of them 1.0
        alphas[f] = 1 + (alphas[f].astype(np.int64) - 1) * (249 - 20 * f) // 254       # codes 1 .. 250 - 20 f, spread evenly
    k0 = rng.integers(0, K,(T, h, w, 1, nv))      # (at least one invalid sample: a mean of exactly 0 sits on a colour step)
    level = rng.integers(60, 256, (T, h, w, 1, nv))
    invalid = np.where(np.arange(K).reshape(1, 1, 1, K, 1) >= k0, level, 0).astype(np.uint8)
    depth = (Z_NEAR + 0.2 + (Z_FAR - Z_NEAR - 0.4) * rng.random((S, T, h, w)) ** 2).astype(np.float32)
    if T * h * w >= 150:        # (both clamp to a colour step exactly: two pixels of case d's 36 would be more than the 2 % set aside)
        depth[:, 0, 0, 2], depth[:, 0, 0, 3] = 2.5, 95.0              # nearer than z_near (-> 1), farther than z_far (-> 0)
    if case == "z":
        rows = TO.profile_rows(h)
        alphas[:, rows] = 0                                           # the whole profile 0 / 0
        depth[(0,) + TO.Z_DEPTH_ZERO], depth[(0,) + TO.Z_DEPTH_NAN] = 0.0, np.nan
        alphas[TO.Z_ALPHAS_ZERO] = 0                                  # uniform p: entropy ln 2 = ln 8 / log2 8
        invalid[TO.Z_ALL_INVALID] = 255                               # 1.0 -> N - 1
        assert all(p[1] not in rows for p in (TO.Z_ALPHAS_ZERO, TO.Z_ALL_INVALID, TO.Z_AGREE))
        # (input == reconstruction at Z_AGREE: decode(agree=) gives that pixel's rgb the image's colour, a float no byte code holds)
    return dict(imgs=imgs, rgb=rgb, alphas=alphas, invalid=invalid, depth=depth)


def generate():
    import matplotlib
    run = reference_visualize()
    cm = matplotlib.colormaps["plasma"]
    cm._init()
    lut = np.array(cm._lut, dtype=np.float64)
    N = lut.shape[0] - 3
    arrays, meta = dict(lut_plasma=lut), dict(matplotlib=matplotlib.__version__, cases={}, z_near=Z_NEAR, z_far=Z_FAR)
    gaps = {m: 0.0 for m in TO.MUTANTS}
    for case, shape in CASES.items():
        stored = codes(case)
        x = TO.decode(stored, shape["v"], agree=TO.Z_AGREE if case == "z" else None)
        S, v, T = shape["S"], shape["v"], min(shape["v"], 6)
        tt = lambda a: torch.from_numpy(np.array(a))          # noqa: E731
        part = dict(alphas=tt(x["alphas"])[None], invalid=tt(x["invalid"])[None])
        data = dict(imgs=[tt(x["imgs"][i])[None] for i in range(v)], coarse=[part],
                    fine=[dict(rgb=tt(x["rgb"])[None], depth=tt(x["depth"][s])[None]) for s in range(S)],
                    z_near=torch.tensor(Z_NEAR), z_far=torch.tensor(Z_FAR))
        with np.errstate(all="ignore"):
            fields, grids, images = run(data)
        # the reference's order: color_tensor on mse, the S depths, profile, entropy, alpha sum, invalids
        names = ["f_mse"] + [f"f_depth_{s}" for s in range(S)] + ["f_profile", "f_entropy", "f_alpha_sum", "f_invalid"]
        assert len(fields) == len(names) and all(f.dtype == np.float32 for f in fields)
        ref = dict(zip(names, fields))
        tags = ["input_im", "recon_im"] + [f"recon_depth_{s}" for s in range(S)] + ["depth_profile", "ray_entropy", "alpha_sum", "recon_mse",
                                                                                      "invalids"]
        assert [t for t, _, _ in images] == ["vis/" + t for t in tags] and all(step == 7 for _, _, step in images)
        assert all(nrow == int(T ** .5) for _, nrow in grids) and len(grids) == len(tags)
        shown = {t[4:]: img for t, img, _ in images}
        # the reference edits the caller's alphas in place; the copy it was handed shows it, the stored inputs do not
        assert not np.array_equal(part["alphas"].numpy()[0, :T], x["alphas"][:T])
        mine32 = TO.evaluate(x["imgs"], x["rgb"], x["depth"], x["alphas"], x["invalid"], Z_NEAR, Z_FAR)
        mine64 = TO.evaluate(x["imgs"], x["rgb"], x["depth"], x["alphas"], x["invalid"], Z_NEAR, Z_FAR, dtype=torch.float64)
        for k in names + ["input_im", "recon_im"]:
            want = ref[k] if k in ref else shown[k]
            assert want.dtype == np.float32 and want.shape == mine32[k].shape, (case, k, want.shape, mine32[k].shape)
            assert np.array_equal(want.view(np.uint32), mine32[k].view(np.uint32)), (case, k)      # the fp32 restatement IS the reference
        info = dict(shape, T=T, D={}, share={})
        for k in names + ["recon_im"]:
            want, exact = (ref[k] if k in ref else shown[k]).astype(np.float64), mine64[k]
            assert np.array_equal(np.isnan(want), np.isnan(exact)), (case, k)
            with np.errstate(invalid="ignore"):
                gap = np.abs(want - exact)
            info["D"][k] = float(np.nanmax(gap)) if np.isfinite(gap).any() else 0.0
        for tag, f in TO.coloured(S).items():
            idx = TO.colour_indices(ref[f], N)
            panel = shown[tag]
            assert panel.dtype == np.float64 and np.array_equal(TO.panel_from_indices(idx, lut).view(np.uint64), panel.view(np.uint64)), (case, tag)
            arrays[f"{case}_{tag}_idx"] = idx.astype(np.uint16)
            band = 2 * max(4 * info["D"][f], EPS32)
            near = TO.near_step(mine64[f], N, band)
            if case == "z":
                near &= ~TO.special_mask(f, ref[f].shape, T)
            info["share"][tag] = float(near.mean())
            assert info["share"][tag] <= MAX_SHARE, (case, tag, info["share"][tag])
        for m in TO.MUTANTS:
            mut = TO.evaluate(x["imgs"], x["rgb"], x["depth"], x["alphas"], x["invalid"], Z_NEAR, Z_FAR, mutant=m)
            for k in names:
                bar = max(4 * info["D"][k], EPS32)
                with np.errstate(invalid="ignore"):
                    diff = np.abs(mut[k].astype(np.float64) - mine64[k])
                both_nan = np.isnan(mut[k]) & np.isnan(mine64[k])
                diff = np.where(both_nan, 0.0, np.where(np.isnan(diff), np.inf, diff))
                over = float(diff.max() / bar)
                gaps[m] = max(gaps[m], min(over, 1e30))
        for k, a in stored.items():
            arrays[f"{case}_{k}"] = a
        for k in names:
            arrays[f"{case}_{k}"] = ref[k]
        arrays[f"{case}_recon_im"] = shown["recon_im"]
        meta["cases"][case] = info
    assert all(g > 1.0 for g in gaps.values()), gaps
    meta["mutants"] = {m: float(min(g, 1e30)) for m, g in gaps.items()}      # the largest distance in units of the bar
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return arrays


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    meta = json.loads(str(arrays["meta"]))
    print(json.dumps(meta, indent=1))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1 << 20
