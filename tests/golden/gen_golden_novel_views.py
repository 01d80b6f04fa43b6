"""Writes tests/golden/novel_views.npz FROM THE REAL REFERENCE, on CPU tensors:

  * the colour cases through the reference's own ``color_tensor`` (utils/plotting.py:41-46) with the installed matplotlib -- the
    fixture below was written with matplotlib 3.10.8 (the version is also stored in its ``meta``) -- and matplotlib's ``bytes=True``
    path for the uint8 form;
  * the finish cases through the reference's own ``render_poses`` (scripts/inference_setup.py:182-198; the module itself cannot be
    imported -- hydra, the datasets, an os.system call at module scope -- so the function's source is compiled from the file) with a
    stand-in renderer and ray sampler that hand it the stored ``rgb`` / ``depth`` / ``weights`` / ``invalid``, followed by the per-frame
    statements of scripts/videos/gen_vid_nvs.py:105-120, compiled from that file in the same way (image over depth).

    python tests/golden/gen_golden_novel_views.py

Tables: magma, plasma and "extremes" (magma with under / over / bad colours of its own, cases a and b).
Colour cases (each with every table, ``norm`` off and on): s 1 x 1; a 7 x 9 with a NaN; b 16 x 64; c 33 x 70 (b, c: the special values
without the NaN, so that ``norm`` has finite extrema); k 7 x 9 constant (0 / 0 under ``norm``); m three 7 x 9 images of different
ranges (the reference is called once per image: its ``norm`` is per call).  Special values: negatives, 0, 1, nextafter(1, 2),
255.5 / 256, a value above 1.
Finish cases: p 5 x 7 (its maximum depth sits on an invalid pixel) and q 24 x 40, ``black_invalid`` off and on; K = 8 samples per
pixel; some pixels carry their whole weight on one invalid sample so that the fp32 sum IS float32(0.8) or one of its two neighbours;
case q's colours hold, for every byte value k, the two float32 neighbours of k / 255.

tests/_novel_views_oracle.py must reproduce every stored output exactly, and each of its mutants (t == N not folded, NaN not bad,
the 0.8 threshold as double, the maximum taken after masking) must change at least one stored output byte: asserted here, the
numbers of changed bytes go to ``meta``.  The fifth candidate, x 255 in fp32 instead of double, cannot change a byte for any float32
colour in [0, 1] (see generate()); that equivalence is asserted instead."""
import ast
import json
import os
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import _novel_views_oracle as NO
from oracle.ref_shim import REFERENCE_ROOT, reference_available

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "novel_views.npz")
TABLES = ("magma", "plasma", "extremes")     # extremes: magma with under / over / bad colours of its own (cases a, b only)
K = 8
RANGES = dict(p=(3.0, 80.0), q=(2.5, 51.3))


def reference_functions():
    """color_tensor (imported), render_poses and the frame statements of gen_vid_nvs.py (compiled from the reference's files)"""
    assert reference_available(), f"reference tree not found at {REFERENCE_ROOT}"
    sys.dont_write_bytecode = True
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    from utils.plotting import color_tensor
    src = open(os.path.join(REFERENCE_ROOT, "scripts", "inference_setup.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "render_poses")
    ns = {}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "inference_setup.py", "exec"), ns)
    lines = open(os.path.join(REFERENCE_ROOT, "scripts", "videos", "gen_vid_nvs.py")).read().split("\n")
    # :105-107 the numpy image, the normalised depth and its colours; :110 the concatenation; :120 the bytes of every frame
    text = textwrap.dedent("\n".join(lines[104:107])) + "\n" + lines[109].strip() + "\nframes = [frame]\n" + lines[119].strip() + "\n"
    assert "color_tensor" in text and "concatenate" in text and "astype" in text, text
    return color_tensor, ns["render_poses"], compile(text, "gen_vid_nvs.py", "exec")


def specials(with_nan):
    v = [-0.25, -1e-8, 0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 255.5 / 256, 1.25, 0.5, 1.0 / 256, 255.0 / 256]
    return np.array(v + ([float("nan")] if with_nan else []), dtype=np.float32)


def colour_inputs():
    rng = np.random.default_rng(14)

    def image(h, w, with_nan, lo=-0.1, hi=1.1):
        x = (lo + (hi - lo) * rng.random((h, w))).astype(np.float32)
        s = specials(with_nan)
        if x.size > s.size:
            x.reshape(-1)[rng.choice(x.size, s.size, replace=False)] = s
        return x
    m = np.stack([rng.random((7, 9)), 3 + 77 * rng.random((7, 9)), -5 + 4 * rng.random((7, 9))]).astype(np.float32)
    return dict(s=np.array([[0.37]], dtype=np.float32), a=image(7, 9, True), b=image(16, 64, False), c=image(33, 70, False),
                k=np.full((7, 9), 0.5, dtype=np.float32), m=m)


def byte_edges():
    """per byte value k the largest float32 below k / 255 and the smallest at or above it: where trunc(c * 255) steps"""
    out = []
    for k in range(1, 256):
        c = np.float32(k / 255)
        while float(c) * 255.0 >= k:
            c = np.nextafter(c, np.float32(0))
        out += [c, np.nextafter(c, np.float32(1))]
    return np.array(out, dtype=np.float32)


def finish_inputs(name):
    h, w = dict(p=(5, 7), q=(24, 40))[name]
    rng = np.random.default_rng(dict(p=5, q=6)[name])
    rgb = rng.random((h, w, 3)).astype(np.float32)
    depth = (3 + 60 * rng.random((h, w))).astype(np.float32)
    alphas = rng.random((h, w, K)).astype(np.float32)
    weights = rng.random((h, w, K)).astype(np.float32)
    weights = (weights / weights.sum(-1, keepdims=True) * rng.random((h, w, 1))).astype(np.float32)
    invalid = (rng.random((h, w, K)) < np.linspace(0.0, 1.0, w)[None, :, None]).astype(np.float32)     # more invalid to the right
    # the threshold and its two fp32 neighbours, exactly: the whole weight on one invalid sample
    t = np.float32(0.8)
    edge = [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))]
    for i, v in enumerate(edge * 2):
        y, x = (i * 2 + 1) % h, (i * 3 + 1) % w
        weights[y, x], invalid[y, x] = 0, 0
        weights[y, x, i % K], invalid[y, x, i % K] = v, 1
    if name == "q":
        edges = byte_edges()
        rgb.reshape(-1)[rng.choice(rgb.size, edges.size, replace=False)] = edges
    rgb[0, 0], rgb[h - 1, w - 1, 0] = (0.0, 1.0, 0.5), 1.0
    if name == "p":     # the maximum depth on a pixel that is invalid for certain
        weights[2, w - 1], invalid[2, w - 1] = 0, 1
        weights[2, w - 1, 0] = 0.95
        depth[2, w - 1] = 79.5
    return dict(rgb=rgb, depth=depth, weights=weights, alphas=alphas, invalid=invalid)


class _Sampler:
    def sample(self, images, poses, projs):
        return None, None

    def reconstruct(self, render_dict):
        return render_dict


def run_render_poses(render_poses, x, black_invalid):
    h, w = x["depth"].shape
    coarse = dict(rgb=torch.from_numpy(x["rgb"].copy()).view(1, 1, h, w, 1, 3), depth=torch.from_numpy(x["depth"].copy()).view(1, 1, h, w),
                  weights=torch.from_numpy(x["weights"]).view(1, 1, h, w, K), alphas=torch.from_numpy(x["alphas"]).view(1, 1, h, w, K),
                  invalid=torch.from_numpy(x["invalid"]).view(1, 1, h, w, K, 1))

    def renderer(rays, want_weights, want_alphas):
        assert want_weights and want_alphas
        return dict(coarse=coarse)
    return render_poses(renderer, _Sampler(), torch.eye(4).view(1, 1, 4, 4), torch.eye(3).view(1, 1, 3, 3), black_invalid=black_invalid)


def changed(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return int((a.view(np.uint8) != b.view(np.uint8)).sum())


def generate():
    import matplotlib
    color_tensor, render_poses, frame_code = reference_functions()
    arrays, meta = {}, dict(matplotlib=matplotlib.__version__, mutants={})
    luts = {}
    cmaps = {n: matplotlib.colormaps[n] for n in TABLES[:2]}
    # magma's and plasma's over colour IS their last colour: only a table whose extremes differ shows whether t == N was folded
    cmaps["extremes"] = matplotlib.colormaps["magma"].with_extremes(under="cyan", over="lime", bad="red")
    for name in TABLES:
        cm = cmaps[name]
        cm._init()
        luts[name] = arrays[f"lut_{name}"] = np.array(cm._lut, dtype=np.float64)
        assert luts[name].shape == (259, 4)
    hits = dict(fold=0, nan_bad=0, threshold64=0, max_after=0, u8_fp32=0)
    for case, x in colour_inputs().items():
        arrays[f"col_{case}_x"] = x
        for name in TABLES:
            if name == "extremes" and case not in ("a", "b"):
                continue
            cm = cmaps[name]
            for norm in (0, 1):
                imgs = x if x.ndim == 3 else x[None]
                with np.errstate(invalid="ignore"):
                    f64 = np.stack([color_tensor(torch.from_numpy(i), cm, norm=bool(norm)).numpy() for i in imgs])
                    u8 = np.stack([cm(NO.normalise(i) if norm else i, bytes=True)[..., :3] for i in imgs])
                assert f64.dtype == np.float64 and u8.dtype == np.uint8
                mine = np.stack([NO.colorize(i, luts[name], norm=bool(norm)) for i in imgs])
                mine_u8 = np.stack([NO.colorize_u8(i, luts[name], norm=bool(norm)) for i in imgs])
                assert changed(mine, f64) == 0 and np.array_equal(mine_u8, u8), (case, name, norm)
                assert np.array_equal(u8, (f64 * 255).astype(np.uint8))
                for k in ("fold", "nan_bad"):
                    hits[k] += changed(np.stack([NO.colorize_u8(i, luts[name], norm=bool(norm), **{k: False}) for i in imgs]), u8)
                arrays[f"col_{case}_{name}_{norm}_f64"] = f64 if x.ndim == 3 else f64[0]
                arrays[f"col_{case}_{name}_{norm}_u8"] = u8 if x.ndim == 3 else u8[0]
    for case in ("p", "q"):
        x = finish_inputs(case)
        d_min, d_max = RANGES[case]
        t = {k: torch.from_numpy(v) for k, v in x.items()}
        wsum32 = (t["invalid"] * t["weights"]).sum(-1).numpy()
        wsum64 = (x["invalid"].astype(np.float64) * x["weights"].astype(np.float64)).sum(-1)
        for k, v in x.items():
            arrays[f"fin_{case}_{k}"] = v
        arrays[f"fin_{case}_wsum"], arrays[f"fin_{case}_wsum64"] = wsum32, wsum64
        arrays[f"fin_{case}_range"] = np.array([d_min, d_max], dtype=np.float64)
        assert sum(int((wsum32 == v).sum()) for v in (np.float32(0.8), np.nextafter(np.float32(0.8), np.float32(0)),
                                                     np.nextafter(np.float32(0.8), np.float32(1)))) >= 3
        for bi in (0, 1):
            frame, depth = run_render_poses(render_poses, x, bool(bi))
            assert tuple(frame.shape) == (1, *x["depth"].shape, 1, 3) and tuple(depth.shape) == x["depth"].shape
            ns = dict(novel_view=frame, depth=depth, d_min=d_min, d_max=d_max, color_tensor=color_tensor, np=np, torch=torch)
            exec(frame_code, ns)
            canvas = ns["frames"][0]
            h = depth.shape[0]
            assert canvas.dtype == np.uint8 and canvas.shape == (2 * h, depth.shape[1], 3)
            arrays[f"fin_{case}_{bi}_rgb"], arrays[f"fin_{case}_{bi}_depth"] = frame[0, :, :, 0].numpy(), depth.numpy()
            arrays[f"fin_{case}_{bi}_canvas"] = canvas
            inv = wsum32 > np.float32(0.8)
            assert inv.any() and (~inv).any()
            if case == "p" and bi:
                assert inv.reshape(-1)[x["depth"].argmax()] and depth.max() == x["depth"].max()
            mine = NO.finish(x["rgb"], x["depth"], wsum32, d_min, d_max, luts["magma"], bool(bi))
            got = np.concatenate((mine["img_u8"], mine["depth_u8"]), axis=0)
            assert np.array_equal(got, canvas) and changed(mine["rgb"], arrays[f"fin_{case}_{bi}_rgb"]) == 0 and \
                changed(mine["depth"], arrays[f"fin_{case}_{bi}_depth"]) == 0, (case, bi)
            for k in ("threshold64", "max_after", "u8_fp32"):
                if k == "u8_fp32" or bi:
                    m = NO.finish(x["rgb"], x["depth"], wsum32, d_min, d_max, luts["magma"], bool(bi), **{k: True})
                    hits[k] += changed(np.concatenate((m["img_u8"], m["depth_u8"]), axis=0), canvas)
    # x 255 in fp32 is NOT a mutant: for a float32 c in [0, 1] and an integer k, c * 255 < k implies fl32(c * 255) < k (the gap
    # k - c * 255 is at least 128 / 255 of the spacing of fp32 below k, never under half of it, because 255 = 2^8 - 1), and rounding is
    # monotone above k.  Case q carries both neighbours of every k / 255; the two evaluations agree on all of them, and on every byte.
    assert hits.pop("u8_fp32") == 0
    e = byte_edges()
    assert np.array_equal(NO.to_u8(e), NO.to_u8(e, u8_fp32=True)) and np.array_equal(NO.to_u8(e)[1::2], np.arange(1, 256).astype(np.uint8))
    assert all(v > 0 for v in hits.values()), hits
    meta["mutants"] = hits
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return arrays


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(json.dumps(json.loads(str(arrays["meta"])), indent=1))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
