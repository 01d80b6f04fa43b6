"""ms per frame of the image half of the NVS evaluation (evaluator_nvs.py:141-170: PSNR and SSIM over the 5 % crop) at 192 x 640 and
256 x 384, eval_resolution = the frame size.  Times, in ONE process,

  library        bts_nvs_metrics on the frame's real views (a [:, 1] slice of the render's (1, 3, H, W, 1, 3) output, the channel-planar
                 ground truth): the tile pass and finish
  host           the reference's route, restated: two F.interpolate calls and the crop on the device, two permuted device-to-host
                 copies, then tests/_nvs_metrics_oracle.py on the CPU (scipy.ndimage.uniform_filter under skimage's formulas -- skimage
                 itself is no dependency) and the PSNR
  eval_frame     FusedEvalFrame alone (bts_eval_frame, v = 3, K = 64, to_z = False)
  nvs_eval       FusedNVSEval.frame: the same frame + bts_nvs_metrics on the same stream -- the number to report is
                 added_by_metrics = nvs_eval - eval_frame

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window; the host route ends in its own copies, so the
closing event covers it).  The frame with and without the metrics is alternated in blocks.  Prints ONE JSON line and, with --out,
writes the same numbers as text.

    python tools/nvs_metrics_probe.py [--out profiles/<dir>/nvs_metrics.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import native, synthetic  # noqa: E402
from tests import _nvs_metrics_oracle as NO  # noqa: E402

SIZES = ((192, 640), (256, 384))
V, C, HD, K = 3, 64, 64, 64


def mean_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def frame_setup(H, W):
    scene = synthetic.synthetic_scene(1, V, H, W, C, seed=9, intrinsics=synthetic.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(synthetic.field_conf(C, HD, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), C, num_views=1)
    synthetic.init_mlp_(net.mlp_coarse, seed=7)
    net = net.cuda().eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().cuda()
    return wrapped, bts.ImageRaySampler(3.0, 80.0), [scene[k].cuda() for k in ("images", "projs", "poses")]


def host_route(rgb_pred, rgb_gt, res):
    """evaluator_nvs.py:146-170 without LPIPS"""
    sf_id = rgb_gt.shape[1] // 2
    gt = rgb_gt[:, sf_id:sf_id + 1].squeeze(0).permute(0, 3, 1, 2)
    pred = rgb_pred[:, sf_id:sf_id + 1].squeeze(0).squeeze(-2).permute(0, 3, 1, 2)
    gt, pred = F.interpolate(gt, res), F.interpolate(pred, res)
    y0, y1, x0, x1 = NO.crop_box(*res)
    gt, pred = gt[:, :, y0:y1, x0:x1], pred[:, :, y0:y1, x0:x1]
    gt_np, pred_np = gt.detach().squeeze().permute(1, 2, 0).cpu().numpy(), pred.detach().squeeze().permute(1, 2, 0).cpu().numpy()
    return NO.evaluate_cropped(pred_np, gt_np)


def run(iters, warmup):
    out = dict(metric="ms_per_frame", views=V, iters=iters, warmup=warmup)
    for H, W in SIZES:
        tag = f"{H}x{W}"
        wrapped, sampler, frame_inputs = frame_setup(H, W)
        kw = dict(ids_encoder=[0], ids_render=[0], jitter=torch.rand(V * H * W, K, device="cuda"))
        alone = bts.FusedEvalFrame(wrapped, sampler)
        data = alone(*frame_inputs, to_z=False, **kw)
        rgb_pred, rgb_gt = data["fine"][0]["rgb"], data["rgb_gt"]
        pv, gv = rgb_pred[:, V // 2, :, :, 0], rgb_gt[:, V // 2]
        row = torch.empty((1, 8), device="cuda", dtype=torch.float64)
        out[f"{tag}_library"] = round(mean_ms(lambda: native.nvs_metrics(pv, gv, (H, W), out=row), iters, warmup), 4)
        out[f"{tag}_host"] = round(mean_ms(lambda: host_route(rgb_pred, rgb_gt, (H, W)), max(20, iters // 4), max(5, warmup // 5)), 4)
        a, b = row[0].cpu().tolist(), host_route(rgb_pred, rgb_gt, (H, W)).tolist()
        out[f"{tag}_ssim_psnr_library_vs_host"] = [a[:2], b[:2]]
        ev = bts.FusedNVSEval(wrapped, sampler, (H, W), capacity=iters + warmup)
        # the two are alternated in blocks, so that a drifting clock meets both
        t_alone, t_with = [], []
        for _ in range(4):
            ev.reset()
            t_alone.append(mean_ms(lambda: alone(*frame_inputs, to_z=False, **kw), iters // 4, warmup // 4 + 1))
            t_with.append(mean_ms(lambda: ev.frame(*frame_inputs, **kw), iters // 4, warmup // 4 + 1))
        out[f"{tag}_eval_frame"] = round(sum(t_alone) / 4, 4)
        out[f"{tag}_nvs_eval"] = round(sum(t_with) / 4, 4)
        out[f"{tag}_added_by_metrics"] = round(out[f"{tag}_nvs_eval"] - out[f"{tag}_eval_frame"], 4)
        out[f"{tag}_eval_frame_blocks"], out[f"{tag}_nvs_eval_blocks"] = [round(t, 4) for t in t_alone], [round(t, 4) for t in t_with]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nvs_metrics_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("NVS evaluation metrics (PSNR, SSIM over the 5 % crop), ms per frame (tools/nvs_metrics_probe.py; HIP events, mean over "
                    f"{res['iters']} iterations after {res['warmup']} warm-ups)\n")
            for k, v in res.items():
                f.write(f"{k:44s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
