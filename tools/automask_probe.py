"""ms per call of auto-masking (use_automasking) on the GPU, in ONE process:

  map_kitti_360 / map_kitti_raw   the error map of trainer.py:203-206 at exp_kitti_360.yaml's shape (16 x 8 frames, 4 loss frames,
                    192 x 640) and exp_kitti_raw.yaml's (8 x 4 frames, 2 loss frames): automask.automask_images (bts_automask_errors,
                    csrc/bts_automask.hip, one launch) against the eager torch restatement of those four lines; both maps are compared,
                    and the kernel's achieved GB/s against its compulsory traffic (every input plane read once, four planes per frame
                    written once) is reported
  loss_*            the three loss entry points WITH the per-ray bound against the same entry point WITHOUT it (whose device code is the
                    previous revision's, instruction for instruction) on the same inputs: 16 x 4096 rays, nv = 4, forward + gradients --
                    wave (8 x 8 patches, bts_photometric_loss), tiled (16 x 16 patches, bts_photometric_loss_tiled), pixel l2 and
                    pixel l1 + median (bts_pixel_loss); `added` is the number to read

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  The two sides of every comparison are
alternated in four blocks, so that a drifting clock meets both.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/automask_probe.py [--out profiles/r17a/automask.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import native  # noqa: E402

K = 64
_WINDOW = [[0.0947, 0.1183, 0.0947], [0.1183, 0.1478, 0.1183], [0.0947, 0.1183, 0.0947]]


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


def blocks(fn_a, fn_b, iters, warmup, names):
    t_a, t_b = [], []
    for _ in range(4):
        t_a.append(mean_ms(fn_a, max(iters // 4, 1), warmup // 4 + 1))
        t_b.append(mean_ms(fn_b, max(iters // 4, 1), warmup // 4 + 1))
    a, b = sum(t_a) / 4, sum(t_b) / 4
    return {names[0]: round(a, 4), names[1]: round(b, 4), f"{names[0]}_blocks": [round(t, 4) for t in t_a], f"{names[1]}_blocks": [round(t, 4) for t in t_b]}


# ---- the reference's op sequence, restated in eager torch (trainer.py:203-206, loss.py:10-18, layers.py:79-150)
def _gauss(x, window):
    return F.conv2d(x, window.repeat(x.shape[1], 1, 1, 1), padding=0, groups=x.shape[1])


def _errors_l1ssim(img0, img1, window):
    n, pc, h, w, nv, c = img0.shape
    img1 = img1.expand(img0.shape)
    x = img0.permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    y = img1.permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    xp, yp = F.pad(x, (1, 1, 1, 1)), F.pad(y, (1, 1, 1, 1))
    mu_x, mu_y = _gauss(xp, window), _gauss(yp, window)
    mu_x_sq, mu_y_sq, mu_x_y = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    sigma_x, sigma_y, sigma_xy = _gauss(xp ** 2, window) - mu_x_sq, _gauss(yp ** 2, window) - mu_y_sq, _gauss(xp * yp, window) - mu_x_y
    ssim_n = (2 * mu_x_y + 0.01 ** 2) * (2 * sigma_xy + 0.03 ** 2)
    ssim_d = (mu_x_sq + mu_y_sq + 0.01 ** 2) * (sigma_x + sigma_y + 0.03 ** 2)
    e = .85 * torch.mean(torch.clamp(1 - ssim_n / ssim_d, 0, 1) / 2, dim=1) + .15 * torch.mean(torch.abs(x - y), dim=1)
    return e.view(n, pc, nv, h, w).permute(0, 1, 3, 4, 2).unsqueeze(-1)


def eager_images4(images_ip, ids_loss, window):
    n, v, c, h, w = images_ip.shape
    L = len(ids_loss)
    frames = images_ip.permute(0, 1, 3, 4, 2).reshape(n, v, h, w, 1, c).expand(-1, -1, -1, -1, L, -1) * .5
    partners = images_ip[:, ids_loss].permute(0, 3, 4, 1, 2).reshape(n, 1, h, w, L, c).expand(-1, v, -1, -1, -1, -1) * .5
    errors = _errors_l1ssim(frames, partners, window).mean(-2).squeeze(-1).unsqueeze(2)
    return torch.cat((images_ip, errors), dim=2)


def probe_map(n, v, L, H, W, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(17)
    base = F.avg_pool2d(torch.rand(n, 3, H + 2 * v + 4, W + 2 * v + 4, device="cuda", generator=g), 5, 1, 2)
    images_ip = torch.stack([base[:, :, k:k + H, 2 * k:2 * k + W] for k in range(v)], dim=1).contiguous()
    ids_loss = list(range(0, 2 * L, 2))[:L] if 2 * L <= v else list(range(L))
    window = torch.tensor(_WINDOW, device="cuda")
    with torch.no_grad():
        lib, eag = bts.automask_images(images_ip, ids_loss), eager_images4(images_ip, ids_loss, window)
        diff = (lib[:, :, 3] - eag[:, :, 3]).abs().max().item()
        same_planes = torch.equal(lib[:, :, :3], images_ip)
        del lib, eag

        def f_lib():
            bts.automask_images(images_ip, ids_loss)

        def f_eager():
            eager_images4(images_ip, ids_loss, window)

        res = blocks(f_lib, f_eager, iters, warmup, ("library", "eager"))
    gb = (n * v * 3 * H * W + n * v * 4 * H * W) * 4 / 1e9
    res.update(shape=[n, v, L, H, W], ratio=round(res["eager"] / res["library"], 2), separated=max(res["library_blocks"]) < min(res["eager_blocks"]),
               map_max_abs_diff_library_vs_eager=diff, colour_planes_copied_exactly=same_planes, compulsory_gb=round(gb, 4),
               achieved_gb_per_s=round(gb / (res["library"] * 1e-3), 1))
    return res


def loss_inputs(n, pc, h, w, nv, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = dict(device="cuda", generator=g)
    gt = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, **r), 3, 1, 1)[:, :, 2:-2, 2:-2]
    gt = gt.reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous()
    rgb = (gt.unsqueeze(-2) + 0.15 * torch.randn(n, pc, h, w, nv, 3, **r)).clamp(0, 1)
    depth = torch.rand(n, pc, h, w, **r) * 100 + 0.5
    wts = torch.rand(n, pc, h, w, K, **r)
    wts = wts / wts.sum(-1, keepdim=True)
    inv = ((torch.rand(n, pc, h, w, K, nv, **r) < 0.3) & (torch.rand(n, pc, h, w, 1, nv, **r) < 0.2)).float()
    B = n * pc * h * w
    return dict(rgb=rgb.reshape(B, nv * 3), depth=depth.reshape(B), weights=wts.reshape(B, K), invalid=inv.reshape(B, K, nv), rgb_gt=gt.reshape(B, 3),
                thresh=(0.02 + 0.2 * torch.rand(B, **r)))


def probe_loss(iters, warmup):
    out = {}
    for tag, (n, pc, h, w), kind in (("loss_wave_p8", (16, 64, 8, 8), "ssim"), ("loss_tiled_p16", (16, 16, 16, 16), "ssim"),
                                     ("loss_pixel_l2", (16, 64, 8, 8), "l2"), ("loss_pixel_l1_median", (16, 64, 8, 8), "l1_median")):
        t = loss_inputs(n, pc, h, w, 4, seed=13)

        def call(thresh):
            if kind == "ssim":
                return native.photometric_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], h, w, "weight_guided", True, 1.0, 1.0,
                                               thresh=thresh)
            return native.pixel_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], n, h, w, kind[:2], "strict", kind.endswith("median"),
                                     True, thresh=thresh)

        res = blocks(lambda: call(None), lambda: call(t["thresh"]), iters, warmup, ("without_bound", "with_bound"))
        res["added"] = round(res["with_bound"] - res["without_bound"], 4)
        a, b = call(None), call(t["thresh"])
        res["rgb_term_without_vs_with"] = [(a[0][:, 0].sum() if kind == "ssim" else a[0][0]).item(), (b[0][:, 0].sum() if kind == "ssim" else b[0][0]).item()]
        out[tag] = res
        del t
        torch.cuda.empty_cache()
    return out


def run(iters, warmup):
    out = dict(metric="ms_per_call", iters=iters, warmup=warmup)
    out["map_kitti_360"] = probe_map(16, 8, 4, 192, 640, iters, warmup)
    torch.cuda.empty_cache()
    out["map_kitti_raw"] = probe_map(8, 4, 2, 192, 640, iters, warmup)
    torch.cuda.empty_cache()
    out.update(probe_loss(iters, warmup))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("automask_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Auto-masking (use_automasking): the error map and the per-ray bound in the loss kernels, ms per call (tools/automask_probe.py; "
                    f"HIP events, mean over {res['iters']} iterations after {res['warmup']} warm-ups, alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:24s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
