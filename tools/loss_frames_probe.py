"""ms per call of the photometric loss on patches of more than 64 pixels (bts_photometric_loss_tiled through ReconstructionLoss) against
an eager torch restatement of the reference's loss sequence (models/bts/model/loss.py:83-293 for l1+ssim, weight_guided,
lambda_edge_aware_smoothness = 0.01; without its nine .item() synchronisations, which only favours it) on the same GPU, in ONE process:

  val_v2 / val_v8   the validation loss (base_trainer.py:70-84, loss_during_validation): n = 1, 192 x 640 frames, v = 2 and v = 8 frames
                    as ImageRaySampler.reconstruct lays them out, nv = 1, K = 64, forward only (under no_grad)
  train_p16         the trainer's default patch: 16 x 16 patches at exp_kitti_360.yaml's ray count (16 x 4096 rays), nv = 4, K = 64,
                    forward + gradients with respect to rgb and depth
  frame_v2          FusedEvalFrame alone (v = 2, nv = 1, K = 64) and followed by the criterion on its output: the number to report is
                    added_by_loss = frame_loss - frame

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  The two sides of every comparison are
alternated in four blocks, so that a drifting clock meets both; `separated` says whether the slowest library block is faster than the
fastest eager block.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/loss_frames_probe.py [--out profiles/r13a/loss_frames.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import synthetic  # noqa: E402

CONFIG = {"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_edge_aware_smoothness": 0.01}
K = 64
_WINDOW = torch.tensor([[0.0947, 0.1183, 0.0947], [0.1183, 0.1478, 0.1183], [0.0947, 0.1183, 0.0947]])


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


# ---- the reference's op sequence, restated in eager torch (layers.py:79-150, loss.py:10-40, 83-293)
def _gauss(x):
    return F.conv2d(x, _WINDOW.to(x.device, x.dtype).repeat(x.shape[1], 1, 1, 1), padding=0, groups=x.shape[1])


def _ssim(x, y):
    x, y = F.pad(x, (1, 1, 1, 1)), F.pad(y, (1, 1, 1, 1))
    mu_x, mu_y = _gauss(x), _gauss(y)
    sigma_x, sigma_y, sigma_xy = _gauss(x ** 2) - mu_x ** 2, _gauss(y ** 2) - mu_y ** 2, _gauss(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sigma_xy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sigma_x + sigma_y + 0.03 ** 2)
    return torch.clamp(1 - n / d, 0, 1) / 2


def _errors(img0, img1):
    n, pc, h, w, nv, c = img0.shape
    img1 = img1.expand(img0.shape)
    a = img0.permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    b = img1.permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    e = .85 * torch.mean(_ssim(a, b), dim=1) + .15 * torch.mean(torch.abs(a - b), dim=1)
    return e.view(n, pc, nv, h, w).permute(0, 1, 3, 4, 2).unsqueeze(-1)


def _eas(gt_img, depth):
    n, pc, h, w = depth.shape
    gt = gt_img.permute(0, 1, 4, 5, 2, 3).reshape(-1, 3, h, w)
    d = 1 / depth.reshape(-1, 1, h, w).clamp(1e-3, 80)
    d = d / torch.mean(d, dim=[2, 3], keepdim=True)
    d_dx, d_dy = torch.abs(d[:, :, :, :-1] - d[:, :, :, 1:]), torch.abs(d[:, :, :-1, :] - d[:, :, 1:, :])
    i_dx = torch.mean(torch.abs(gt[:, :, :, :-1] - gt[:, :, :, 1:]), 1, keepdim=True)
    i_dy = torch.mean(torch.abs(gt[:, :, :-1, :] - gt[:, :, 1:, :]), 1, keepdim=True)
    return (F.pad(d_dx * torch.exp(-i_dx), (0, 1)) + F.pad(d_dy * torch.exp(-i_dy), (0, 0, 0, 1))).view(n, pc, h, w)


def eager_loss(level, rgb_gt):
    inv, wts = level["invalid"], level["weights"]
    invalid = torch.all((inv.to(torch.float32) * wts.unsqueeze(-1)).sum(-2) > .9, dim=-1, keepdim=True)
    keep = 1 - invalid.to(torch.float32)
    gt = rgb_gt.unsqueeze(-2)
    rgb_loss = (_errors(level["rgb"], gt).amin(-2) * keep).mean()
    fine_loss = (_errors(level["rgb"], gt).amin(-2) * keep).mean()        # the reference evaluates the aliased fine dict again (:171-184)
    loss = rgb_loss * 1 + fine_loss * 1
    eas = _eas(gt, level["depth"])
    eas = (eas * (1 - torch.ceil(F.interpolate(invalid.squeeze(-1).to(torch.float32), size=level["depth"].shape[-2:])))).mean()
    return loss + eas * CONFIG["lambda_edge_aware_smoothness"]


def inputs(n, pc, h, w, nv, seed, grad):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = dict(device="cuda", generator=g)
    gt = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, **r), 3, 1, 1)[:, :, 2:-2, 2:-2]
    gt = gt.reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous()
    rgb = (gt.unsqueeze(-2) + 0.15 * torch.randn(n, pc, h, w, nv, 3, **r)).clamp(0, 1)
    depth = torch.rand(n, pc, h, w, **r) * 100 + 0.5
    wts = torch.rand(n, pc, h, w, K, **r)
    wts = wts / wts.sum(-1, keepdim=True)
    inv = (torch.rand(n, pc, h, w, K, nv, **r) < 0.3).float()
    inv[:, :, 0] = 1.0
    level = dict(rgb=rgb.requires_grad_(grad), depth=depth.requires_grad_(grad), weights=wts, invalid=inv)
    return level, gt


def blocks(fn_lib, fn_eager, iters, warmup):
    t_lib, t_eager = [], []
    for _ in range(4):
        t_lib.append(mean_ms(fn_lib, max(iters // 4, 1), warmup // 4 + 1))
        t_eager.append(mean_ms(fn_eager, max(iters // 4, 1), warmup // 4 + 1))
    lib, eager = sum(t_lib) / 4, sum(t_eager) / 4
    return dict(library=round(lib, 4), eager=round(eager, 4), ratio=round(eager / lib, 2), separated=max(t_lib) < min(t_eager),
                library_blocks=[round(t, 4) for t in t_lib], eager_blocks=[round(t, 4) for t in t_eager])


def run(iters, warmup):
    out = dict(metric="ms_per_call", K=K, iters=iters, warmup=warmup)
    crit = bts.ReconstructionLoss(dict(CONFIG))
    for tag, shape, grad in (("val_v2", (1, 2, 192, 640, 1), False), ("val_v8", (1, 8, 192, 640, 1), False), ("train_p16", (16, 16, 16, 16, 4), True)):
        level, gt = inputs(*shape, seed=13, grad=grad)
        data = dict(coarse=[level], fine=[dict(level)], rgb_gt=gt)

        def lib():
            if grad:
                torch.autograd.grad(crit(data)[0], [level["rgb"], level["depth"]])
            else:
                with torch.no_grad():
                    crit(data)

        def eager():
            if grad:
                torch.autograd.grad(eager_loss(level, gt), [level["rgb"], level["depth"]])
            else:
                with torch.no_grad():
                    eager_loss(level, gt)

        with torch.no_grad():
            out[f"{tag}_loss_library_vs_eager"] = [crit(data)[0].item(), eager_loss(level, gt).item()]
        out[tag] = blocks(lib, eager, iters, warmup)
        del level, gt, data
        torch.cuda.empty_cache()

    # the validation frame with and without its loss
    H, W, V = 192, 640, 2
    scene = synthetic.synthetic_scene(1, V, H, W, 64, seed=9, intrinsics=synthetic.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(synthetic.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=1)
    synthetic.init_mlp_(net.mlp_coarse, seed=7)
    net = net.cuda().eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().cuda()
    frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(3.0, 80.0))
    frame_inputs = [scene[k].cuda() for k in ("images", "projs", "poses")]
    kw = dict(ids_encoder=[0], ids_render=[0], jitter=torch.rand(V * H * W, K, device="cuda"))

    def with_loss():
        with torch.no_grad():
            crit(frame(*frame_inputs, **kw))

    t_alone, t_with = [], []
    for _ in range(4):
        t_alone.append(mean_ms(lambda: frame(*frame_inputs, **kw), max(iters // 4, 1), warmup // 4 + 1))
        t_with.append(mean_ms(with_loss, max(iters // 4, 1), warmup // 4 + 1))
    out["frame_v2"] = dict(frame=round(sum(t_alone) / 4, 4), frame_loss=round(sum(t_with) / 4, 4),
                           added_by_loss=round((sum(t_with) - sum(t_alone)) / 4, 4), path=frame.last_path,
                           frame_blocks=[round(t, 4) for t in t_alone], frame_loss_blocks=[round(t, 4) for t in t_with])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_frames_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Photometric loss on patches of more than 64 pixels and on whole frames, ms per call (tools/loss_frames_probe.py; HIP events, "
                    f"mean over {res['iters']} iterations after {res['warmup']} warm-ups, alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:32s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
