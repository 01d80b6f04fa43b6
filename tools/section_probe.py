"""Per-section cycle counters of the pipelined render kernel (probe build): where does a wave's time go?
    python tools/section_probe.py
Sections (s_memtime deltas accumulated per wave, averaged over waves, per ray iteration):
 0 geometry (ray/camera loads, projection, taps, colour issue, tile broadcast)   1 gather + encoding + MFMA
 2 lin_out + softplus   3 colour blend + compositing scan   4 per-sample stores   5 per-ray sums + stores
Ablations (BTS_ABLATE bits, probe build only) the render loop reads: 8 no colour taps, 16 no per-sample stores, 32 lin_out as three adds, 64 every ray
takes the shared-texel loop (one fetch of G per ray; wrong rows for view 1 -- what a single fetch would buy there), 128 the counters above.
Bits 1 (no gather), 2 (no trigonometry) and 4 (no MFMAs) act in eval_point only -- the exact cold path and the raw-feature query --
since the register gather, the one loop that read them, left the render kernel.
    python tools/section_probe.py --lifetimes [--no-tail] [--out FILE]
the flagship evaluation frame instead: per-wave lifetimes of its render launch over the chip, per XCD and per CU (the probe build stores
XCC_ID and HW_ID next to the counters); --no-tail: fixed ray lists to the end; BTS_DYN_TAIL_DIV=d: a claimed tail of 1 / d of the rays.
With them the launch's preheader per work-group: ticks from kernel entry to the barrier behind the staged MLP (the slowest of its waves)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BTS_RENDER_LIB", os.path.join(ROOT, "behindthescenes_amd", "variants", "libbts_probe.so"))
os.environ.setdefault("BTS_ALLOW_LIB_OVERRIDE", "1")
import torch
import behindthescenes_amd as bts
from behindthescenes_amd import native
from behindthescenes_amd import synthetic as S



def lifetime_table(d, out=sys.stdout):
    """Per-wave lifetime (d[6]) over the chip, per XCD and per CU.  d[7] = XCC_ID << 32 | HW_ID as the wave read them at kernel start
    (HW_ID: SIMD 5:4, CU 11:8, SH 12, SE 15:13).  gap = (max - mean) / max: the share of the launch a persistent grid idles away."""
    life, hw = d[:, 6], d[:, 7].long()
    xcd, cu = (hw >> 32) & 15, (hw >> 8) & 255

    def row(name, x):
        return (f"{name:<14s} waves {x.numel():5d}  mean {x.mean():10.0f}  min {x.min():10.0f}  max {x.max():10.0f}  "
                f"max/mean {x.max() / x.mean():.4f}  gap {(x.max() - x.mean()) / x.max() * 100:5.2f} %")
    print(row("chip", life), file=out)
    q = torch.quantile(life, torch.tensor([0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99], dtype=life.dtype))
    print("   quantiles 1 10 25 50 75 90 99 %: " + " ".join(f"{v:.0f}" for v in q.tolist()), file=out)
    for x in sorted(set(xcd.tolist())):
        print(row(f"xcd {x}", life[xcd == x]), file=out)
    cu_mean, cu_max = [], []
    for x in sorted(set(xcd.tolist())):
        for c in sorted(set(cu[xcd == x].tolist())):
            sel = life[(xcd == x) & (cu == c)]
            cu_mean.append(sel.mean()), cu_max.append(sel.max())
            print(row(f"xcd {x} cu {c:3d}", sel), file=out)
    cu_mean, cu_max = torch.stack(cu_mean), torch.stack(cu_max)
    print(f"per-CU means: {cu_mean.numel()} CUs, min {cu_mean.min():.0f} mean {cu_mean.mean():.0f} max {cu_mean.max():.0f}; "
          f"slowest CU's mean over the chip mean {cu_mean.max() / life.mean():.4f}; mean over CUs of (CU max / CU mean) {(cu_max / cu_mean).mean():.4f}", file=out)
    return (life.max() - life.mean()) / life.max()


def preheader_row(raw, frame_ms, out=sys.stdout):
    """The preheader of every work-group that ran (the probe build keeps it, 16 bits saturated, above XCC_ID in d[7]): median and maximum
    over the work-groups, in cycles of the counter the lifetimes are in and in microseconds.  Two conversions are printed: the device's
    shader clock as the driver reports it, and the rate this very frame shows -- its longest wave's lifetime over the frame's event time,
    which holds the other dispatches too, so that rate is a lower bound and the microseconds from it an upper one."""
    ran = raw[:, :, 6].amax(dim=1) > 0
    pre = ((raw[:, :, 7] >> 36) & 0xFFFF).amax(dim=1)[ran].double()
    life = raw[:, :, 6].amax(dim=1)[ran].double()
    import ctypes
    khz = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(khz), 5, torch.cuda.current_device())   # hipDeviceAttributeClockRate
    mhz = khz.value / 1e3 if khz.value > 0 else float("nan")
    mhz_run = float(life.max()) / (frame_ms * 1e3)
    print(f"preheader per work-group ({pre.numel()} work-groups): median {pre.median():.0f} cycles, max {pre.max():.0f} cycles"
          f"{' (saturated)' if pre.max() >= 0xFFFF else ''}; at the reported {mhz:.0f} MHz: median {pre.median() / mhz:.2f} us, max {pre.max() / mhz:.2f} us; "
          f"at the >= {mhz_run:.0f} MHz of this frame (longest wave {life.max():.0f} cycles in {frame_ms:.3f} ms): median <= {pre.median() / mhz_run:.2f} us, "
          f"max <= {pre.max() / mhz_run:.2f} us", file=out)


def eval_frame_lifetimes(argv):
    """python tools/section_probe.py --lifetimes [--no-tail] [--out FILE]: the flagship frame (bench.py's KITTI eval_depth workload through
    FusedEvalFrame) on the probe build; per-wave lifetimes of its render launch."""
    H, W, K, V, C, HD = 192, 640, 64, 2, 64, 64
    dev = torch.device("cuda")
    scene = S.synthetic_scene(1, V, H, W, C, seed=1000, intrinsics=S.K_KITTIRAW)
    torch.manual_seed(4242)
    net = bts.BTSNet(S.field_conf(C, HD, 0, H, W, z_near=3.0, z_far=80.0, learn_empty=True))
    S.init_mlp_(net.mlp_coarse, seed=7)
    S.set_feature_map(net, scene["feat"])
    net = net.to(dev).eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().to(dev)
    frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(3.0, 80.0))
    if "--no-tail" in argv and hasattr(frame, "dynamic_tail"):
        frame.dynamic_tail = False
    images, projs, poses = scene["images"].to(dev), scene["projs"].to(dev), scene["poses"].to(dev)
    dbg = torch.zeros(512 * 4 * 8, dtype=torch.int64, device=dev)
    os.environ["BTS_DBG_PTR"] = str(dbg.data_ptr())
    os.environ["BTS_ABLATE"] = "128"
    torch.manual_seed(4242)
    for _ in range(30):   # the device's steady state (bench.py: SETTLE_FRAMES)
        frame(images, projs, poses, ids_encoder=[0], ids_render=[0])
    out = open(argv[argv.index("--out") + 1], "w") if "--out" in argv else sys.stdout
    gaps = []
    for rep in range(3):
        dbg.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame(images, projs, poses, ids_encoder=[0], ids_render=[0])
        e1.record()
        torch.cuda.synchronize()
        assert frame.last_path == "fused", frame.last_path
        raw = dbg.view(-1, 4, 8).cpu()
        d = raw.view(-1, 8).double()
        d = d[d[:, 6] > 0]
        print(f"--- frame {rep}: {e0.elapsed_time(e1):.3f} ms (probe build, counters on), {V * H * W / d.shape[0]:.1f} rays per wave, "
              f"one ray = {d[:, 6].mean() * d.shape[0] / (V * H * W):.0f} ticks of wave time", file=out)
        gaps.append(float(lifetime_table(d, out)))
        preheader_row(raw, e0.elapsed_time(e1), out)
    print("gap (max - mean) / max per frame: " + " ".join(f"{100 * g:.2f} %" for g in gaps), file=out)


if "--lifetimes" in sys.argv:
    eval_frame_lifetimes(sys.argv)
    sys.exit(0)

H, W, K, V = 192, 640, 64, 2
scene =S.synthetic_scene(1, V, H, W, 64, seed=1, intrinsics=S.K_KITTIRAW)
net = S.build_net(scene, 64, 0, [0])
ft = net.native_field()
params = net.mlp_coarse.packed().detach()
rays = bts.ImageRaySampler(3.0, 80.0, H, W).sample(None, scene["poses"].cuda(), scene["projs"].cuda())[0].reshape(-1, 8).contiguous()
z = native.sample_coarse(rays, torch.rand(rays.shape[0], K, device="cuda"), True)
dbg = torch.zeros(512 * 4 * 8, dtype=torch.int64, device="cuda")
os.environ["BTS_DBG_PTR"] = str(dbg.data_ptr())
half = rays.shape[0] // 2
sets = {"both": (rays, z), "view0": (rays[:half].contiguous(), z[:half].contiguous()), "view1": (rays[half:].contiguous(), z[half:].contiguous())}
for name, (r_, z_) in sets.items():
    for extra in ((0, 64) if name != "both" else (0,)):
        os.environ["BTS_ABLATE"] = str(128 | extra)
        for _ in range(2):
            dbg.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            native.render_fwd(ft, params, r_, z_, hard_alpha_cap=True, want_weights=True, want_alphas=True, want_invalid=True)
            e1.record()
            torch.cuda.synchronize()
        d = dbg.view(-1, 8).double().cpu()
        d = d[d[:, 6] > 0]
        iters = r_.shape[0] / d.shape[0]
        per = d[:, :6].mean(0) / iters
        print(f"{name} ablate={extra}: {e0.elapsed_time(e1):.3f} ms, waves {d.shape[0]}, iterations/wave {iters:.1f}, wave lifetime {d[:,6].mean():.0f} ticks (max {d[:,6].max():.0f})")
        print("   ticks per iteration by section:", " ".join(f"{x:8.1f}" for x in per.tolist()), " sum", f"{per.sum():.1f}")
