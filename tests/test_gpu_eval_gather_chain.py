"""GPU: the gather chain of the evaluation frame's pinned kernel (render_kernel_p's PINNED form), whose general loop forms its LDS-DMA
offsets from tap table rows held in registers (one read per point tile, ``GTapRegs``), against the general kernel, which reads the
table for every block.  The offsets are the same integers and every accumulator sees the same FMAs in the same order in both loops,
so every output is the same bits (``torch.equal``, the outputs NaN before the call as in tests/test_gpu_eval_pinned.py, whose helpers
run the frames here).

What the cases are about
  * clamped and out-of-frame taps: a stereo baseline at which a good part of view 1's samples leave the encoder frame -- their taps are
    clamped to the border, and o11 = o10 + o01 - o00 of a clamped tap is where a wrong register-held row shows;
  * loop switches: v = 2, n = 2 is shared -> general -> shared per wave; v = 1 is every ray in the shared-texel loop.  A frame whose
    every ray takes the GENERAL loop cannot be had on the pinned kernel: the pinned set wants the render view to be the encoder view,
    ``ImageRaySampler`` casts the rays of every pixel of every view, and the encoder view's own rays start at the encoder camera's
    centre -- they are the rays whose samples share their texels.  v = 3 (two thirds of the rays general, the general loop entered once
    and kept across a view boundary) stands in for it;
  * rerun identity: the DMA-against-ds_read ordering fault of an early round showed as differences from run to run; the frame of the
    first case three times through one arena, once."""
import pytest
import torch

from tests._pinned_helpers import pinned
from tests.test_gpu_eval_pinned import H, W, _assert_same, _has_tail, _run

pytestmark = pytest.mark.gpu

K = 64
BAND = (0.05, 0.95)     # the share of view 1's samples outside the encoder frame that makes the first case what it is (a condition)


def _scene(n, v, baseline):
    from behindthescenes_amd import synthetic as S
    return S.synthetic_scene(n, v, H, W, 64, seed=9, intrinsics=S.K_KITTIRAW, smooth=True, baseline=baseline)


def _frame(scene, n):
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    dev = torch.device("cuda")
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W, learn_empty=True))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=n)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to(dev).eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().to(dev)
    return bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(3.0, 80.0)), [scene[k].to(dev) for k in ("images", "projs", "poses")]


def _invalid_share_view1(scene, jitter, n, v):
    """share of view 1's samples whose projection into view 0 (the encoder view) is invalid, by the oracle on the CPU"""
    from oracle import bts_oracle as O
    rays = O.image_rays(scene["poses"], scene["projs"], H, W, 3.0, 80.0).view(n, v, H * W, 8)
    u = jitter.view(n, v, H * W, K)
    bad = 0.0
    for i in range(n):
        r = rays[i, 1]
        z = O.sample_coarse(r, K, True, u[i, 1])
        xyz = r[:, None, :3] + z[..., None] * r[:, None, 3:6]
        inv = O.project(xyz.reshape(1, -1, 3), torch.linalg.inv(scene["poses"][i, 0]).view(1, 1, 4, 4), scene["projs"][i, 0].view(1, 1, 3, 3))[3]
        bad += inv.float().mean().item() / n
    return bad


@pytest.fixture(scope="module")
def wide_stereo():
    """v = 2, n = 2 at the first baseline of 0.54 m x 2^i whose share of out-of-frame samples of view 1 lies well inside BAND (chosen on the
    CPU); the frame, its inputs, its jitter, and the general kernel's outputs (computed once, compared against and never written)"""
    n, v = 2, 2
    jitter = torch.rand((n * v * H * W, K), generator=torch.Generator().manual_seed(3))
    for i in range(10):
        scene = _scene(n, v, 0.54 * 2 ** i)
        share = _invalid_share_view1(scene, jitter, n, v)
        print(f"baseline {0.54 * 2 ** i:.2f} m: {share:.3f} of view 1's samples leave the encoder frame (CPU oracle)")
        if 0.25 <= share <= 0.75:
            break
    else:
        pytest.fail("no baseline puts the out-of-frame share inside the band")
    frame, inputs = _frame(scene, n)
    jitter = jitter.cuda()
    off = _run(frame, inputs, jitter, False, pytest.MonkeyPatch)
    return dict(n=n, v=v, frame=frame, inputs=inputs, jitter=jitter, off=off, share=share)


def test_clamped_and_out_of_frame_taps(wide_stereo):
    c = wide_stereo
    assert _has_tail(c["n"] * c["v"] * H * W) and pinned(K=K, n=c["n"], v=c["v"], H=H, W=W) == 1
    got = c["off"]["coarse"][0]["invalid"][:, 1].mean().item()       # the general kernel's own word on view 1
    print(f"general kernel: {got:.3f} of view 1's samples invalid (CPU oracle {c['share']:.3f})")
    assert BAND[0] <= got <= BAND[1], got
    on = _run(c["frame"], c["inputs"], c["jitter"], True, pytest.MonkeyPatch)
    _assert_same(c["off"], on, "wide stereo")


# v = 1: every ray shared; v = 3: shared, then general across a view boundary (see the module docstring for "every ray general")
@pytest.mark.parametrize("v,n", [(1, 1), (3, 1)])
def test_loop_switches(v, n):
    assert _has_tail(n * v * H * W) and pinned(K=K, n=n, v=v, H=H, W=W) == 1
    frame, inputs = _frame(_scene(n, v, 0.54), n)
    jitter = torch.rand((n * v * H * W, K), generator=torch.Generator().manual_seed(3)).cuda()
    off = _run(frame, inputs, jitter, False, pytest.MonkeyPatch)
    on = _run(frame, inputs, jitter, True, pytest.MonkeyPatch)
    _assert_same(off, on, (v, n))


def test_rerun_identity(wide_stereo):
    c = wide_stereo
    runs = [_run(c["frame"], c["inputs"], c["jitter"], True, pytest.MonkeyPatch) for _ in range(3)]
    _assert_same(runs[0], runs[1], "run 2 against run 1")
    _assert_same(runs[0], runs[2], "run 3 against run 1")
    _assert_same(c["off"], runs[2], "run 3 against the general kernel")
