"""GPU: the evaluation frame's render launch on the kernel with the frame's switches compiled in (render_kernel_p's PINNED form,
``FusedEvalFrame.pinned_kernel``) against the same launch on the general kernel: the same arithmetic in the same order, so every output
is the same bits.  The outputs are NaN before the call, so a sample no lane wrote shows.  Frames that miss the pinned set by one switch
take the general kernel and still equal the entry-by-entry sequence."""
import pytest
import torch

from tests._pinned_helpers import pinned

pytestmark = pytest.mark.gpu

H, W = 24, 160      # the smallest frame at which the render launch gets a claimed tail (tests/test_gpu_eval_dynamic_tail.py)


def _frame(K, v, n=1, learn_empty=True, hard_alpha_cap=True):
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    dev = torch.device("cuda")
    scene = S.synthetic_scene(n, v, H, W, 64, seed=9, intrinsics=S.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W, learn_empty=learn_empty))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=n)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to(dev).eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=hard_alpha_cap)).bind_parallel(net).eval().to(dev)
    frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(3.0, 80.0))
    return frame, [scene[k].to(dev) for k in ("images", "projs", "poses")]


def _has_tail(groups):
    from behindthescenes_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = (min((groups + 3) // 4, 2 * cus) + 7) // 8 * 8
    return _lib.load().bts_render_dyn_first(grid, groups, None) < groups


def _run(frame, inputs, jitter, on, monkeypatch):
    """one frame with every freshly allocated float tensor NaN before the library writes it"""
    empty = torch.empty

    def nan_empty(*a, **kw):
        t = empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    frame.pinned_kernel = on
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", nan_empty)
        out = frame(*inputs, ids_encoder=[0], ids_render=[0], jitter=jitter)
    assert frame.last_path == "fused"
    torch.cuda.synchronize()
    return out


def _assert_same(a, b, what, keys=("rgb", "depth", "weights", "alphas", "invalid")):
    assert torch.equal(a["rays"], b["rays"]), (what, "rays")
    assert torch.equal(a["rgb_gt"].contiguous(), b["rgb_gt"].contiguous()), (what, "rgb_gt")
    for k in keys:
        x, y = a["coarse"][0][k], b["coarse"][0][k]
        assert x.shape == y.shape, (what, k)
        assert not torch.isnan(x).any() and not torch.isnan(y).any(), (what, k, "a value nothing wrote")
        assert torch.equal(x, y), (what, k)


# v, n: two views = both loops and one loop switch per wave; one view = every ray in the shared-texel loop; n = 2 = the batch-element boundary
@pytest.mark.parametrize("v,n", [(2, 1), (1, 1), (2, 2)])
def test_pinned_kernel_equals_the_general_kernel(v, n, monkeypatch):
    K = 64
    frame, inputs = _frame(K, v, n)
    groups = n * v * H * W
    assert _has_tail(groups) and pinned(K=K, n=n, v=v, H=H, W=W) == 1      # the launch this test is about takes the pinned kernel
    jitter = torch.rand((groups, K), generator=torch.Generator().manual_seed(3)).cuda()
    off = _run(frame, inputs, jitter, False, monkeypatch)
    on = _run(frame, inputs, jitter, True, monkeypatch)
    _assert_same(off, on, (v, n))


def test_two_frames_in_a_row_through_one_arena(monkeypatch):
    K, v = 64, 2
    frame, inputs = _frame(K, v)
    groups = v * H * W
    js = [torch.rand((groups, K), generator=torch.Generator().manual_seed(s)).cuda() for s in (5, 6)]
    off = [_run(frame, inputs, j, False, monkeypatch) for j in js]
    on = [_run(frame, inputs, j, True, monkeypatch) for j in js]
    for i in range(2):
        _assert_same(off[i], on[i], f"frame {i}")
    assert not torch.equal(on[0]["coarse"][0]["depth"], on[1]["coarse"][0]["depth"])    # (two different frames)


# what misses the pinned set: the frame, the call, and the same miss for the host's test
NEAR_MISSES = [
    ("K = 48", dict(K=48), dict(), dict(K=48)),
    ("hard_alpha_cap off", dict(hard_alpha_cap=False), dict(), dict(hard_alpha_cap=0)),
    ("learn_empty off", dict(learn_empty=False), dict(), dict(learn_empty=0)),
    ("want_weights = False", dict(), dict(want_weights=False), dict(weights=False)),
    ("a render view that is not the encoder view", dict(), dict(ids_render=[1]), dict(enc_view=-1)),
    ("two render views", dict(), dict(ids_render=[0, 1]), dict(nv=2)),
]


@pytest.mark.parametrize("what,frame_kw,call_kw,miss", NEAR_MISSES, ids=[m[0] for m in NEAR_MISSES])
def test_a_near_miss_takes_the_general_kernel_and_equals_the_entry_by_entry_frame(what, frame_kw, call_kw, miss):
    assert pinned(**miss) == 0
    frame, inputs = _frame(frame_kw.pop("K", 64), 2, **frame_kw)
    call = dict(dict(ids_encoder=[0], ids_render=[0]), **call_kw)
    outs = []
    for fused in (False, True):
        frame.fused = fused
        torch.manual_seed(21)          # the same jitter stream on both routes
        # (ImageRaySampler.reconstruct, which the entry-by-entry route ends in, needs the weights: that route always asks for them, and the
        # frame without them is held against its other outputs)
        outs.append(frame(*inputs, **(call if fused else dict(call, want_weights=True))))
        assert frame.last_path == ("fused" if fused else "entries: switched off (fused=False)")
    torch.cuda.synchronize()
    keys = [k for k in ("rgb", "depth", "weights", "alphas", "invalid") if k != "weights" or call.get("want_weights", True)]
    assert ("weights" in outs[1]["coarse"][0]) == call.get("want_weights", True)
    _assert_same(outs[0], outs[1], what, keys)
