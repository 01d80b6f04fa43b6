"""The evaluation frame's render launch with a claimed tail (bts_eval_frame_sched: the waves walk fixed ray lists over the first part of
the frame and claim the rest ray by ray from their XCD's counter) against the same launch on fixed lists alone: a ray is evaluated by exactly one
wave iteration whichever wave that is, so every output is the same bits.  The outputs are NaN before the call, so a ray rendered by no
wave shows; a ray rendered twice would show in the counter."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _frame(H, W, K, v):
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    dev = torch.device("cuda")
    scene = S.synthetic_scene(1, v, H, W, 64, seed=9, intrinsics=S.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W, learn_empty=True))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=1)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to(dev).eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().to(dev)
    frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(3.0, 80.0))
    return frame, [scene[k].to(dev) for k in ("images", "projs", "poses")]


def _split(groups):
    """(first claimed group, waves) of a one-ray launch over `groups` rays on this device, from the library's own host function"""
    from behindthescenes_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = (min((groups + 3) // 4, 2 * cus) + 7) // 8 * 8
    return _lib.load().bts_render_dyn_first(grid, groups, None), grid * 4


def _run(frame, inputs, jitter, tail, monkeypatch):
    """one frame with every freshly allocated float tensor NaN before the library writes it"""
    empty = torch.empty

    def nan_empty(*a, **kw):
        t = empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    frame.dynamic_tail = tail
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", nan_empty)
        out = frame(*inputs, ids_encoder=[0], ids_render=[0], jitter=jitter)
    assert frame.last_path == "fused"
    torch.cuda.synchronize()
    return out


def _assert_same(a, b, what):
    assert torch.equal(a["rays"], b["rays"]), (what, "rays")
    for k in ("rgb", "depth", "weights", "alphas", "invalid"):
        x, y = a["coarse"][0][k], b["coarse"][0][k]
        assert not torch.isnan(x).any() and not torch.isnan(y).any(), (what, k, "a ray no wave rendered")
        assert torch.equal(x, y), (what, k)


def _tickets(frame):
    (sc,) = frame._scratch.values()
    return int(sc["sched"].sum().item())          # (one counter per XCD)


# H, W, K, v, a tail is expected
CASES = [
    (24, 160, 64, 2, True),    # 7 680 rays on 2 048 waves, both views: the static part ends inside view 1, the tail is general-loop rays
    (24, 160, 64, 1, True),    # every ray in the shared-texel loop; the tail (768 rays) is smaller than the grid: most waves claim nothing
    (25, 160, 40, 2, False),   # 40 samples: four rays in three iterations (the 48-lane mode) -- not a one-ray launch, fixed lists
    (25, 160, 56, 2, True),    # 8 000 rays, no multiple of the chunk; lanes 56 - 63 idle
    (8, 32, 64, 2, False),     # 512 rays on 512 waves: too few rays per wave for a tail
]


@pytest.mark.parametrize("H,W,K,v,has_tail", CASES)
def test_claimed_tail_equals_fixed_lists(H, W, K, v, has_tail, monkeypatch):
    frame, inputs = _frame(H, W, K, v)
    groups = v * H * W
    first, waves = _split(groups)
    one_ray = K > 48 or (v * H * W) % 4 != 0
    assert (one_ray and first < groups) == has_tail, (first, groups)
    assert first <= groups and (first == groups or first >= waves)
    jitter = torch.rand((groups, K), generator=torch.Generator().manual_seed(3)).cuda()
    fixed = _run(frame, inputs, jitter, False, monkeypatch)
    assert _tickets(frame) == 0          # (the counter is not touched without the tail)
    tail = _run(frame, inputs, jitter, True, monkeypatch)
    _assert_same(fixed, tail, (H, W, K, v))
    t = _tickets(frame)
    if has_tail:
        # every group of the tail was handed out once; a wave draws at most two tickets past the end (its last prefetch and the claim
        # behind it) and waves that never reach the end of their list draw none
        assert groups - first <= t <= groups - first + 2 * waves, (t, groups - first)
    else:
        assert t == 0


def test_two_frames_in_a_row_through_one_arena(monkeypatch):
    """the hand-over launch zeroes the counters in front of every render: the second frame starts its tickets at 0 again"""
    H, W, K, v = 24, 160, 64, 2
    frame, inputs = _frame(H, W, K, v)
    groups = v * H * W
    first, waves = _split(groups)
    assert first < groups
    js = [torch.rand((groups, K), generator=torch.Generator().manual_seed(s)).cuda() for s in (5, 6)]
    fixed = [_run(frame, inputs, j, False, monkeypatch) for j in js]
    tail = []
    for j in js:
        tail.append(_run(frame, inputs, j, True, monkeypatch))
        assert groups - first <= _tickets(frame) <= groups - first + 2 * waves
    for i in range(2):
        _assert_same(fixed[i], tail[i], f"frame {i}")
    assert not torch.equal(tail[0]["coarse"][0]["depth"], tail[1]["coarse"][0]["depth"])    # (two different frames)
