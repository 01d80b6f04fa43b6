"""GPU: the list-driven form of the fused training step's two sparse projection passes (csrc/bts_prep.hip: compact_tiles_kernel ->
project_kernel with `list` / project_bwd_tiles_kernel<.., LIST = true>), which only maps of >= 4096 tiles reached through
bts_train_step_fwd / bts_train_step_bwd take -- every training line of bench.py and every real training run, and no other test.

* the fused step against the entry-by-entry step (whose public entry points pass no list workspace: always the flag form) at shapes
  above the threshold, at the bars of tests/test_gpu_train_fused.py: forward outputs bit-identical, loss within 1e-6 relative, gradients
  within 2e-5 of the largest entry (the order of the float atomics);
* a white-box observer (tests/_tile_list.py) reads the lists back from the arena's workspace, so that every case KNOWS which form ran: a
  silent fall-back to the flag form would otherwise turn these tests into repeats of tests/test_gpu_train_fused.py.  The workspace is
  filled with NaN words before each call, so a list that is found was written by that call;
* stale-buffer poisoning: the sparse forward leaves unsampled tiles of the arena's projected map as they are, so re-running the same
  inputs on the same arena hides a wrongly skipped tile behind the previous run's values -- every observed step here starts from
  NaN-filled maps, and one test changes patches, jitter and weights from step to step on one arena;
* the "listall" build (BTS_LIST_MIN_TILES = 1, behindthescenes_amd/build.py) in a process of its own: the list form on the small odd
  geometries of the other files' fused cases (one-tile maps, HW % 64 != 0, W' % 16 != 0, the 48-lane pyramid) and on this file's own.

Mutation check (one-line edits of csrc/bts_prep.hip on a scratch copy, each built as the product and as listall, run on an MI355X; every
edit keeps all accesses in bounds).  Red in the product build / red under listall:
  1. compact_tiles_kernel drops the last flagged tile of each work-group (count and entry): every test of this file above the threshold
     (the forward list's count != the flagged tiles) and both kitti_raw_list anchor cases / test_odd_pyramid_*, test_which_form_runs_*, 9 of
     tests/test_gpu_train_fused.py + channels_last's fused cases;
  2. the LIST kernel skips do_clean for tile 0: the kitti_raw, pyramid, coarser-scale, stale-buffer, learn_empty and frozen_mlp cases (NaN
     rows in d_feat: the NaN blocks freed before backward()) / test_which_form_runs_*, test_concurrent_scales_*, channels_last's fused cases;
  3. do_dirty leaves dG as it is in the LIST form: every test above the threshold ((d_proj, d_tiles) left dirty) and both anchor cases /
     test_odd_pyramid_*, test_which_form_runs_*, test_fused_step_state_is_clean_*;
  4. project_kernel reads its list one entry off (list[3 + ..]: the last tile dropped): every test above the threshold (NaN-filled maps ->
     non-finite outputs) and both anchor cases / test_odd_pyramid_*, test_fused_step_equals_the_entry_by_entry_step[*]."""
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import _tile_list as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_KITTI = dict(V=4, H=192, W=640, C=64, HD=64, NB=0, K=64, ids_loss=[0, 1], ids_render=[2, 3], z=(3.0, 80.0), hard_cap=True, code_mode="z",
              policy="weight_guided", patch=8)
SHAPES = {
    # exp_kitti_raw.yaml's per-sample shape at n = 3: 5760 tiles
    "kitti_raw_n3": dict(_KITTI, n=3, rays=2048, scales=1),
    # n = 9, the smallest batch with TWO pyramid scales on the list form: 17 280 / 4320 tiles, and 1080 / 270 below the threshold
    "pyramid_n9": dict(_KITTI, n=9, rays=512, scales=4),
    # The list lives in the backward workspace, whose size follows the RAYS: ~20 bytes per field sample (+ 512 per ray) and the 80 KB of pass
    # C's slot copies.  exp_kitti_raw.yaml's maps never lack room (n = 9 with as few as 64 rays per sample: 737 KB against a list of 86 KB);
    # two 384 x 1280 maps (15 360 tiles: 76 832 bytes) under one 4 x 4 patch per sample do: 40 960 bytes in front of the slot copies -- the
    # BACKWARD falls back to the flag form, while the forward's slice (which includes the slot copies: 122 880 bytes) still holds the list
    "small_workspace": dict(_KITTI, n=2, H=384, W=1280, rays=16, patch=4, scales=1),
    # both passes fall back: four such maps (30 720 tiles: 153 632 bytes) and K = 16 (a workspace of 126 976 bytes in all)
    "tiny_workspace": dict(_KITTI, n=4, H=384, W=1280, rays=16, patch=4, K=16, scales=1),
    # HW & 3 != 0 at the coarsest scale (5 x 9 texels: the scalar paths of the clean pass and of the weight gradient); W' % 16 != 0 everywhere, so
    # a channels-last map's tiles are runs of 64 texels, not blocks.  Far below 4096 tiles: list form in the listall build only
    "odd_40x72": dict(_KITTI, n=2, H=40, W=72, rays=256, scales=4),
}


def _setup(cfg, channels_last=False, learn_empty=False, seed=5, baseline=0.4):
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    from behindthescenes_amd.train_step import FusedTrainStep
    dev = torch.device("cuda")
    scene = S.synthetic_scene(cfg["n"], cfg["V"], cfg["H"], cfg["W"], 1, seed=seed, baseline=baseline, smooth=True)   # (its one-channel map is not used)
    conf = S.field_conf(cfg["C"], cfg["HD"], cfg["NB"], cfg["H"], cfg["W"], z_near=cfg["z"][0], z_far=cfg["z"][1], code_mode=cfg["code_mode"],
                        learn_empty=learn_empty)
    torch.manual_seed(11)
    net = bts.BTSNet(conf)
    net.encoder = bts.FeatureMapEncoder((cfg["H"], cfg["W"]), cfg["C"], num_views=cfg["n"], n_scales=cfg["scales"], pyramid=cfg["scales"] > 1,
                                        channels_last=channels_last)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to(dev).train()
    assert all(bts.native.is_channels_last(p) == channels_last for p in net.encoder.feats)
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=cfg["K"], lindisp=True, hard_alpha_cap=cfg["hard_cap"], lean_training_outputs=True)).to(dev).train()
    sampler = bts.PatchRaySampler(ray_batch_size=cfg["rays"], z_near=cfg["z"][0], z_far=cfg["z"][1], patch_size=cfg["patch"])
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": cfg["policy"], "lambda_edge_aware_smoothness": 0.001})
    step = FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit, multiscale=cfg["scales"] > 1)
    return step, net, [scene[k].to(dev) for k in ("images", "projs", "poses")]


def _call(step, inputs, cfg, seed):
    torch.manual_seed(seed)          # the CPU generator (patches) and the device generator (jitter) both start over
    return step(*inputs, ids_encoder=[0], ids_render=cfg["ids_render"], ids_loss=cfg["ids_loss"])


def _run(step, net, inputs, cfg, fused, seed=3, between=None):
    step.fused = fused
    net.zero_grad(set_to_none=True)
    loss, loss_dict, data = _call(step, inputs, cfg, seed)
    assert step.last_path == ("fused" if fused else "entries: switched off (fused=False)"), step.last_path
    if between is not None:
        between()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return loss.detach().clone(), dict(loss_dict), data, grads


def _assert_same_step(tag, entries, fused, n_scales):
    """The bars of tests/test_gpu_train_fused.py::test_fused_step_equals_the_entry_by_entry_step."""
    (l_e, d_e, data_e, g_e), (l_f, d_f, data_f, g_f) = entries, fused
    assert torch.equal(data_e["rays"], data_f["rays"]) and torch.equal(data_e["rgb_gt"], data_f["rgb_gt"])
    assert len(data_e["coarse"]) == len(data_f["coarse"]) == n_scales
    for s, (ce, cf) in enumerate(zip(data_e["coarse"], data_f["coarse"])):
        for k in ("rgb", "depth", "invalid_wsum", "invalid_any"):
            assert ce[k].shape == cf[k].shape, (k, ce[k].shape, cf[k].shape)
            assert torch.isfinite(cf[k]).all(), (tag, s, k)
            assert torch.equal(ce[k].detach(), cf[k]), (tag, s, k, (ce[k].detach() - cf[k]).abs().max().item())
    assert abs(l_e.item() - l_f.item()) <= 1e-6 * max(1.0, abs(l_e.item())), (l_e.item(), l_f.item())
    assert set(d_e) == set(d_f)
    for k in d_e:
        assert abs(d_e[k] - d_f[k]) <= 1e-6 * max(1.0, abs(d_e[k])), (k, d_e[k], d_f[k])
    assert set(g_e) == set(g_f) and len(g_e) >= 1
    for k in g_e:
        assert torch.isfinite(g_f[k]).all(), (tag, k)
        top = g_e[k].abs().max().item()
        assert top > 0, k
        err = (g_e[k] - g_f[k]).abs().max().item() / top
        assert err <= 2e-5, (tag, k, err)


class _Observer:
    """Runs around one fused step on a primed arena (TL.the_arena()): `between()` after the forward, `after()` after the backward.
    Asserts for every scale which form each pass took -- computed here from the sizes alone -- and, where a list was written, that it is
    right.  `forms` ends up as [(forward took the list form, backward did | None where it cannot be told)] per scale."""

    def __init__(self, step, net, cfg, channels_last):
        self.step, self.net, self.cl = step, net, channels_last
        n, nv = cfg["n"], len(cfg["ids_render"])
        self.need = TL.render_bwd_need(net, n, cfg["H"], cfg["W"], nv, cfg["rays"], cfg["K"])
        self.arena = TL.the_arena()
        assert TL.ws_bytes(self.arena) == ((self.need + 255) // 256 * 256) * len(self.arena.scales) + 16
        self.concurrent = bool(step.concurrent_scales) and len(self.arena.scales) > 1
        self.sampled, self.forms, self.copies = [], [], []
        TL.poison(self.arena)

    def scale_of(self, s):
        return self.net.encoder.scales[s] if self.step.multiscale else self.net.get_scale()

    def between(self):
        for s, sc in enumerate(self.arena.scales):
            want = TL.expect_list(sc["tiles"].numel(), TL.fwd_slice(self.arena))
            self.sampled.append(TL.check_forward_list(self.arena, s, want))
            self.forms.append([want, None])
        TL.poison(self.arena)           # (idle between the two calls; the backward zeroes what it needs zero)

    def after(self):
        S = len(self.arena.scales)
        for s, sc in enumerate(self.arena.scales):
            p = self.net.encoder.feats[self.scale_of(s)]
            d_feat = p.grad if p.requires_grad else None
            mlp_grad = any(q.requires_grad for q in self.net.mlp_coarse.parameters())
            want = TL.expect_list(sc["tiles"].numel(), TL.bwd_capacity(self.need, self.net.spec.d_hidden)) and (d_feat is not None or mlp_grad)
            # one after the other, a later scale's render passes park their state over an earlier scale's list: only the last one survives
            if self.concurrent or s == S - 1:
                self.copies.append(TL.check_backward_list(self.arena, s, TL.bwd_offset(self.need, s, self.concurrent), want, self.sampled[s], d_feat, self.cl))
                self.forms[s][1] = want
            else:
                self.copies.append(None)
            if d_feat is not None:      # whichever form ran: finite, and nothing outside the tiles the forward sampled
                assert torch.isfinite(d_feat).all(), f"scale {s}: non-finite feature gradient"
                n, h, w, _ = sc["proj"].shape
                outside = ~TL.dirty_texels(self.sampled[s], n, h, w, self.cl).to(d_feat.device)
                assert not (d_feat.detach() != 0).any(dim=1)[outside].any(), f"scale {s}: feature gradient on a texel of an unsampled tile"
                if self.copies[-1] is not None:     # exactly zero outside the DIRTY tiles (the list form's clean pass)
                    clean = ~TL.dirty_texels(self.copies[-1], n, h, w, self.cl).to(d_feat.device)
                    assert (d_feat.detach().permute(0, 2, 3, 1)[clean] == 0).all(), f"scale {s}: a clean tile's gradient rows are not zero"
        TL.check_kept_pairs_are_clean(self.arena)


def _observed_fused_run(step, net, inputs, cfg, channels_last, seed=3, prime=True, poison_maps=True):
    """One fused step under the observer, on buffers that hold nothing a wrong step could live on.  prime: a forward without grad first
    (other patches), so that the arena exists.  poison_maps: every scale's projected map is NaN-filled -- the sparse forward leaves
    unsampled tiles as they are, and a tile of an earlier forward holds CORRECT values (G depends on the map and the weights, not on the
    rays).  The workspace is NaN-filled before either call (_Observer).  d_feat is allocated inside backward() (empty_like): NaN-filled
    blocks of the maps' sizes are allocated and freed right before it, best effort, so that rows nobody writes show."""
    from behindthescenes_amd import train_step as TS
    step.fused = True
    if prime:
        TS.release_arenas()
        with torch.no_grad():
            _call(step, inputs, cfg, seed + 100)
    ob = _Observer(step, net, cfg, channels_last)
    if poison_maps:
        for sc in ob.arena.scales:
            sc["proj"].fill_(float("nan"))

    def between():
        ob.between()
        blocks = [torch.full_like(p, float("nan")) for p in net.encoder.feats if p.requires_grad for _ in range(2)]
        torch.cuda.synchronize()
        del blocks
    res = _run(step, net, inputs, cfg, fused=True, seed=seed, between=between)
    ob.after()
    return res, ob


def _compare(shape, channels_last=False, concurrent=False, learn_empty=False, freeze=None, scale=None):
    from behindthescenes_amd import train_step as TS
    cfg = SHAPES[shape]
    # learn_empty: a stereo baseline of 2 m -- at z_near = 3 m the partner frame's rays start half a frustum width (0.52 of the
    # normalised image) outside the encoder view, so that samples which read the empty feature are certain
    step, net, inputs = _setup(cfg, channels_last, learn_empty, baseline=2.0 if learn_empty else 0.4)
    step.concurrent_scales = concurrent
    if scale is not None:           # one render of that scale alone
        step.multiscale = False
        net.set_scale(scale)
    if freeze == "maps":
        net.encoder.requires_grad_(False)
    elif freeze == "mlp":
        net.mlp_coarse.requires_grad_(False)
    entries = _run(step, net, inputs, cfg, fused=False)
    fused, ob = _observed_fused_run(step, net, inputs, cfg, channels_last)
    n_scales = cfg["scales"] if step.multiscale else 1
    _assert_same_step(shape, entries, fused, n_scales)
    if freeze == "maps":
        assert not any(k.startswith("encoder") for k in fused[3])
    if freeze == "mlp":
        assert not any(k.startswith("mlp_coarse") for k in fused[3]) and any(k.startswith("encoder") for k in fused[3])
    if learn_empty:
        assert "empty_feature" in fused[3]
    TS.release_arenas()
    return ob


# ---- (b) the product build at the real threshold: the fused step (list form) against the entry-by-entry step (flag form) ---------------

@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_list_form_at_the_kitti_raw_shape_equals_the_entry_by_entry_step(channels_last):
    """exp_kitti_raw.yaml's per-sample shape at n = 3 (5760 tiles): both passes on the list form (asserted), NCHW maps (runs of 64 texels)
    and channels-last maps (16 x 4 block tiles)."""
    ob = _compare("kitti_raw_n3", channels_last)
    assert ob.forms == [[True, True]]


@pytest.mark.parametrize("concurrent", [False, True], ids=["serial", "concurrent"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_list_form_on_a_pyramid_with_scales_on_either_side_of_the_threshold(channels_last, concurrent):
    """n = 9 at 192 x 640 with four pyramid scales: 17 280 and 4320 tiles on the list form, 1080 and 270 on the flag form IN THE SAME
    step, the scales' chains one after the other and side by side (each scale's list in its own slice: all four backward forms seen)."""
    ob = _compare("pyramid_n9", channels_last, concurrent)
    assert [f[0] for f in ob.forms] == [True, True, False, False]
    assert [f[1] for f in ob.forms] == ([True, True, False, False] if concurrent else [None, None, None, False])


def test_list_form_at_a_single_coarser_scale():
    """The serial pyramid step above cannot show scale 1's backward list (scale 2's passes overwrite it): one render of scale 1 alone
    (n = 9: 4320 tiles of a 96 x 320 map read through feat_shift = 1)."""
    ob = _compare("pyramid_n9", scale=1)
    assert ob.forms == [[True, True]] and ob.arena.scales[0]["tiles"].numel() == 4320


def test_workspace_too_small_for_the_list_falls_back_to_the_flag_form():
    """The list lives in the backward workspace, which is sized by the rays (bts_render_bwd_workspace), not by the maps: large maps and
    few rays leave no room for it, and the passes must quietly take the flag form -- same results.  Two shapes (see SHAPES): the
    backward alone falls back (its share excludes pass C's slot copies, the forward's slice does not), and both passes fall back.  The
    sizes are computed here from the layout, the observer shows what ran."""
    for shape, fwd in (("small_workspace", True), ("tiny_workspace", False)):
        cfg = SHAPES[shape]
        n_tiles = cfg["n"] * (cfg["H"] * cfg["W"] // 64)
        assert n_tiles >= 4096
        ob = _compare(shape)
        assert ob.arena.scales[0]["tiles"].numel() == n_tiles
        assert TL.bwd_capacity(ob.need, 64) < TL.list_bytes(n_tiles)
        assert (TL.fwd_slice(ob.arena) >= TL.list_bytes(n_tiles)) == fwd
        assert ob.forms == [[fwd, False]]


@pytest.mark.parametrize("what", ["learn_empty", "frozen_maps", "frozen_mlp"])
def test_list_form_with_the_optional_gradients(what):
    """n = 3: the learned empty feature (its gradient and its share of lin_in's come out of the second call); frozen feature maps (no d_feat:
    the list kernel's clean pass is skipped, the (d_proj, tiles) pair must still come back clean); a frozen MLP (no d_mlp: the weight
    gradient's role is idle)."""
    ob = _compare("kitti_raw_n3", learn_empty=what == "learn_empty", freeze={"frozen_maps": "maps", "frozen_mlp": "mlp"}.get(what))
    assert ob.forms == [[True, True]]


# ---- (c) stale buffers ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_list_form_does_not_live_on_the_previous_steps_buffers(channels_last):
    """Step 1 builds the arena; its projected maps are then NaN-filled; step 2 runs on OTHER patches, jitter and MLP weights: a flagged tile
    the forward skipped would now read NaN (before, the previous run's identical values).  Step 3 follows with its maps left as step 2
    wrote them: it starts from the (d_proj, tiles) pair step 2 left behind.  Both must equal the entry-by-entry step on their inputs."""
    from behindthescenes_amd import train_step as TS
    cfg = SHAPES["kitti_raw_n3"]
    step, net, inputs = _setup(cfg, channels_last)
    TS.release_arenas()
    _run(step, net, inputs, cfg, fused=True, seed=3)
    g = torch.Generator().manual_seed(19)
    with torch.no_grad():
        for p in net.mlp_coarse.parameters():
            p.add_(0.02 * p.abs().mean() * torch.randn(p.shape, generator=g).to(p.device))
    second, ob2 = _observed_fused_run(step, net, inputs, cfg, channels_last, seed=4, prime=False)
    third, ob3 = _observed_fused_run(step, net, inputs, cfg, channels_last, seed=5, prime=False, poison_maps=False)
    assert ob2.forms == [[True, True]] and ob3.forms == [[True, True]]
    assert not torch.equal(ob2.sampled[0], ob3.sampled[0])          # (other patches: other tiles)
    _assert_same_step("second", _run(step, net, inputs, cfg, fused=False, seed=4), second, 1)
    _assert_same_step("third", _run(step, net, inputs, cfg, fused=False, seed=5), third, 1)
    TS.release_arenas()


# ---- (d) the listall build: the list form at every size ----------------------------------------------------------------------------------

@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_odd_pyramid_equals_the_entry_by_entry_step(channels_last):
    """40 x 72 with four scales (20 x 36, 10 x 18, 5 x 9: HW & 3 != 0 at the coarsest, tiles cut by the end of the map at every scale, W' % 16
    != 0 so that a channels-last map's tiles are runs).  60 / 16 / 4 / 2 tiles: the flag form in the product build, the list form in the
    listall build (test_listall_variant runs this test there) -- the observer asserts which."""
    ob = _compare("odd_40x72", channels_last)
    small = TL.list_min_tiles() <= 2
    assert [f[0] for f in ob.forms] == [small] * 4 and ob.forms[3][1] == small


def test_which_form_runs_below_the_threshold():
    """A 48 x 160 map, n = 2 (tests/test_gpu_train_fused.py's "kitti"): 240 tiles.  The product build must NOT write a list (the workspace
    stays NaN where it would be); a build with BTS_LIST_MIN_TILES = 1 must -- test_listall_variant selects this test to prove that the
    variant it loads is that build."""
    from behindthescenes_amd import train_step as TS
    from tests.test_gpu_train_fused import SHAPES as TOY
    cfg = dict(TOY["kitti"], patch=8)
    step, net, inputs = _setup(cfg)
    (_, _, _, grads), ob = _observed_fused_run(step, net, inputs, cfg, False)
    TS.release_arenas()
    assert ob.arena.scales[0]["tiles"].numel() == 240 and "encoder.feats.0" in grads
    want = TL.list_min_tiles() <= 240
    assert ob.forms == [[want, want]]


_LISTALL = {
    # the fused step / eval frame against the entry-by-entry sequence at the toy shapes: one- and two-tile maps, HW % 64 != 0, the 48-lane pyramid
    "train_fused": (["tests/test_gpu_train_fused.py"], None, 10),
    # channels-last maps: 64 x 96 (blocks) and its pyramid down to 16 x 24 (W' % 16 != 0: runs)
    "channels_last": (["tests/test_gpu_channels_last.py"], "fused_train_step", 2),
    # the reference's golden step and the two yaml shapes against the oracle
    "anchor": (["tests/test_gpu_fused_anchor.py::test_fused_train_step_vs_reference_golden",
                "tests/test_gpu_fused_anchor.py::test_fused_train_step_vs_oracle_at_the_yaml_shapes[kitti_raw]",
                "tests/test_gpu_fused_anchor.py::test_fused_train_step_vs_oracle_at_the_yaml_shapes[re10k]"], None, 3),
    # this file's odd pyramid, and the observer's proof that the variant IS the variant
    "own": (["tests/test_gpu_tile_list.py"], "odd_pyramid or which_form_runs", 3),
}


@pytest.mark.parametrize("group", list(_LISTALL))
def test_listall_variant(group):
    """The same sources built with -DBTS_LIST_MIN_TILES=1 (behindthescenes_amd/build.py: "listall"), in a process of its own: the library
    is chosen at load time through BTS_RENDER_LIB.  Every fused training step of the selected tests then takes the list form wherever the
    workspace holds the list -- test_which_form_runs_below_the_threshold asserts through the observer that it does."""
    lib = os.path.join(ROOT, "behindthescenes_amd", "variants", "libbts_listall.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() builds the variants"
    files, sel, n_min = _LISTALL[group]
    env = dict(os.environ, BTS_RENDER_LIB=lib, BTS_ALLOW_LIB_OVERRIDE="1", BTS_TEST_LIST_MIN_TILES="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + (["-k", sel] if sel else []) + files
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"\b(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= n_min and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-500:]
