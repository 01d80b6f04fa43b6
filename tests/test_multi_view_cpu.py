"""Merged encoder views (``combine_ids`` / several ``ids_encoder``) on the HIP kernels, host side: the ABI additions (symbols, error codes
and messages, nothing launched), the group tables against ``torch_modes._merge_groups`` on exhaustive flag patterns, and the
``native_multi_view`` switch of BTSNet.  No GPU needed."""
import ctypes as C
import itertools
import warnings

import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native, torch_modes

NEW_SYMBOLS = ("bts_render_fwd_multi_view", "bts_render_bwd_multi_view_workspace", "bts_render_bwd_multi_view", "bts_field_query_multi_view")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_are_exported_and_the_abi_is_still_9(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert _lib.BTS_MV_MAX_VIEWS == 8
    # 4 ints, 8 cfgs, 8 tensor blocks, the five tables (9 + 8 + 8 + 9 + 8 ints)
    assert C.sizeof(_lib.BtsMultiViewField) == 16 + 8 * C.sizeof(_lib.BtsFieldCfg) + 8 * C.sizeof(_lib.BtsFieldTensors) + 4 * 42


def _field(V=3, nv=3, enc_groups=((0, 1), (2,)), ren_groups=((0, 1), (2,)), C_=64, hd=64, nb=0):
    """a field every check accepts (pointers are never dereferenced: each call below fails its host-side checks first)"""
    p = 16
    mv = _lib.BtsMultiViewField()
    mv.V = V
    for v in range(V):
        mv.cfg[v] = native._spec_cfg(native.FieldSpec(C=C_, d_hidden=hd, n_blocks=nb, learn_empty=True), n=1, H=8, W=16, nv=nv)
        mv.view[v] = _lib.BtsFieldTensors(feat_nhwc=None, proj_nhwc=p, K_enc=p, w2c_enc=p, imgs_nhwc4=p, K_r=p, w2c_r=p, empty_feature=p,
                                          mlp_params=p)
    es, em, ek = native.group_tables(enc_groups, V, True)
    rs, rm, _ = native.group_tables(ren_groups, nv, False)
    mv.n_enc_groups, mv.n_ren_groups = len(ek), len(rs) - 1
    for name, vals in (("enc_group_start", es), ("enc_member", em), ("enc_mult", ek), ("ren_group_start", rs), ("ren_member", rm)):
        for i, x in enumerate(vals):
            getattr(mv, name)[i] = x
    return mv


def _args(K=16, **kw):
    p = C.c_void_p(16)
    base = dict(rays_per_sample=4, K=K, rays=p, z_samp=p, rgb=p, depth=p, sigma_raw=p, trans=p, reserved_=0)
    base.update(kw)
    return _lib.BtsRenderArgs(**base)


def _bad(edit, **kw):
    mv = _field(**kw)
    edit(mv)
    return mv


INVALID = {
    "V < 1": (lambda mv: setattr(mv, "V", 0), b"encoder views"),
    "V above the limit": (lambda mv: setattr(mv, "V", 9), b"encoder views"),
    "no encoder group": (lambda mv: setattr(mv, "n_enc_groups", 0), b"groups"),
    "encoder groups above the limit": (lambda mv: setattr(mv, "n_enc_groups", 9), b"groups"),
    "render groups above the limit": (lambda mv: setattr(mv, "n_ren_groups", 9), b"groups"),
    "member out of range": (lambda mv: mv.enc_member.__setitem__(1, 3), b"is not one of"),
    "negative member": (lambda mv: mv.enc_member.__setitem__(0, -1), b"is not one of"),
    "render member out of range": (lambda mv: mv.ren_member.__setitem__(2, 3), b"is not one of"),
    "view in two groups": (lambda mv: mv.enc_member.__setitem__(2, 0), b"two groups"),
    "render view in two groups": (lambda mv: mv.ren_member.__setitem__(1, 0), b"two groups"),
    "empty group": (lambda mv: mv.enc_group_start.__setitem__(1, 0), b"empty"),
    "table does not start at 0": (lambda mv: mv.enc_group_start.__setitem__(0, 1), b"start at member 0"),
    "table past its end": (lambda mv: mv.ren_group_start.__setitem__(2, 9), b"runs past"),
    "multiplicity 0": (lambda mv: mv.enc_mult.__setitem__(0, 0), b"multiplicity"),
    "multiplicity 3": (lambda mv: mv.enc_mult.__setitem__(1, 3), b"multiplicity"),
    "NULL map of view 1": (lambda mv: setattr(mv.view[1], "proj_nhwc", None), b"required"),
    "NULL camera of view 2": (lambda mv: setattr(mv.view[2], "w2c_enc", None), b"required"),
    "NULL parameters": (lambda mv: setattr(mv.view[0], "mlp_params", None), b"NULL"),
    "NULL frames": (lambda mv: setattr(mv.view[0], "imgs_nhwc4", None), b"NULL"),
    "NULL empty feature": (lambda mv: setattr(mv.view[0], "empty_feature", None), b"empty_feature"),
    "no render view": (lambda mv: setattr(mv.cfg[0], "nv", 0), b"render views"),
}
UNSUPPORTED = {
    "C differs": (lambda mv: setattr(mv.cfg[1], "C", 32), b"differs"),
    "d_hidden differs": (lambda mv: setattr(mv.cfg[2], "d_hidden", 32), b"differs"),
    "n_blocks differs": (lambda mv: setattr(mv.cfg[1], "n_blocks", 1), b"differs"),
    "map size differs": (lambda mv: setattr(mv.cfg[1], "W", 32), b"differs"),
    "feat_shift differs": (lambda mv: setattr(mv.cfg[2], "feat_shift", 1), b"differs"),
    "batch differs": (lambda mv: setattr(mv.cfg[1], "n", 2), b"differs"),
}


@pytest.mark.parametrize("case", list(INVALID) + list(UNSUPPORTED))
def test_a_bad_field_is_a_code_with_a_message_at_every_entry(lib, case):
    edit, text = INVALID.get(case) or UNSUPPORTED[case]
    code = -1 if case in INVALID else -2
    mv, a, g, p = _bad(edit), _args(), _lib.BtsRenderGrads(), C.c_void_p(16)
    calls = (lambda: lib.bts_render_fwd_multi_view(C.byref(mv), C.byref(a), None),
             lambda: lib.bts_render_bwd_multi_view(C.byref(mv), C.byref(a), C.byref(g), None, None, p, 1 << 40, None),
             lambda: lib.bts_field_query_multi_view(C.byref(mv), p, 4, p, p, p, None))
    for call in calls:
        assert call() == code, case
        assert text in lib.bts_last_error(), (case, lib.bts_last_error())


def test_shapes_outside_the_envelope_are_unsupported(lib):
    mv = _field(C_=48)
    assert lib.bts_render_fwd_multi_view(C.byref(mv), C.byref(_args()), None) == -2 and b"envelope" in lib.bts_last_error()
    assert lib.bts_field_query_multi_view(C.byref(mv), C.c_void_p(16), 4, None, None, C.c_void_p(16), None) == -2


def test_argument_errors(lib):
    mv, p = _field(), C.c_void_p(16)
    assert lib.bts_render_fwd_multi_view(None, None, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_field_query_multi_view(None, None, 0, None, None, None, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_render_fwd_multi_view(C.byref(mv), None, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_render_fwd_multi_view(C.byref(mv), C.byref(_args(rgb=None)), None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_render_bwd_multi_view(C.byref(mv), C.byref(_args(trans=None)), C.byref(_lib.BtsRenderGrads()), None, None, p, 1 << 40, None) == -1
    assert lib.bts_render_bwd_multi_view(C.byref(mv), C.byref(_args()), None, None, None, p, 1 << 40, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_field_query_multi_view(C.byref(mv), p, 0, None, None, p, None) == -1
    assert lib.bts_field_query_multi_view(C.byref(mv), p, 4, None, None, None, None) == -1
    # whole rays of at most 256 samples; no per-ray invalid sums
    assert lib.bts_render_fwd_multi_view(C.byref(mv), C.byref(_args(K=257)), None) == -2 and b"256" in lib.bts_last_error()
    for key in ("invalid_wsum", "invalid_any"):
        assert lib.bts_render_fwd_multi_view(C.byref(mv), C.byref(_args(**{key: p})), None) == -2 and b"invalid_wsum" in lib.bts_last_error()
    # short workspace: two row buffers (u0 and one view's rows), the slots, c_v per view
    a = _args()
    need = lib.bts_render_bwd_multi_view_workspace(C.byref(mv), C.byref(a))
    assert need >= 4 * 16 * 4 * (2 * 64 + 2 + 3)
    assert lib.bts_render_bwd_multi_view(C.byref(mv), C.byref(a), C.byref(_lib.BtsRenderGrads()), None, None, p, need - 1, None) == -4
    assert b"workspace" in lib.bts_last_error()
    assert lib.bts_render_bwd_multi_view_workspace(None, C.byref(a)) == 0 and lib.bts_render_bwd_multi_view_workspace(C.byref(mv), None) == 0


def _kernel_rule(tables, flags):
    """What the kernels do with the tables (csrc/bts_multi_view.hip: mv_field): per group the first member whose flag is clear, else the
    first member; c_v = multiplicity / T.  flags (V,) bools -> (c (V,), T, any of the picked flags)"""
    start, member, mult = tables
    T = sum(mult)
    c, any_flag = [0.0] * len(flags), False
    for g in range(len(mult)):
        members = member[start[g]:start[g + 1]]
        pick = next((v for v in members if not flags[v]), members[0])
        c[pick] += mult[g] / T
        any_flag = any_flag or flags[pick]
    return c, T, any_flag


GROUPINGS = [None, [[0]], [[0, 1]], [[1, 0]], [[0, 1, 2]], [[2, 0, 1]], [[0, 1], [2]], [[2], [1, 0]], [[0], [1]], [[0], [1], [2]],
             [[0, 1, 2], [3]], [[1, 0], [3, 2]], [[0], [2, 1], [3]], [[3, 1, 0], [2]]]


@pytest.mark.parametrize("groups", GROUPINGS, ids=[str(g) for g in GROUPINGS])
@pytest.mark.parametrize("singles_twice", [True, False], ids=["features", "colours"])
def test_group_tables_reproduce_merge_groups_on_every_flag_pattern(groups, singles_twice):
    V = 3 if groups is None else 1 + max(max(g) for g in groups)
    tables = native.group_tables(groups, V, singles_twice)
    patterns = list(itertools.product([False, True], repeat=V))
    outside = torch.tensor(patterns).t().reshape(1, V, len(patterns), 1)                    # (n, V, P, 1): point p has pattern p
    values = torch.eye(V).view(1, V, 1, V).expand(1, V, len(patterns), V).contiguous()       # view v's entry is e_v: the mean is c
    if groups is None:
        merged, flags = values, outside
    else:
        merged, flags = torch_modes._merge_groups(values, outside, groups, singles_twice=singles_twice)
    assert merged.shape[1] == sum(tables[2])                                                 # T, singles counted twice included
    mean, any_flag = merged.mean(dim=1)[0], torch.any(flags, dim=1)[0, :, 0]
    for p, pattern in enumerate(patterns):
        c, T, flag = _kernel_rule(tables, pattern)
        assert T == merged.shape[1]
        assert torch.allclose(mean[p], torch.tensor(c), atol=1e-7, rtol=0), (groups, pattern)
        assert bool(any_flag[p]) == flag, (groups, pattern)
        if not singles_twice and groups is not None:      # the colour merge: one entry per group, its flag the picked member's
            for g, grp in enumerate(groups):
                pick = next((v for v in grp if not pattern[v]), grp[0])
                assert torch.equal(merged[0, g, p], values[0, pick, p]) and bool(flags[0, g, p, 0]) == pattern[pick]


def test_multiplicities_and_T():
    assert native.group_tables([[0, 1], [2]], 3, True) == ([0, 2, 3], [0, 1, 2], [1, 2])       # the fixture's case a: T = 3
    assert native.group_tables([[0, 1], [2]], 3, False) == ([0, 2, 3], [0, 1, 2], [1, 1])
    assert native.group_tables([[0], [1], [2, 3]], 4, True)[2] == [2, 2, 1]                    # T = 5 with V = 4
    assert native.group_tables(None, 2, True) == ([0, 1, 2], [0, 1], [1, 1])                   # no combine_ids: the plain mean


def _conf(**kw):
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=True, code_mode="z",
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="feature_map", size=(8, 16), d_out=64, num_views=3),
                mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=64), mlp_fine=dict(type="empty"))
    conf.update(kw)
    return conf


def _scene():
    from oracle import bts_oracle as O
    return O.synthetic_scene(1, 4, 8, 16, 64, seed=0)


@pytest.mark.parametrize("enc", [dict(ids_encoder=[0, 2, 3], ids_render=[1, 2], combine_ids=[(0, 2)]), dict(ids_encoder=[0, 1, 2], ids_render=[3])],
                         ids=["combine_ids", "several ids_encoder"])
def test_the_key_keeps_encode_off_the_composition(enc):
    s = _scene()
    net = bts.BTSNet(_conf(native_multi_view=True)).eval()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch_modes._warned.discard("combine_ids / several encoder views")
        # (the hand-over into the kernels' layouts is HIP: on CPU tensors encode says so loudly -- after it has chosen its path)
        with pytest.raises(bts.BtsNativeError, match="GPU"):
            net.encode(s["images"], s["projs"], s["poses"], **enc)
    assert not net.torch_mode and net.multi_view
    assert not [w for w in seen if "PyTorch composition" in str(w.message)]


def test_without_the_key_nothing_changes():
    s = _scene()
    net = bts.BTSNet(_conf()).eval()
    assert not net.native_multi_view
    torch_modes._warned.discard("combine_ids / several encoder views")
    with pytest.warns(UserWarning, match="PyTorch composition"):
        net.encode(s["images"], s["projs"], s["poses"], ids_encoder=[0, 2, 3], ids_render=[1, 2], combine_ids=[(0, 2)])
    assert net.torch_mode and not net.multi_view
    assert net.grid_f_combine == [[0, 1], [2]] and net.grid_c_combine == [[1], [0]]
    with pytest.raises(bts.BtsNativeError, match="PyTorch composition"):
        net.native_field()
    # one encoder view: the key changes nothing either
    single = bts.BTSNet(_conf(native_multi_view=True, encoder=dict(type="feature_map", size=(8, 16), d_out=64)))
    assert not single.torch_mode and not single.multi_view


def test_both_unshipped_modes_at_once_stay_on_the_composition():
    net = bts.BTSNet(_conf(sample_color=False, native_mlp_color=True, native_multi_view=True))
    net._combined = True
    assert net.torch_mode and not net.multi_view


def test_single_view_only_paths_name_the_encoder_views():
    net = bts.BTSNet(_conf(native_multi_view=True)).train()
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=64, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).train()
    sampler = bts.PatchRaySampler(ray_batch_size=256, z_near=3.0, z_far=80.0, patch_size=8)
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_edge_aware_smoothness": 0.001})
    step = bts.FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit)
    assert "more than one encoder view" in step.why_not(None, ids_encoder=[0, 2], ids_render=[1, 3], ids_loss=[0, 1])
    net.eval(), renderer.eval()
    frame = bts.FusedEvalFrame(renderer.bind_parallel(net).eval(), bts.ImageRaySampler(3.0, 80.0, 8, 16))
    assert "more than one encoder view" in frame.why_not(None, ids_encoder=[0, 2], ids_render=[0])
    net._combined = True
    from behindthescenes_amd import novel_views
    assert "more than one encoder view" in novel_views._why_not(renderer.bind_parallel(net).eval(), bts.ImageRaySampler(3.0, 80.0, 8, 16))
    with pytest.raises(bts.BtsNativeError, match="more than one encoder view"):
        net.occupancy_profile(torch.zeros(1, 8, 3), 2)
