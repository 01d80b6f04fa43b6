"""CPU (no GPU, no kernel launches): the argument checks of the projection and render entry points, pinned call by call -- the return code
and the WHOLE bts_last_error() text of calls that fail validation.  Every call here is rejected before anything is enqueued; the pointers
are fakes (16) that nothing dereferences."""
import ctypes as C

import pytest

from behindthescenes_amd import _lib, native
from behindthescenes_amd.build import build_library

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
P = 16          # a non-NULL pointer that is never followed


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


def _cfg(C_=64, H=32, W=96, nv=2, feat_shift=0, enc_view=-1, d_hidden=64, n_blocks=0):
    cfg = native._spec_cfg(native.FieldSpec(C=C_, d_hidden=d_hidden, n_blocks=n_blocks), n=2, H=H, W=W, nv=nv, feat_shift=feat_shift)
    cfg.enc_render_view = enc_view
    return cfg


OK = _cfg()
ODD = _cfg(C_=48)                               # outside the compiled envelope
SHIFT = _cfg(H=36, W=100, feat_shift=3)         # H, W no multiples of 2^feat_shift
# the compiled shapes (C, d_hidden, n_blocks); the odd shapes: C = 48 and two neighbours of the supported set, each one field away from a
# compiled shape
SHAPES = {(64, 64, 0), (32, 32, 1), (32, 32, 0)}
ODD_SHAPES = {"C48": (48, 64, 0), "C64_blocks1": (64, 64, 1), "C32_hidden64": (32, 64, 0)}
ODD_CFGS = {k: _cfg(C_=c, d_hidden=hd, n_blocks=nb) for k, (c, hd, nb) in ODD_SHAPES.items()}

NULL_SIZE = "%s: NULL pointer or non-positive size"
ENVELOPE = "%s: configuration outside the compiled envelope (C=%d d_hidden=%d n_blocks=%d)"
BAD_SHIFT = "%s: feat_shift=3 needs 0 <= feat_shift <= 6 and H=36, W=100 multiples of 2^feat_shift"

# entry -> (its arguments behind cfg with every pointer given and N = 1, index of N, index of a required pointer, index of `tiles` where the
# entry REQUIRES the flags, indices of (feature map, d_mlp_params) for the backward forms)
PROJECTION = {
    "bts_project_features":           ([P, P, 1, P, None], 2, 0, None, None),
    "bts_project_features_tiles":     ([P, P, 1, P, P, None], 2, 1, 3, None),
    "bts_project_features_cl":        ([P, P, 1, P, P, None], 2, 4, None, None),
    "bts_project_features_bwd":       ([P, P, P, 1, P, P, None], 3, 1, None, (0, 5)),
    "bts_project_features_bwd_tiles": ([P, P, P, P, 1, P, P, 1, None], 4, 3, 2, (0, 6)),
    "bts_project_features_bwd_cl":    ([P, P, P, P, 1, P, P, 1, None], 4, 1, None, (0, 6)),
}


def _projection_cases():
    for name, (args, i_n, i_ptr, i_tiles, bwd) in PROJECTION.items():
        def but(i, v, args=args):
            return args[:i] + [v] + args[i + 1:]
        yield f"{name}-null", name, [OK] + but(i_ptr, None), INVALID, NULL_SIZE % name
        yield f"{name}-null_cfg", name, [None] + args, INVALID, NULL_SIZE % name
        yield f"{name}-N0", name, [OK] + but(i_n, 0), INVALID, NULL_SIZE % name
        for odd, shape in ODD_SHAPES.items():
            yield f"{name}-{odd}", name, [ODD_CFGS[odd]] + args, UNSUPPORTED, ENVELOPE % ((name,) + shape)
        yield f"{name}-shift", name, [SHIFT] + args, INVALID, BAD_SHIFT % name
        # a doubly wrong call reports the first check that fails: NULL / size, then the envelope, then feat_shift
        yield f"{name}-null_and_C48", name, [ODD] + but(i_ptr, None), INVALID, NULL_SIZE % name
        if i_tiles is not None:
            yield f"{name}-null_tiles", name, [OK] + but(i_tiles, None), INVALID, NULL_SIZE % name
        if bwd is not None:
            yield f"{name}-d_mlp_without_map", name, [OK] + but(bwd[0], None), INVALID, NULL_SIZE % name


TENS = dict(feat_nhwc=P, proj_nhwc=P, K_enc=P, w2c_enc=P, imgs_nhwc4=P, K_r=P, w2c_r=P, empty_feature=P, mlp_params=P)
FWD_ARGS = dict(rays_per_sample=320, K=16, hard_alpha_cap=1, rays=P, z_samp=P, rgb=P, depth=P)
BWD_ARGS = dict(rays_per_sample=320, K=16, hard_alpha_cap=1, rays=P, z_samp=P, sigma_raw=P, trans=P)

FWD_NULL = "%s: NULL render argument (rays, z_samp or jitter, rgb and depth are required)"
BWD_NULL = "%s: NULL argument (rays, z_samp, the forward's sigma_raw + trans and proj_nhwc are required)"
MC_BWD_NULL = "%s: NULL argument (rays, z_samp and the forward's sigma_raw + trans are required)"
SIZES = "%s: non-positive rays_per_sample=%d K=%d"
WS = "%s: workspace too small (%d bytes needed)"

# bts_render_bwd_workspace of OK with BWD_ARGS: 20 B per sample rounded to 16 + the eight slot copies of dW_pe / db_in (tests/test_abi_cpu.py)
WS_PLAIN = (2 * 320 * (16 * 3 + 128) * 4 + 15) // 16 * 16 + 8 * 40 * 64 * 4
# bts_render_bwd_mlp_color_workspace: the gradient row + g_s per sample, the same slot copies behind them
WS_MC = (2 * 320 * 16 * (64 + 1) * 4 + 15) // 16 * 16 + 8 * 40 * 64 * 4


def _render_cases():
    def args(base, **kw):
        return _lib.BtsRenderArgs(**{**base, **kw})
    tens, grads = _lib.BtsFieldTensors(**TENS), _lib.BtsRenderGrads(g_rgb=P)
    mc = _cfg(nv=1)
    for name, cfg, base, null_msg, bwd in (("bts_render_fwd", OK, FWD_ARGS, FWD_NULL, False), ("bts_render_bwd", OK, BWD_ARGS, BWD_NULL, True),
                                           ("bts_render_fwd_mlp_color", mc, FWD_ARGS, FWD_NULL, False),
                                           ("bts_render_bwd_mlp_color", mc, BWD_ARGS, MC_BWD_NULL, True)):
        is_mc = name.endswith("mlp_color")

        def call(a, g=grads, ws=P, ws_bytes=1 << 40, cfg=cfg, tens=tens, bwd=bwd):
            return [cfg, tens, a] + ([g, ws, ws_bytes] if bwd else []) + [None]
        yield f"{name}-null_args", name, call(None), INVALID, null_msg % name
        yield f"{name}-no_z_samp_no_jitter", name, call(args(base, z_samp=None)), INVALID, null_msg % name
        yield f"{name}-null_rays", name, call(args(base, rays=None)), INVALID, null_msg % name
        yield f"{name}-K0", name, call(args(base, K=0)), INVALID, SIZES % (name, 320, 0)
        yield f"{name}-rays0", name, call(args(base, rays_per_sample=0)), INVALID, SIZES % (name, 0, 16)
        yield f"{name}-null_and_K0", name, call(args(base, rays=None, K=0)), INVALID, null_msg % name
        if not bwd:
            yield f"{name}-null_rgb", name, call(args(base, rgb=None)), INVALID, null_msg % name
        else:
            need = WS_MC if is_mc else WS_PLAIN
            yield f"{name}-null_trans", name, call(args(base, trans=None)), INVALID, null_msg % name
            yield f"{name}-null_grads", name, call(args(base), g=None), INVALID, \
                ("%s: NULL gradient struct" if is_mc else null_msg) % name
            yield f"{name}-null_workspace", name, call(args(base), ws=None), WORKSPACE, WS % (name, need)
            yield f"{name}-small_workspace", name, call(args(base), ws_bytes=need - 1), WORKSPACE, WS % (name, need)
            # the argument checks come before the workspace's
            yield f"{name}-K0_and_small_workspace", name, call(args(base, K=0), ws_bytes=0), INVALID, SIZES % (name, 320, 0)
        if is_mc:
            yield f"{name}-nv2", name, call(args(base), cfg=OK), INVALID, \
                f"{name}: nv=2, but MLP-predicted colour has exactly one colour output (nv = 1, models_bts.py:321)"
            yield f"{name}-enc_render_view0", name, call(args(base), cfg=_cfg(nv=1, enc_view=0)), INVALID, \
                f"{name}: enc_render_view=0 must be -1 (this head has no render views)"
            yield f"{name}-K257", name, call(args(base, K=257)), UNSUPPORTED, \
                f"{name}: K=257 samples per ray; this head's kernels take whole rays of at most 256 samples per work-group"
            yield f"{name}-no_proj", name, call(args(base), tens=_lib.BtsFieldTensors(**{**TENS, "proj_nhwc": None})), INVALID, \
                f"{name}: the projected feature map (proj_nhwc) is required"
            if not bwd:
                for k in ("invalid_wsum", "invalid_any"):
                    yield f"{name}-{k}", name, call(args(base, **{k: P})), UNSUPPORTED, \
                        f"{name}: invalid_wsum / invalid_any are not produced for MLP-predicted colour (request weights and invalid)"
            else:   # the backward takes no offence at invalid_wsum: the call fails at the NEXT check
                yield f"{name}-invalid_wsum", name, call(args(base, invalid_wsum=P), g=None), INVALID, f"{name}: NULL gradient struct"
        else:
            # the field checks come first and speak as "bts"
            yield f"{name}-null_cfg", name, [None, tens, args(base)] + call(None)[3:], INVALID, "bts: NULL cfg/tensors"
            for odd, shape in ODD_SHAPES.items():
                yield f"{name}-{odd}", name, call(args(base), cfg=ODD_CFGS[odd]), UNSUPPORTED, \
                    "bts: configuration outside the compiled envelope (C=%d d_hidden=%d n_blocks=%d; also needs num_freqs=6, nv<=8)" % shape
            yield f"{name}-shift", name, call(args(base), cfg=SHIFT), INVALID, BAD_SHIFT % "bts"
            if bwd:
                yield f"{name}-no_proj", name, call(args(base), tens=_lib.BtsFieldTensors(**{**TENS, "proj_nhwc": None})), INVALID, null_msg % name


CASES = list(_projection_cases()) + list(_render_cases())


def test_the_table_covers_every_entry():
    names = {c[1] for c in CASES}
    assert names == set(PROJECTION) | {"bts_render_fwd", "bts_render_bwd", "bts_render_fwd_mlp_color", "bts_render_bwd_mlp_color"}
    assert len({c[0] for c in CASES}) == len(CASES)


def test_workspace_sizes_in_the_messages_are_the_library_s(lib):
    a = _lib.BtsRenderArgs(**BWD_ARGS)
    assert lib.bts_render_bwd_workspace(C.byref(OK), C.byref(a)) == WS_PLAIN
    assert lib.bts_render_bwd_mlp_color_workspace(C.byref(_cfg(nv=1)), C.byref(a)) == WS_MC


def test_bts_supported_answers_1_for_exactly_the_compiled_shapes(lib):
    for c in (16, 32, 48, 64):
        for hd in (32, 64):
            for nb in (0, 1, 2):
                assert lib.bts_supported(C.byref(_cfg(C_=c, d_hidden=hd, n_blocks=nb))) == (1 if (c, hd, nb) in SHAPES else 0), (c, hd, nb)


@pytest.mark.parametrize("name,args,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_rejected_call_answers_its_code_and_its_whole_message(lib, name, args, code, message):
    args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
    assert getattr(lib, name)(*args) == code
    assert lib.bts_last_error().decode() == message
