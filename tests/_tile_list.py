"""White-box observer of the list-driven projection passes of the fused training step (tests/test_gpu_tile_list.py,
tests/test_gpu_fused_anchor.py): reads the tile lists back from the arena's backward workspace.

The layout is the one include/bts_render.h documents for ``BtsTrainStep.bwd_workspace`` (csrc/bts_prep.hip: compact_tiles_kernel,
project_bwd_list_bytes; csrc/bts_train.hip: the slices):

* a list of a map with ``n_tiles`` tiles takes L = (4 + n_tiles) * 4 + n_tiles + 16 bytes: int32[0] the count, int32[1 .. 3] zero,
  int32[4 ..] the indices (no particular order); in the backward a copy of the flags, one byte per tile, follows at byte (4 + n_tiles) * 4;
* the forward of scale s writes at byte s * slice, slice = (workspace bytes / n_scales) & ~255, when slice >= L;
* the backward of scale s writes at the start of the workspace -- with concurrent_scales at s * (bts_render_bwd_workspace rounded up to
  256) -- when bts_render_bwd_workspace minus pass C's slot copies (8 x 40 x d_hidden floats at its end) >= L;
* either only for maps of at least LIST_MIN_TILES tiles (BTS_LIST_MIN_TILES; 1 in the "listall" variant of behindthescenes_amd/build.py)."""
import ctypes as C
import os

import torch

POISON = float("nan")


def list_min_tiles():
    """The threshold the loaded library is EXPECTED to have been built with: 4096, or what the process that launched this one with
    another library says (tests/test_gpu_tile_list.py::test_listall_variant sets 1 next to BTS_RENDER_LIB).  Only an expectation: the
    observer below is what shows which form ran."""
    return int(os.environ.get("BTS_TEST_LIST_MIN_TILES", "4096"))


def list_bytes(n_tiles):
    return (4 + n_tiles) * 4 + n_tiles + 16


def the_arena():
    from behindthescenes_amd import train_step as TS
    arenas = [a for pool in TS._ARENAS.values() for a in pool]
    assert len(arenas) == 1, f"{len(arenas)} arenas: release_arenas() before the step under observation"
    return arenas[0]


def ws_bytes(arena):
    return arena.ws.numel() * 4


def render_bwd_need(net, n, H, W, nv, Bp, K):
    """bts_render_bwd_workspace of the step (the same for every scale: it depends on the rays only), as FusedTrainStep sizes its arena."""
    from behindthescenes_amd import _lib, native
    cfg0 = native._spec_cfg(net.spec, n, H, W, nv, 0, -1)
    args = _lib.BtsRenderArgs(rays_per_sample=Bp, K=K)
    return int(_lib.load().bts_render_bwd_workspace(C.byref(cfg0), C.byref(args)))


def fwd_slice(arena):
    return (ws_bytes(arena) // len(arena.scales)) & ~255


def bwd_capacity(need, d_hidden):
    return need - 4 * 8 * 40 * d_hidden


def bwd_offset(need, s, concurrent):
    return ((need + 255) & ~255) * s if concurrent else 0


def expect_list(n_tiles, capacity):
    return n_tiles >= list_min_tiles() and capacity >= list_bytes(n_tiles)


def poison(arena):
    """NaN words (0x7FC00000) over the whole workspace: 'contents need no initialisation', and no count, index or flag byte pattern."""
    arena.ws.fill_(POISON)


def read_list(arena, offset, n_tiles, with_copy):
    """-> (indices sorted (count,) int64, copy (n_tiles,) uint8 | None), or None when the bytes at `offset` are not a well-formed list: count
    in range, three zero words, indices in range without duplicates, and (backward) flag bytes 0 / 1 whose set positions ARE the indices."""
    torch.cuda.synchronize()
    if offset + list_bytes(n_tiles) - 16 > ws_bytes(arena):
        return None
    raw = arena.ws.view(torch.uint8)
    head = raw[offset:offset + (4 + n_tiles) * 4].view(torch.int32).cpu()
    count = int(head[0])
    if not (0 <= count <= n_tiles) or head[1:4].any():
        return None
    idx = head[4:4 + count].long().sort().values
    if count and (idx[0] < 0 or idx[-1] >= n_tiles or (idx[1:] == idx[:-1]).any()):
        return None
    if not with_copy:
        return idx, None
    copy = raw[offset + (4 + n_tiles) * 4:offset + (4 + n_tiles) * 4 + n_tiles].cpu()
    if copy.max() > 1 or int(copy.sum()) != count or not torch.equal(torch.nonzero(copy).flatten(), idx):
        return None
    return idx, copy


def check_forward_list(arena, s, want):
    """After the forward, before backward(): scale s's list is there and IS the sampled set (`want`), or is not there (the flag form ran).
    -> the sampled flags (n, tiles per image) uint8 on the CPU."""
    tiles = arena.scales[s]["tiles"]
    n_tiles = tiles.numel()
    got = read_list(arena, s * fwd_slice(arena), n_tiles, with_copy=False)
    flags = tiles.cpu()
    on = torch.nonzero(flags.flatten()).flatten()
    assert on.numel() > 0
    ran = got is not None and torch.equal(got[0], on)
    if want:
        assert got is not None, f"scale {s}: no well-formed tile list in the forward's slice ({n_tiles} tiles): the flag form ran"
        assert got[0].numel() == on.numel(), f"scale {s}: the list counts {got[0].numel()} tiles, {on.numel()} are flagged"
        assert ran, f"scale {s}: the forward's list is not the set of flagged tiles"
    else:
        assert not ran, f"scale {s}: a tile list was written for a map of {n_tiles} tiles (slice {fwd_slice(arena)} bytes)"
    return flags


def dirty_texels(copy, n, h, w, blocks):
    from behindthescenes_amd import native
    return copy.view(n, -1).bool()[:, native.proj_tile_map(h, w, blocks)]        # (n, h, w)


def check_backward_list(arena, s, offset, want, sampled, d_feat, blocks):
    """After the backward: scale s's list and flag copy at `offset` are consistent, the dirty set is inside the forward's sampled set and
    covers every texel with a non-zero feature gradient (`blocks`: the map is channels-last, 16 x 4 block tiles) -- or no such list is there
    (the flag form ran).  -> the flag copy | None."""
    sc = arena.scales[s]
    n, h, w, _ = sc["proj"].shape
    n_tiles = sc["tiles"].numel()
    got = read_list(arena, offset, n_tiles, with_copy=True)
    problems = []
    if got is None:
        problems.append("no well-formed list and flag copy")
    else:
        idx, copy = got
        if idx.numel() == 0:
            problems.append("an empty list")
        if (copy.view(n, -1) > sampled).any():
            problems.append("a dirty tile the forward did not sample")
        if d_feat is not None:
            nz = (d_feat.detach() != 0).any(dim=1).cpu()
            stray = int((nz & ~dirty_texels(copy, n, h, w, blocks)).sum())
            if stray:
                problems.append(f"{stray} texels with a gradient outside the dirty tiles")
    if want:
        assert not problems, f"scale {s} ({n_tiles} tiles): {problems}"
        return got[1]
    assert problems, f"scale {s}: a tile list was written by the backward for a map of {n_tiles} tiles"
    return None


def check_kept_pairs_are_clean(arena):
    for s, sc in enumerate(arena.scales):
        assert not sc["d_proj"].any() and not sc["d_tiles"].any(), f"scale {s}: (d_proj, d_tiles) left dirty"
