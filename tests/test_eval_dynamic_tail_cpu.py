"""The host's split of a render launch into fixed ray lists and a claimed tail (render_dyn_first of bts_fwd.hip, through the exported
bts_render_dyn_first): no GPU needed."""
import ctypes as C

import pytest

from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library


@pytest.fixture(scope="module")
def split():
    build_library()
    lib = _lib.load()

    def f(grid, groups):
        c = C.c_int32(-1)
        return int(lib.bts_render_dyn_first(grid, groups, C.byref(c))), int(c.value)
    return f


def _grid(groups, cus):
    return (min((groups + 3) // 4, 2 * cus) + 7) // 8 * 8      # render_grid: 2 work-groups per CU, a multiple of 8


GROUPS = [1, 7, 64, 512, 2047, 2048, 2049, 3840, 4095, 4096, 4097, 7680, 8000, 8192, 12345, 24576, 65536, 100000, 245760, 245761, 1 << 20,
          3 * (1 << 20) + 17, 0x7FF00000]


@pytest.mark.parametrize("cus", [8, 64, 256, 304])
def test_split_is_chunk_aligned_and_covers_every_group_once(split, cus):
    for groups in GROUPS:
        grid = _grid(groups, cus)
        first, chl = split(grid, groups)
        waves, unit = grid * 4, 8 << chl
        assert 6 <= chl <= 20
        assert 0 < first <= groups
        if first == groups:
            continue                      # no tail: the fixed lists hold every group, as without a counter
        assert first % unit == 0          # whole chunks on every XCD
        assert first >= waves             # every wave has a group of its own in front of its first ticket
        assert groups - first >= groups // 8 and groups - first < groups // 8 + unit    # an eighth, rounded up to the chunk
        # position i of XCD x's chunk list is group ((i >> chl) * 8 + x) << chl | i & (chunk - 1) while that is a group.  Fixed lists:
        # i < first / 8; ticket t of XCD x: i = first / 8 + t, until the first position that is no group.  Together every group exactly
        # once, the fixed part exactly [0, first) (counted on the small launches)
        if groups <= 100000:
            seen, n_chunks = [0] * groups, (groups + (1 << chl) - 1) >> chl
            for x in range(8):
                i = 0
                while True:
                    c = ((i >> chl) << 3) + x
                    g = (c << chl) + (i & ((1 << chl) - 1))
                    if c >= n_chunks or g >= groups:
                        break
                    assert (g < first) == (i < first // 8)
                    seen[g] += 1
                    i += 1
                for k in range(i, i + 3 * waves, 97):      # ... and no group behind it: a ticket past the end ends the wave
                    c = ((k >> chl) << 3) + x
                    assert c >= n_chunks or (c << chl) + (k & ((1 << chl) - 1)) >= groups
            assert min(seen) == 1 and max(seen) == 1


def test_no_tail_below_the_size_threshold(split):
    for cus in (64, 256):
        for groups in range(1, 8 * cus + 1, 37):          # fewer groups than waves: one round of the grid at most
            first, _ = split(_grid(groups, cus), groups)
            assert first == groups
    # 256 CUs = 2 048 waves: a tail needs 2 048 groups in front of it
    assert split(512, 2048) == (2048, split(512, 2048)[1])
    assert split(512, 3840)[0] == 3072 and split(512, 7680)[0] == 6144 and split(512, 245760)[0] == 212992
    assert split(128, 512)[0] == 512
