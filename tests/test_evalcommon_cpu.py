"""What the evaluators share (behindthescenes_amd/_evalcommon.py, native._req_as): pure host code, no GPU."""
import math

import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import bbox_occupancy as BB, lidar_occupancy as L, native
from behindthescenes_amd._evalcommon import MetricRows

# lidar_occupancy's names -> bbox_occupancy's, position by position
RENAMED = dict(zip(L.METRIC_KEYS, BB.METRIC_KEYS))

COUNTS = [[10, 20, 30, 40, 50, 60],     # all six positive
          [0, 0, 0, 0, 0, 0],           # everything empty
          [3, 4, 0, 0, 5, 6],           # o_rec: no occupied point (c2 + c3 = 0)
          [0, 7, 0, 2, 0, 9],           # o_prec: nothing predicted occupied (c0 + c2 + c4 = 0)
          [3, 4, 0, 0, 0, 0],           # ie_acc (and ie_rec, ie_prec, o_rec): every point visible
          [1, 2, 3, 4, 0, 0],           # ie_rec: no free invisible point (c4 + c5 = 0)
          [1, 2, 3, 0, 4, 0]]           # ie_prec: nothing invisible predicted free (c3 + c5 = 0)


def same(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, torch.Tensor):
        if a.dtype != b.dtype or a.dim() != 0 or b.dim() != 0 or a.device != b.device:
            return False
        a, b = a.item(), b.item()
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("c", COUNTS)
def test_both_evaluators_form_the_same_nine_ratios(c):
    lidar, bbox = L.metrics_from_counts(c), BB.metrics_from_counts(c + [17])      # the seventh entry (active boxes) is not a cell
    assert tuple(lidar) == L.METRIC_KEYS and tuple(bbox) == BB.METRIC_KEYS
    for k in L.METRIC_KEYS:
        assert same(lidar[k], bbox[RENAMED[k]]), (k, lidar[k], bbox[RENAMED[k]])
    # the reference's types (evaluator_lidar.py:319-340): .item() floats, except ie_rec / ie_prec / t_no_nop_nv, which stay tensors
    for k in ("o_acc", "o_rec", "o_prec", "ie_acc", "ie_r", "t_ie"):
        assert type(lidar[k]) is float, k
    for k in ("ie_rec", "ie_prec", "t_no_nop_nv"):
        assert isinstance(lidar[k], torch.Tensor) and lidar[k].dtype == torch.float32 and lidar[k].dim() == 0 and lidar[k].device.type == "cpu", k


def test_ratios_of_one_count_vector_by_hand():
    """[V&P, V&!P, !V&O&P, !V&O&!P, !V&!O&P, !V&!O&!P] = [10, 20, 30, 40, 50, 60], n = 210, through evaluator_lidar.py:319-330 by hand
    (O holds only where V does not): P == O in cells 1, 2, 5; O[P] = c2 / (c0 + c2 + c4); P[O] = c2 / (c2 + c3); !O & !V = c4 + c5;
    (P == O)[!V] = (c2 + c5) / (c2 + .. + c5); (!O)[!P & !V] = c5 / (c3 + c5); (!P)[!O & !V] = c5 / (c4 + c5).  The quotients are fp32
    divisions (a mean of a float tensor), written here to more digits than fp32 holds."""
    def f32(x):
        return torch.tensor(x, dtype=torch.float32).item()
    m = L.metrics_from_counts([10, 20, 30, 40, 50, 60])
    assert m["o_acc"] == f32(0.5238095238095238)        # 110 / 210
    assert m["o_rec"] == f32(0.42857142857142855)       # 30 / 70
    assert m["o_prec"] == f32(0.3333333333333333)       # 30 / 90
    assert m["ie_acc"] == 0.5                           # 90 / 180
    assert m["ie_rec"].item() == f32(0.5454545454545454)    # 60 / 110
    assert m["ie_prec"].item() == f32(0.6)              # 60 / 100
    assert m["ie_r"] == f32(0.5238095238095238)         # 110 / 210
    assert m["t_ie"] == 110.0 and m["t_no_nop_nv"].item() == 60.0
    empty = L.metrics_from_counts([3, 4, 0, 0, 0, 0])   # nothing invisible: the means over !V are means of nothing
    assert all(math.isnan(float(empty[k])) for k in ("o_rec", "ie_acc", "ie_rec", "ie_prec")) and empty["o_acc"] == f32(4 / 7)


def test_metric_rows_mean_skips_nan_in_fp64_and_never_wraps():
    r = MetricRows(5, torch.float32, 4, "Rows")
    cpu = torch.device("cpu")
    inf, nan = float("inf"), float("nan")
    filled = [[1.0, nan, 1.0, 0.5, 7.0], [nan, nan, inf, 0.25, 7.0], [3.0, nan, 2.0, 0.125, 7.0], [4.5, nan, 3.0, 2.0, 7.0]]
    for k, vals in enumerate(filled):
        row = r.next_row(cpu)
        assert row.shape == (1, 5) and r.n_frames == k      # the writer counts the row once it is written
        row[0] = torch.tensor(vals)
        r.n_frames += 1
    assert r.rows.shape == (4, 5) and r.rows.dtype == torch.float32 and r.capacity == 4
    keys = ("a", "all_nan", "with_inf", "d")                # the first len(keys) columns
    want = {}
    for i, k in enumerate(keys):
        kept = [float(torch.tensor(v[i], dtype=torch.float32)) for v in filled if not math.isnan(v[i])]     # fp64 of the stored fp32 values
        want[k] = sum(kept) / len(kept) if kept else nan    # (every sum here is exact in fp64, whatever its order)
    got = r.means(keys)
    assert tuple(got) == keys and got["a"] == want["a"] == 8.5 / 3 and math.isnan(got["all_nan"]) and got["with_inf"] == inf
    assert got["d"] == want["d"] == 2.875 / 4 and all(type(v) is float for v in got.values())
    with pytest.raises(bts.BtsNativeError, match="Rows: 4 frames are stored"):
        r.next_row(cpu)
    with pytest.raises(bts.BtsNativeError, match="capacity"):
        r.full()
    r.reset()
    assert r.n_frames == 0 and not r.rows.any()
    assert r.next_row(cpu).data_ptr() == r.rows.data_ptr()  # the same buffer, from its first row
    with pytest.raises(bts.BtsNativeError, match="capacity"):
        MetricRows(5, torch.float32, 0, "Rows")


def test_the_one_tensor_checker_rejects_with_the_package_error():
    with pytest.raises(bts.BtsNativeError, match="expected a tensor"):
        native._req_as([1, 2], "x", torch.int32)
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        native._req_as(torch.zeros(2, dtype=torch.int32), "x", torch.int32)
    with pytest.raises(bts.BtsNativeError):
        native._req_as(torch.zeros(2, dtype=torch.float64), "x", torch.uint8)
    with pytest.raises(bts.BtsNativeError, match="x: must live on the GPU"):      # _req: the float32 case of the same checker
        native._req(torch.zeros(2), "x", (2,))
    assert native._addr(None) is None and native._addr(torch.zeros(1)) != 0
