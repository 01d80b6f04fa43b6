"""Golden fixture for the LiDAR ground-truth depth maps FROM THE REAL REFERENCE.  Run in the build container only:

    python -B tests/golden/gen_golden_lidar_depth.py

Imports the reference's datasets/kitti_raw/kitti_raw_dataset.py and datasets/kitti_360/kitti_360_dataset.py unmodified (cv2, torchvision
and the annotation module are stubbed before the import, ``np.int = int`` stands in for the alias kitti_raw:282 needs on current numpy)
and calls their two ``load_depth`` functions unbound on a minimal stand-in for ``self``: ``data_path`` a temporary directory with the
synthetic .bin files, ``_calibs``, ``target_image_size``, ``eigen_depth``.  kitti_raw reads its size from the module's BASE_SIZES, which
gets a fake day key per small size.  Nothing of the reference's source enters the repository; the inputs and the recorded maps do:
tests/golden/lidar_depth.npz.

Cases: (H, W) = (1, 2), (2, 2), (5, 7), (24, 40) x both conventions x fp32 / fp64 P, and kitti_raw with eigen_depth at (5, 7) and
(24, 40), where the crop's int32 truncation drops a row and a column.  The clouds are CONSTRUCTED (solved back from the pixel and the
depth every point is meant to have); per pair slot y -- the pixels R = (y, W - 1) and L = (y + 1, 0) share a key --
  type A (even y): R one point (index first), then two points in L whose last is not the nearer: R receives L's minimum, a depth from
                   another row; L keeps its last write;
  type B (odd y):  L one point (first), then two points in R: L receives R's minimum; R keeps its last write;
and apart from the pairs: a pixel of three points whose last is not its nearest, a pixel whose only point has a negative z (behind the
camera; kitti_raw's front filter drops it), a point with x < 0 and z > 0 that lands in frame (kitti_raw drops it, kitti_360 shows it),
points aimed at rows and columns -1, 0, H - 1, H, W - 1, W, and the cloud's origin point, whose u is P's fourth column EXACTLY in either
dtype: a coordinate on a half over a power-of-two u2 in EVERY case (kitti_raw: px = 2.5 -> 2, half away 3; kitti_360: (px * .5 + .5) * 2
= .5 -> 0 / 1 at W = 2, (py * .5 + .5) * 5 = 2.5 -> 2 / 3 at H = 5, .4375 * 24 = 10.5 -> 10 / 11 at H = 24).  What fits a size is said by
``expect`` below and COUNTED per case; at (1, 2) there is no pair, at (1, 2) and (2, 2) no pixel is free for a lone point, so the
front-filter point joins the three-point pixel as its nearest and there is no lone negative z (the origin point cannot carry one: with
u2 < 0 its pixel shows 0 wherever it lands, and the half would no longer tell rint from round-half-away in the map).
Asserted on the reference alone: no projected coordinate (but the constructed half) within 1e-2 pixel of a rounding boundary; the z
competing in one pixel or key group differ by at least 1e-3 relative; every mutant of tests/_lidar_depth_oracle.py differs from the
reference's map in every case where it can show (``shows`` below says where, and why not elsewhere).
Per pixel the file also records the source point (whose z the pixel shows) and that z evaluated exactly (rational arithmetic on the
stored P and point), as a double-double hi + lo: the GPU test measures its distances against it."""
import os
import sys
import tempfile
import types
from fractions import Fraction

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from oracle import ref_shim
import _lidar_depth_oracle as LD

OUT = os.path.join(HERE, "lidar_depth.npz")
SIZES = ((1, 2), (2, 2), (5, 7), (24, 40))
EIGEN_SIZES = ((5, 7), (24, 40))
T_Z = 0.5                       # P[2, 3]: the origin point's u2, a power of two
COORD_MARGIN, Z_REL = 1e-2, 1e-3


def load_datasets():
    """the reference's two data-set modules, imported unmodified"""
    ref_shim.load_reference()
    tr = sys.modules["torchvision.transforms"]
    if not hasattr(tr, "ColorJitter"):
        tr.ColorJitter = object
    if "datasets.kitti_360.annotation" not in sys.modules:
        m = types.ModuleType("datasets.kitti_360.annotation")
        m.KITTI360Bbox3D = object
        sys.modules["datasets.kitti_360.annotation"] = m
    if not hasattr(np, "int"):
        np.int = int            # kitti_raw_dataset.py:282
    import datasets.kitti_raw.kitti_raw_dataset as raw
    import datasets.kitti_360.kitti_360_dataset as k360
    return raw, k360


def day_key(size):
    return f"fake_{size[0]}x{size[1]}"


def reference_map(mods, tmp, points, P, size, convention, eigen):
    raw, k360 = mods
    if convention == "kitti_raw":
        raw.BASE_SIZES[day_key(size)] = tuple(size)
        d = os.path.join(tmp, day_key(size), "seq", "velodyne_points", "data")
        os.makedirs(d, exist_ok=True)
        points.tofile(os.path.join(d, f"{7:010d}.bin"))
        me = types.SimpleNamespace(data_path=tmp, eigen_depth=eigen)
        return raw.KittiRawDataset.load_depth(me, day_key(size), "seq", 7, P)
    d = os.path.join(tmp, "data_3d_raw", "seq", "velodyne_points", "data")
    os.makedirs(d, exist_ok=True)
    points.tofile(os.path.join(d, f"{7:010d}.bin"))
    # K @ T[:3] must BE P, bit for bit: K a power-of-two diagonal, T's rows scaled the other way
    K = np.diag([2.0, 0.5, 1.0]).astype(P.dtype)
    T = np.vstack([P / np.diag(K)[:, None], [[0, 0, 0, 1]]]).astype(P.dtype)
    assert np.array_equal(K @ T[:3, :], P) and (K @ T[:3, :]).dtype == P.dtype
    me = types.SimpleNamespace(data_path=tmp, target_image_size=tuple(size), _calibs={"T_velo_to_cam": {"00": T}, "K_perspective": K})
    return k360.Kitti360Dataset.load_depth(me, "seq", 7, False)


def half_row(size):
    """the row of the constructed pixels: inside the Eigen crop where the size has one"""
    return {1: 0, 2: 1, 5: 2, 24: 10}[size[0]]


def make_P(size, convention, dtype, rng):
    """a generic P (velodyne x forward, y left, z up -> camera x right, y down, z forward, a small yaw and pitch, a pinhole) whose fourth
    column is the origin point's u: a half over a power of two"""
    H, W = size
    a, b = np.radians(1.7), np.radians(-0.9)
    base = np.array([[0., -1, 0], [0, 0, -1], [1, 0, 0]])
    yaw = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    pitch = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = yaw @ pitch @ base
    if convention == "kitti_raw":
        Kc = np.array([[0.93 * W, 0, 0.5 * W + 0.53], [0, 0.97 * W, 0.5 * H + 0.47], [0, 0, 1]])
        hx, hy = 2.5, half_row(size) + 1.0                       # px = 2.5 -> x = 1 (half away: 2); py -> y = half_row
    else:
        Kc = np.array([[1.13, 0, 0.021], [0, 1.13 * W / H, -0.017], [0, 0, 1]])
        # W = 2: (px * .5 + .5) * 2 = .5 -> x = 0 (half away: 1).  The larger sizes carry the half in y, (py * .5 + .5) * H = row + .5
        # with a dyadic factor: H = 5: .5 * 5 = 2.5 -> y = 2 (half away: 3); H = 24: .4375 * 24 = 10.5 -> y = 10 (half away: 11)
        hx = 1.0 / W - 1.0 if W == 2 else 2 * 1.25 / W - 1
        hy = {1: 0.0, 2: -0.75, 5: 0.0, 24: -0.125}[H]
    A = Kc @ R
    A = A * (1 + 1e-3 * rng.standard_normal((3, 3)))             # nothing special about it
    P = np.concatenate([A, [[hx * T_Z], [hy * T_Z], [T_Z]]], axis=1)
    if dtype == np.float32:
        return P.astype(np.float32)
    assert not np.array_equal(P[:, :3].astype(np.float32).astype(np.float64), P[:, :3])
    return P


def coords_to_norm(c, n, convention):
    """the px (py) that gives the continuous pixel coordinate c: kitti_raw x = px - 1; kitti_360 x = (px * .5 + .5) * n"""
    return c + 1.0 if convention == "kitti_raw" else 2.0 * c / n - 1.0


def solve_point(P, size, convention, cx, cy, z):
    H, W = size
    px, py = coords_to_norm(cx, W, convention), coords_to_norm(cy, H, convention)
    P64 = P.astype(np.float64)
    p = np.linalg.solve(P64[:, :3], np.array([px * z, py * z, z]) - P64[:, 3])
    return np.array([p[0], p[1], p[2], 1.0])


def build_cloud(P, size, convention, rng):
    """the constructed cloud: rows of (x, y, z, 1) float32 in index order, the tag of every point"""
    H, W = size
    yt = half_row(size)
    pts, tags = [], []

    def add(x, y, z, tag):
        dx, dy = rng.uniform(-0.4, 0.4, 2)
        pts.append(solve_point(P, size, convention, x + dx, y + dy, z)), tags.append(tag)

    reserved = set()
    for y in range(min(H - 1, 6)):                               # the pair slots
        R, L = (W - 1, y), (0, y + 1)
        reserved.update((R, L))
        if y % 2 == 0:
            add(*R, 9.0 + y, "A"), add(*L, 5.0 + y, "A"), add(*L, 6.0 + y, "A")
        else:
            add(*L, 8.0 + y, "B"), add(*R, 4.0 + y, "B"), add(*R, 11.0 + y, "B")
    small = H <= 2
    if convention == "kitti_raw":
        half_px = (1, yt)
    else:
        half_px = (0, 0) if W == 2 else (1, yt)
    if small:
        multi = next(p for p in ((0, 0), (W - 1, H - 1)) if p != half_px)
    else:
        multi = (3, yt)
    reserved.update((half_px, multi, (half_px[0] + 1, half_px[1])))
    pts.append(np.array([0.0, 0.0, 0.0, 1.0])), tags.append("half")          # the origin: u = P[:, 3] exactly
    add(*multi, 6.0, "multi"), add(*multi, 4.0, "multi")
    if small:
        add(*multi, 0.2, "front")                                # x < 0, z > 0: the three-point pixel's nearest under kitti_360
    add(*multi, 9.0, "multi")
    if not small:
        neg, front = (2, yt + 1), (3, yt + 1)
        reserved.update((neg, front))
        add(*neg, -3.0, "neg"), add(*front, 0.2, "front")
        reserved.update(((2, 0), (2, H - 1), (0, 0), (W - 1, H - 1)))
        add(2, 0, 13.0, "edge"), add(2, H - 1, 14.0, "edge"), add(0, 0, 15.0, "edge"), add(W - 1, H - 1, 16.0, "edge")
    for x, y in ((0, -1), (0, H), (-1, yt), (W, yt)):
        add(x, y, 17.0, "outside")
    if not small:                                                # the fill: free pixels, some of them several times, some points outside
        free = [(x, y) for y in range(H) for x in range(1, W - 1) if (x, y) not in reserved]
        for _ in range((3 * len(free)) // 4):
            x, y = free[rng.integers(len(free))]
            add(x, y, float(rng.uniform(2.0, 70.0) if rng.random() > 0.1 else rng.uniform(79.0, 90.0)), "fill")
        for _ in range(max(4, len(free) // 8)):
            x, y = rng.integers(-2, W + 2), rng.integers(-2, H + 2)
            if not (0 <= x < W and 0 <= y < H):
                add(int(x), int(y), float(rng.uniform(2.0, 70.0)), "fill")
    return np.stack(pts).astype(np.float32), np.array(tags)


def exact_z(P, p):
    return sum((Fraction(float(P[2, k])) * Fraction(float(p[k])) for k in range(3)), Fraction(float(P[2, 3])))


def check_cloud(points, tags, P, size, convention):
    """fp64 on the stored fp32 points: the coordinates' margins, the separation of competing depths; drops the fill points that miss them"""
    H, W = size
    P64 = P.astype(np.float64)
    keep = np.ones(len(points), dtype=bool)
    while True:
        pts = points[keep]
        u = (P64 @ pts.astype(np.float64).T).T
        px, py = u[:, 0] / u[:, 2], u[:, 1] / u[:, 2]
        if convention == "kitti_raw":
            cx, cy = px - 1, py - 1
        else:
            cx, cy = (px * .5 + .5) * W, (py * .5 + .5) * H
        near = np.minimum(np.abs(cx - np.floor(cx) - 0.5), np.abs(cy - np.floor(cy) - 0.5)) < 5 * COORD_MARGIN
        t = tags[keep]
        bad = near & (t != "half")
        assert not (bad & (t != "fill")).any(), (size, convention, t[bad])
        # competing depths: per key group of the surviving points
        idx, x, y, z = LD.project(pts, P64, size, convention)
        key = y * (W - 1) + x - 1
        order = np.lexsort((z, key))
        k_s, z_s = key[order], z[order]
        close = (k_s[1:] == k_s[:-1]) & (np.abs(z_s[1:] - z_s[:-1]) < 5 * Z_REL * np.abs(z_s[1:]))
        late = np.zeros(len(pts), dtype=bool)
        late[idx[order[1:][close]]] = True
        assert not (late & (t != "fill")).any(), (size, convention)
        bad |= late
        if not bad.any():
            return keep
        keep[np.flatnonzero(keep)[bad]] = False


def expect(size, convention):
    """what a cloud of this size must hold (counted on the reference's side of things in count_features)"""
    H, W = size
    e = {"outside_rows_cols": True, "multi": True, "front": True}
    e["pair_first_right"] = e["receiver_single"] = H >= 2
    e["pair_first_left"] = H >= 3
    e["neg_lone"] = H >= 3 and convention == "kitti_360"
    e["half"] = True
    return e


def count_features(points, tags, P, size, convention):
    H, W = size
    P64 = P.astype(np.float64)
    c = dict.fromkeys(("pair_first_right", "pair_first_left", "receiver_single", "multi", "neg_lone", "front", "half", "outside_rows_cols"), 0)
    idx, x, y, z = LD.project(points, P64, size, convention, mutant="no_front")       # where every point WOULD land
    q = y * W + x
    per = {p: np.flatnonzero(q == p) for p in np.unique(q)}
    keep_front = points[idx, 0] >= 0 if convention == "kitti_raw" else np.ones(len(idx), dtype=bool)
    for yy in range(H - 1):
        r, l = per.get(yy * W + W - 1, np.array([], int)), per.get((yy + 1) * W, np.array([], int))
        r, l = r[keep_front[r]], l[keep_front[l]]
        if len(r) and len(l):
            right_first = r.min() < l.min()
            c["pair_first_right" if right_first else "pair_first_left"] += 1
            c["receiver_single"] += len(r if right_first else l) == 1
    for p, m in per.items():
        alive = m[keep_front[m]]
        c["multi"] += len(alive) >= 3 and z[alive[-1]] > z[alive].min()
        c["neg_lone"] += len(alive) == 1 and z[alive[0]] < 0
    fr = (points[idx, 0] < 0) & (z > 0)
    c["front"] = int(fr.sum())
    u = (P64 @ np.concatenate([points[:, :3], np.ones((len(points), 1), np.float32)], axis=1).astype(np.float64).T).T
    with np.errstate(all="ignore"):
        cx = u[:, 0] / u[:, 2] - 1 if convention == "kitti_raw" else (u[:, 0] / u[:, 2] * .5 + .5) * W
        cy = u[:, 1] / u[:, 2] - 1 if convention == "kitti_raw" else (u[:, 1] / u[:, 2] * .5 + .5) * H
    c["half"] = int(((cx - np.floor(cx) == 0.5) | (cy - np.floor(cy) == 0.5)).sum())
    raw = convention == "kitti_raw"
    rx, ry = (np.round(cx + 1) - 1, np.round(cy + 1) - 1) if raw else (np.round(cx), np.round(cy))      # (as rule 3 rounds)
    c["outside_rows_cols"] = int(all((ry == v).any() for v in (-1, 0, H - 1, H)) and all((rx == v).any() for v in (-1, 0, W - 1, W)))
    return c


def shows(mutant, size, convention, eigen):
    """where a mutant CAN differ from the reference.  The pair mutants need a pair (H >= 2) whose pixels survive the crop: at (24, 40)
    the crop removes columns 0 and 39, at (5, 7) it keeps column 0 in rows 2 and 3 (the L pixels of slots 1 and 2).  half_away shows in
    every case: each holds the exact half, inside the crop where there is one.  no_clamp needs a lone negative z, which kitti_raw's front filter never
    lets through.  The two front-filter mutants each change the convention that has (has not) the filter."""
    H, W = size
    if mutant in ("zbuffer", "first_write", "no_partner", "partner_min"):
        return H >= 2 and not (eigen and size == (24, 40))
    if mutant == "half_away":
        return True
    if mutant == "no_clamp":
        return convention == "kitti_360" and H >= 3
    if mutant == "no_front":
        return convention == "kitti_raw"
    return convention == "kitti_360"                             # always_front


def generate():
    mods = load_datasets()
    out, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for si, size in enumerate(SIZES):
            for convention in LD.CONVENTIONS:
                for dtype in (np.float32, np.float64):
                    rng = np.random.default_rng(1000 * si + 10 * LD.CONVENTIONS.index(convention) + (dtype == np.float64))
                    P = make_P(size, convention, dtype, rng)
                    points, tags = build_cloud(P, size, convention, rng)
                    keep = check_cloud(points, tags, P, size, convention)
                    points, tags = np.ascontiguousarray(points[keep]), tags[keep]
                    counts = count_features(points, tags, P, size, convention)
                    for k, need in expect(size, convention).items():
                        assert bool(counts[k]) >= need, (size, convention, k, counts)
                    for eigen in (False, True):
                        if eigen and (convention != "kitti_raw" or size not in EIGEN_SIZES):
                            continue
                        name = f"{convention}_{size[0]}x{size[1]}_{'f32' if dtype == np.float32 else 'f64'}{'_eigen' if eigen else ''}"
                        ref = reference_map(mods, tmp, points.copy(), P, size, convention, eigen)
                        assert ref.shape == (1,) + tuple(size) and ref.dtype == np.float64
                        mine, src = LD.load_depth(points, P, size, convention, eigen, want_src=True)
                        assert mine.dtype == P.dtype and np.array_equal(mine.astype(np.float64), ref), name
                        assert np.array_equal(LD.literal(points, P, size, convention, eigen).astype(np.float64), ref), name
                        for mutant in LD.MUTANTS:
                            differs = not np.array_equal(LD.load_depth(points, P, size, convention, eigen, mutant=mutant).astype(np.float64), ref)
                            assert differs == shows(mutant, size, convention, eigen), (name, mutant, differs)
                        hi, lo = np.zeros(size), np.zeros(size)
                        for yy, xx in zip(*np.nonzero(src >= 0)):
                            zf = exact_z(P, points[src[yy, xx]])
                            hi[yy, xx] = float(zf)
                            lo[yy, xx] = float(zf - Fraction(hi[yy, xx]))
                        occ = ref[0] != 0
                        rel = np.abs((ref[0][occ] - hi[occ]) - lo[occ]) / np.abs(hi[occ])
                        names.append(name)
                        out.update({f"{name}_points": points, f"{name}_P": P, f"{name}_depth": ref, f"{name}_src": src.astype(np.int32),
                                    f"{name}_z_hi": hi, f"{name}_z_lo": lo})
                        print(f"{name}: N={len(points)} occupied={int(occ.sum())} features={counts} "
                              f"reference-vs-exact rel max {rel.max() if rel.size else 0:.3e}")
    out["names"] = np.array(names)
    return out


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
