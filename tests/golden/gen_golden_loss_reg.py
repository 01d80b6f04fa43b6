"""Generates tests/golden/loss_reg.npz FROM THE REAL REFERENCE: seeded tensors in the layout the ray samplers' reconstruct() returns,
fed straight to the reference's ReconstructionLoss (models/bts/model/loss.py) with its regularisers on -- alpha_reg (ray | slice),
surfaceness, ray entropy, depth_reg + depth_smoothness -- on four layouts and nine configurations (tests/_loss_reg_oracle.py: LAYOUTS,
CONFIGS).  Stores, per layout, the inputs in a compact EXACT form (_loss_reg_oracle.load_inputs) and, per layout and configuration, the
loss, the loss dict and d loss / d alphas, d loss / d depth of every scale.

The inputs carry, by construction: alphas that are exactly 0 and exactly 1 (hard_alpha_cap's last sample; sign(0) = 0 of both absolute
values); in layout p8 a block of kept rays whose A equals cap exactly (K = 8, fraction 1 / 8, values from {0, .25, .5}: the sum is exact
in any order; the tie takes the full gradient) and a slice row whose sum one ray carries over the cap; in layout odd one sample with more
than half of its rays invalid.  Layout odd draws its rays from 32 distinct alpha rows (the fixture stays small: equal rows have equal
gradient rows).  The script ASSERTS, on the reference alone:
  - outside the tie block (whose two rows tie as slice rows too) no KEPT ray's A - cap (ray) and no row's sum (slice; rows with a kept
    ray) lies within 1e-3 of 0 (an invalid ray and a row of invalid rays sit at exactly 0 with gradient keep = 0 on either side of the gate);
  - the gate binds on 20 - 80 % of those rays and rows;
  - the fp32 reference's terms are within 1e-6 relative of its fp64 evaluation and its gradients within 1e-5 of the largest entry;
  - no (ray, view) is within 1e-4 of a comparison of the weight rules or the diverse rule;
  - the restatement in tests/_loss_reg_oracle.py reproduces the reference;
  - each of its mutants moves the loss, a logged term or a gradient beyond the GPU tests' bars on at least one configuration
    (cap_unmasked: on alpha_slice).

    python -B tests/golden/gen_golden_loss_reg.py      (build container only)"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle.ref_shim import load_reference
from tests import _loss_pixel_oracle as PO
from tests import _loss_reg_oracle as RO

torch.set_num_threads(4)

BAR_LOSS, BAR_TERM, BAR_GRAD = 1e-5, 1e-5, 1e-4        # the GPU tests' bars
MUST_MOVE = {"cap_unmasked": "alpha_slice"}


def compact_inputs(name, n, pc, h, w, K, nv, S, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g)
    ru = lambda *shape: torch.rand(shape, generator=g)
    cap = K / 8
    # alphas as k / 256: per patch row a level, per ray a factor, so that A = sum_{k < K-1} a_k straddles cap for rays and for rows
    row_level = 0.6 + 0.9 * ru(S, n, pc, h, 1, 1)
    ray_factor = 0.4 + 1.2 * ru(S, n, pc, h, w, 1)
    a = (2 * ru(S, n, pc, h, w, K) * row_level * ray_factor * cap / (K - 1) * 256).round().clamp(0, 255).to(torch.int64)
    a[ru(S, n, pc, h, w, K) < 0.1] = 0                          # exact zeros
    a[..., K - 1] = torch.where(ru(S, n, pc, h, w) < 0.5, 256, a[..., K - 1])     # hard_alpha_cap: the last sample is exactly 1
    if name == "odd":       # 32 distinct rows, ordered by their sum; a patch row draws from a window of 16 of them
        pal = a.reshape(-1, K)[torch.randperm(a.numel() // K, generator=g)[:32]]
        pal = pal[pal.sum(-1).argsort()]
        a = pal[(ru(S, n, pc, h, 1) * 17).long().clamp(max=16) + ri(0, 16, S, n, pc, h, w)]
    if name == "p8":
        s, p, rows = RO.TIE_BLOCK
        base = torch.tensor([64, 64, 128, 0, 0, 0, 0])          # .25 + .25 + .5 = cap = 1
        for y in range(rows.start, rows.stop):
            for x in range(w):
                a[0, s, p, y, x, :7] = base[torch.randperm(7, generator=g)]
        a[0, s, p, rows, :, 7] = 256
        s, p, y = RO.CARRIED_ROW
        a[0, s, p, y, :, :7] = ri(28, 36, w, 7)                 # A ~ .875: every ray a little under the cap ...
        a[0, s, p, y, 3, :7] = ri(200, 256, 7)                  # ... and one far above
    # no other ray or row within 1e-3 of its gate (A, cap are multiples of 1 / 256: only exact ties are that close)
    tie = torch.zeros(S, n, pc, h, w, dtype=torch.bool)
    if name == "p8":
        tie[0, RO.TIE_BLOCK[0], RO.TIE_BLOCK[1], RO.TIE_BLOCK[2]] = True
    A = a[..., :-1].sum(-1)
    bump = (A == round(cap * 256)) & ~tie
    a[..., 0] = torch.where(bump, (a[..., 0] + 2).clamp(max=255), a[..., 0])
    depth = 8192 + ri(0, 2048, S, n, pc, h, w)                  # k / 4096: 2 .. 2.5
    gt = ri(16, 200, n, pc, h, w, 3)
    rgb = (gt.view(1, n, pc, h, w, 1, 3) + ri(-40, 41, S, n, pc, h, w, nv, 3)).clamp(0, 255)
    wts = ri(1, 256, n, pc, h, w, K)
    if name == "odd":
        wts = wts.reshape(-1, K)[:32][ri(0, 32, n, pc, h, w)]
    inv = torch.zeros(n, pc, h, w, K, nv, dtype=torch.uint8)
    inv[:, :, 0] = 1                                            # row 0: every sample of every view
    if h > 2:
        inv[:, :, 2, :3, : K // 2, 0] = 1                       # part of view 0's mass
        inv[:, :, 2, w - 3:, 0, :] = 1                          # one sample of every view: strict calls it invalid, the weights do not
    if h > 3:
        inv[:, :, 3, 1:4] = 1                                   # three rays of a row: invalid under every policy (the masked cap of a slice row)
    if name == "odd":
        inv[n - 1, :, (2 * h) // 5:] = 1                        # more than half of the last sample's rays
    code = ri(0, 200, n, pc, h, w)
    code[ru(n, pc, h, w) < 0.15] = 200 + ri(0, 56, 1).item()    # rays without diversity
    if h > 2:
        code[:, :, h - 1, : w // 2] = 203
    if name == "p8":                                            # the constructed blocks stay kept under every policy
        code[RO.TIE_BLOCK[0], RO.TIE_BLOCK[1], RO.TIE_BLOCK[2]] = 7
        code[RO.CARRIED_ROW[0], RO.CARRIED_ROW[1], RO.CARRIED_ROW[2]] = 7
    return {f"{name}_alphas_u16": a.numpy().astype(np.uint16), f"{name}_depth_u16": depth.numpy().astype(np.uint16),
            f"{name}_rgb_u8": rgb.numpy().astype(np.uint8), f"{name}_rgb_gt_u8": gt.numpy().astype(np.uint8),
            f"{name}_weights_u8": wts.numpy().astype(np.uint8), f"{name}_invalid": inv.numpy(),
            f"{name}_samp_code": code.numpy().astype(np.uint8)}


def run_reference(ref, levels, gt, cfg, dtype=torch.float32):
    lv, leaves = RO.leaves(levels, dtype)
    loss, d = ref.ReconstructionLoss(dict(cfg))(dict(coarse=lv, fine=[dict(x) for x in lv], rgb_gt=gt.to(dtype)))
    return loss.detach(), {k: float(d[k]) for k in RO.DICT_KEYS}, RO.grads(loss, leaves)


def run_restatement(levels, gt, cfg, mutant=None, dtype=torch.float32):
    lv, leaves = RO.leaves(levels, dtype)
    loss, d, extra = RO.reconstruction_loss(lv, gt.to(dtype), cfg, mutant)
    return loss.detach(), d, RO.grads(loss, leaves), extra


def moved(want, got):
    """does result `got` differ from the stored result `want` beyond the GPU tests' bars?"""
    if abs(want[0].item() - got[0].item()) > BAR_LOSS:
        return True
    if any(abs(want[1][k] - got[1][k]) > BAR_TERM * abs(want[1][k]) for k in RO.TERM_KEYS):
        return True
    return any((x - y).abs().max().item() > BAR_GRAD * x.abs().max().item() for x, y in zip(want[2], got[2]) if x.abs().max() > 0)


def check_gates(name, levels, keep, K):
    """the margins and the binding fractions of the alpha_reg gates, over the kept rays / the rows with a kept ray, outside the tie block"""
    cap = K / 8
    for s, level in enumerate(levels):
        A = level["alphas"][..., :-1].sum(-1)
        free = keep > 0
        if name == "p8" and s == 0:
            sb, pb, rows = RO.TIE_BLOCK
            assert (A[sb, pb, rows] == cap).all() and (keep[sb, pb, rows] == 1).all(), "the tie block does not tie on kept rays"
            free = free.clone()
            free[sb, pb, rows] = False
            sc, pcar, y = RO.CARRIED_ROW
            over = (A[sc, pcar, y] > cap)
            row = ((A - cap) * keep)[sc, pcar, y]
            assert over.sum() == 1 and row.sum() > 0.5 and (keep[sc, pcar, y] == 1).all(), "the carried row is not carried by one ray"
        m = (A - cap)[free]
        assert (m.abs() > 1e-3).all(), (name, s, "a kept ray sits on the ray gate")
        rows_sum, rows_kept = ((A - cap) * keep).sum(-1), free.sum(-1) > 0          # (the tie block's rows tie as rows too)
        assert (rows_sum[rows_kept].abs() > 1e-3).all(), (name, s, "a row sits on the slice gate")
        fr, fs = (m > 0).float().mean().item(), (rows_sum[rows_kept] > 0).float().mean().item()
        print(name, "scale", s, "gate binds on", round(fr, 3), "of the kept rays,", round(fs, 3), "of the rows with a kept ray")
        assert 0.2 <= fr <= 0.8 and 0.2 <= fs <= 0.8, (name, s, fr, fs)


def main():
    ref = load_reference()
    arrays, caught = {}, {m: set() for m in RO.MUTANTS}
    for name, L in RO.LAYOUTS.items():
        comp = compact_inputs(name, seed=1900 + L["h"], **L)
        arrays.update(comp)
        levels, gt = RO.load_inputs(comp, name)
        assert levels[0]["alphas"].shape == (L["n"], L["pc"], L["h"], L["w"], L["K"]) and len(levels) == L["S"]
        a0 = levels[0]["alphas"]
        assert (a0 == 0).any() and (a0 == 1).any() and a0.max() <= 1
        wsum, std = PO.diverse_stats(levels[0])
        assert ((std - 0.01).abs() > 1e-4).all() and ((wsum - 0.9).abs() > 1e-4).all(), "a (ray, view) sits on a comparison of an invalid rule"
        for policy in ("strict", "weight_guided", "weight_guided_diverse"):
            keep = 1 - PO.invalid_rays(levels[0], policy).squeeze(-1).float()
            frac = 1 - keep.reshape(L["n"], -1).mean(-1)
            print(name, policy, "invalid fraction per sample", frac.tolist())
            assert 0 < frac.min() and (name != "odd" or (frac[-1] > 0.5 and (frac[:-1] < 0.5).all()))
            check_gates(name, levels, keep, L["K"])
        for cname in RO.CONFIGS:
            cfg = RO.config_of(cname)
            want = run_reference(ref, levels, gt, cfg)
            want64 = run_reference(ref, levels, gt, dict(cfg, criterion="l2"), torch.float64)     # (the regularisers do not read the criterion)
            for k in RO.TERM_KEYS:
                assert abs(want[1][k] - want64[1][k]) <= 1e-6 * abs(want64[1][k]), (name, cname, k, want[1][k], want64[1][k])
            for x, y in zip(want[2], want64[2]):
                assert (x.double() - y).abs().max().item() <= 1e-5 * y.abs().max().item(), (name, cname, "fp32 vs fp64 gradient")
            got = run_restatement(levels, gt, cfg)
            got64 = run_restatement(levels, gt, dict(cfg, criterion="l2"), dtype=torch.float64)
            assert abs(want[0].item() - got[0].item()) <= 1e-6, (name, cname, want[0], got[0])
            for k in RO.DICT_KEYS:
                assert abs(want[1][k] - got[1][k]) <= 1e-6 * max(1.0, abs(want[1][k])), (name, cname, k, want[1][k], got[1][k])
            for x, y in zip(want[2], got[2]):
                assert (x - y).abs().max().item() <= 1e-5 * x.abs().max().item(), (name, cname, "restatement gradient")
            assert abs(got[3]["surf"] - got64[3]["surf"]) <= 1e-6 * abs(got64[3]["surf"]) or got64[3]["surf"] == 0
            for m in RO.MUTANTS:
                if moved(want, run_restatement(levels, gt, cfg, m)[:3]):
                    caught[m].add((cname, name))
            key = f"{name}_{cname}"
            arrays.update({f"{key}_loss": want[0].reshape(1).numpy(),
                           f"{key}_loss_dict": np.array([want[1][k] for k in RO.DICT_KEYS], dtype=np.float64),
                           f"{key}_surf": np.array([got64[3]["surf"]], dtype=np.float64)})
            for s in range(L["S"]):
                arrays[f"{key}_g_alphas_{s}"], arrays[f"{key}_g_depth_{s}"] = want[2][2 * s].numpy(), want[2][2 * s + 1].numpy()
            print(name, cname, "loss", want[0].item(), {k: want[1][k] for k in RO.TERM_KEYS})
    for m in RO.MUTANTS:
        print("mutant", m, "moves", sorted(caught[m]))
        assert caught[m], f"mutant {m} is not caught by any configuration"
        if m in MUST_MOVE:
            assert MUST_MOVE[m] in {c for c, _ in caught[m]}, f"mutant {m} does not move {MUST_MOVE[m]}"
    out = os.path.join(HERE, "loss_reg.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 400_000


if __name__ == "__main__":
    main()
