"""Golden fixtures FROM THE REAL REFERENCE for the two CPU tests that used to import it live.  Run in the build container only:

    python -B tests/golden/gen_golden_fullres.py

fullres_slice.npz   the reference's NeRFRenderer.composite at the real 192x640 resolution on every 97th ray of a seeded KITTI-Raw
                    scene (tests/test_oracle_golden.py::test_oracle_against_live_reference_fullres_slice).  Every input is rebuilt by
                    the test from the same seeds through oracle/bts_oracle.py; the file holds the reference's rgb and depth, its
                    invalid flags (all 0 / 1) as packed bits, and the depths of every 64th ray's samples (that the inputs match).
md2_decoder.npz     the reference's Monodepth2 Decoder (models/common/backbones/monodepth2.py) on weights and input maps that
                    seeded() draws from numpy's RandomState (a stream that is the same on every platform), which the test draws
                    again: its state-dict keys in order, and per output scale the SHA-256 of the `disp` tensor's bytes plus its
                    values at 1024 fixed positions (tests/test_monodepth2_cpu.py::test_decoder_matches_the_reference_decoder_bit_for_bit).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

from oracle import bts_oracle as O
from oracle.ref_shim import load_reference
from gen_golden import ref_conf, load_mlp_into

# the seeds and shapes the tests rebuild their inputs from
FULLRES = dict(seed=9, mlp_seed=5, H=192, W=640, C=64, K=64, stride=97)
MD2 = dict(seed=1, num_ch_enc=[64, 64, 128, 256, 512], num_ch_dec=[32, 32, 64, 128, 256], d_out=64, n=1, H=32, W=48)


def fullres_inputs():
    """-> (scene, mlp, rays (1, B, 8), z (B, K)) of the full-resolution slice, built as the test builds them"""
    p = FULLRES
    scene = O.synthetic_scene(1, 2, p["H"], p["W"], p["C"], seed=p["seed"], intrinsics=O.K_KITTIRAW)
    g = torch.Generator().manual_seed(p["mlp_seed"])
    mlp = O.init_mlp(p["C"] + 39, 64, 0, gen=g)
    rays = O.image_rays(scene["poses"], scene["projs"], p["H"], p["W"], 3.0, 80.0)[:, ::p["stride"]].contiguous()
    u = torch.rand(rays.shape[1], p["K"], generator=g)
    z = O.sample_coarse(rays.reshape(-1, 8), p["K"], True, u)
    return scene, mlp, rays, z


def gen_fullres(ref):
    cfg = O.FieldConfig()
    scene, mlp, rays, z = fullres_inputs()
    net = ref.make_net(ref_conf(cfg, 0, 64), [scene["feat"]])
    load_mlp_into(net, mlp)
    renderer = ref.NeRFRenderer(n_coarse=FULLRES["K"], lindisp=True, hard_alpha_cap=True).eval()
    net.eval()
    net.encode(scene["images"], scene["projs"], scene["poses"], ids_encoder=[0], ids_render=[0])
    with torch.no_grad():
        out = renderer.composite(net, rays.reshape(-1, 8), z, coarse=True, sb=1)
    inv = out[4].numpy()
    assert np.isin(inv, (0.0, 1.0)).all()
    np.savez_compressed(os.path.join(HERE, "fullres_slice.npz"), rgb=out[1].numpy(), depth=out[2].numpy(),
                        invalid_bits=np.packbits(inv.reshape(-1) != 0), invalid_shape=np.array(inv.shape), z_every64=z[::64].numpy())


def seeded(rs, shape, fan_in=0):
    """float32 N(0, 1 / fan_in) (weights) or N(0, 0.01) (fan_in 0: biases) from a numpy RandomState; the test draws the same"""
    a = rs.standard_normal(shape)
    return torch.from_numpy((a / fan_in ** 0.5 if fan_in else a * 0.1).astype(np.float32))


def disp_record(t, s):
    """per output scale: the SHA-256 of the tensor's bytes and its values at 1024 fixed positions"""
    import hashlib
    a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
    idx = np.random.RandomState(s).randint(0, a.size, 1024)
    return {f"sha{s}": np.array(hashlib.sha256(a.tobytes()).hexdigest()), f"idx{s}": idx, f"val{s}": a.reshape(-1)[idx]}


def gen_md2_decoder():
    from models.common.backbones.monodepth2 import Decoder as RefDecoder
    p = MD2
    torch.manual_seed(p["seed"])
    ref = RefDecoder(num_ch_enc=np.array(p["num_ch_enc"]), d_out=p["d_out"], num_ch_dec=p["num_ch_dec"], scales=range(4))
    sd = ref.state_dict()
    assert all(v.is_floating_point() for v in sd.values())
    rs = np.random.RandomState(p["seed"])
    ref.load_state_dict({k: seeded(rs, tuple(v.shape), int(np.prod(v.shape[1:])) if v.dim() > 1 else 0) for k, v in sd.items()})
    feats = [seeded(rs, (p["n"], c, p["H"] >> i, p["W"] >> i), 1) for i, c in enumerate(p["num_ch_enc"])]
    with torch.no_grad():
        out = ref([f.clone() for f in feats])
    arrays = {}
    for s in range(4):
        arrays.update(disp_record(out[("disp", s)], s))
    np.savez_compressed(os.path.join(HERE, "md2_decoder.npz"), keys=np.array(list(sd.keys())), **arrays)


def main():
    torch.set_num_threads(4)
    ref = load_reference()
    gen_fullres(ref)
    gen_md2_decoder()
    for f in ("fullres_slice.npz", "md2_decoder.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
