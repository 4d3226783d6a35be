#!/usr/bin/env python3
"""Generate tests/golden/field_query.npz from the REAL reference (build container only): NeRFAll.mlpforward,
mlpforward_noise and raw2outputs (models/lushnerf.py:234-352) called as public methods on free points / free z.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_field.py

The reference is imported read-only through make_golden.py (bytecode writing off).  Inputs are regenerated from
(seed, shape) by tests/field_inputs.py; only the reference's outputs and gradients are written, parameter gradients of
more than 4096 elements as 8 fixed projections + the L2 norm (make_golden.pack_grads).
"""
import inspect
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ServeDraws, build_ref, pack_grads, ROOT  # noqa: E402  (puts ROOT on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import field_inputs as FI  # noqa: E402

assert ROOT in sys.path


def t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(grad)


def net_grads(net, prefix):
    return {k: p.grad for k, p in net.named_parameters() if k.startswith(prefix + ".") and p.grad is not None}


def main():
    out = {"meta": np.array([FI.SEED, FI.R, FI.S, FI.S_NOISE, FI.RMNEAR])}
    for which in FI.WEIGHT_SETS:
        net = build_ref(64, FI.weights(which), rmnear=FI.RMNEAR)
        net.train()
        if "sig.mlpforward" not in out:
            for name in ("mlpforward", "mlpforward_noise", "raw2outputs"):
                out["sig." + name] = np.array([p for p in inspect.signature(getattr(net, name)).parameters])
        for mlp in ("mlp_coarse", "mlp_fine"):
            with torch.no_grad():
                out[f"{which}.raw.{mlp}"] = net.mlpforward(t(FI.points()), t(FI.dirs()), getattr(net, mlp), False, False).numpy()
        with torch.no_grad():
            out[f"{which}.noise"] = net.mlpforward_noise(t(FI.points_noise()), t(FI.dirs()), net.mlp_noise_coarse, False, False).numpy()
        # gradients under one recorded upstream gradient: the coarse net at the free points ...
        pts, dirs = t(FI.points(), True), t(FI.dirs(), True)
        net.zero_grad()
        net.mlpforward(pts, dirs, net.mlp_coarse, False, False).backward(t(FI.g_raw()))
        out[f"{which}.coarse.d_pts"], out[f"{which}.coarse.d_dirs"] = pts.grad.numpy(), dirs.grad.numpy()
        out.update({f"{which}.coarse.{k}": v for k, v in pack_grads(net_grads(net, "mlp_coarse")).items()})
        # ... and the noise net at sample 16
        pts, dirs = t(FI.points_noise(), True), t(FI.dirs(), True)
        net.zero_grad()
        net.mlpforward_noise(pts, dirs, net.mlp_noise_coarse, False, False).backward(t(FI.g_noise()))
        out[f"{which}.noisenet.d_pts"], out[f"{which}.noisenet.d_dirs"] = pts.grad.numpy(), dirs.grad.numpy()
        out.update({f"{which}.noisenet.{k}": v for k, v in pack_grads(net_grads(net, "mlp_noise_coarse")).items()})

    # raw2outputs (weights play no part)
    net = build_ref(64, FI.weights("default"), rmnear=FI.RMNEAR)
    raw_np, z_np, noise_np = FI.r2o_inputs()
    up = FI.r2o_upstream()
    names = ("rgb_map", "density", "acc_map", "weights", "depth_map")
    for case, training, std, white in FI.R2O_CASES:
        net.train(training)
        raw, z, d = t(raw_np, True), t(z_np, True), t(FI.dirs(), True)
        with ServeDraws([noise_np] if std > 0 else []):
            res = net.raw2outputs(raw, z, d, raw_noise_std=std, white_bkgd=white)
        torch.autograd.backward(list(res), [t(up[k]) for k in names])
        for k, v in zip(names, res):
            out[f"r2o.{case}.{k}"] = v.detach().numpy()
        out[f"r2o.{case}.d_raw"], out[f"r2o.{case}.d_z"], out[f"r2o.{case}.d_rays_d"] = raw.grad.numpy(), z.grad.numpy(), d.grad.numpy()
    path = os.path.join(HERE, "field_query.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
