"""NeRFAll.mlpforward / mlpforward_noise / raw2outputs as public methods (models/lushnerf.py:234-352), the parts that need no
GPU: the oracle against the reference's fixture (tests/golden/field_query.npz, made by tests/golden/make_golden_field.py), the
methods' signatures and refusals, and the new C entry points' declarations and host-side refusals."""
import argparse
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from lush_nerf_amd import lib
from oracle import lush_oracle as O
from tests import field_inputs as FI
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5      # tests/test_oracle_golden.py: the oracle and the reference are both fp32 torch-CPU
R2O_NAMES = ("rgb_map", "density", "acc_map", "weights", "depth_map")


def _params(which, prefix=None):
    return {k: torch.from_numpy(v.copy()).requires_grad_(prefix is not None and k.startswith(prefix + "."))
            for k, v in FI.weights(which).items()}


def _sub(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


@pytest.mark.mkl_reproducible
@pytest.mark.parametrize("which", list(FI.WEIGHT_SETS))
def test_oracle_mlpforward_matches_the_reference_at_free_points(which):
    g = util.golden("field_query")
    pts, dirs = torch.from_numpy(FI.points()), torch.from_numpy(FI.dirs())
    assert float(dirs.norm(dim=-1).min()) < 0.7 and float(dirs.norm(dim=-1).max()) > 1.5      # not unit length
    assert float(pts.abs().max()) > 1.0                                                         # some outside the NDC cube
    p = _params(which)
    with torch.no_grad():
        for mlp in ("mlp_coarse", "mlp_fine"):
            assert util.relerr(O.mlpforward(p, mlp, pts, dirs), g[f"{which}.raw.{mlp}"]) < TOL, mlp
        assert util.relerr(O.mlpforward_noise(p, "mlp_noise_coarse", torch.from_numpy(FI.points_noise()), dirs), g[f"{which}.noise"]) < TOL
    if which == "trained":      # a density field with surfaces: raw sigma far from 0 on both sides
        s = g["trained.raw.mlp_coarse"][..., 3]
        assert s.max() > 20 and s.min() < -20
    # gradients under the recorded upstream gradient: points, directions, parameters
    p = _params(which, "mlp_coarse")
    pr, dr = pts.clone().requires_grad_(True), dirs.clone().requires_grad_(True)
    O.mlpforward(p, "mlp_coarse", pr, dr).backward(torch.from_numpy(FI.g_raw()))
    assert util.relerr(pr.grad, g[f"{which}.coarse.d_pts"]) < TOL and util.relerr(dr.grad, g[f"{which}.coarse.d_dirs"]) < TOL
    util.check_grads({k: v.grad for k, v in p.items()}, _sub(g, f"{which}.coarse."), TOL)
    p = _params(which, "mlp_noise_coarse")
    pr, dr = torch.from_numpy(FI.points_noise()).requires_grad_(True), dirs.clone().requires_grad_(True)
    O.mlpforward_noise(p, "mlp_noise_coarse", pr, dr).backward(torch.from_numpy(FI.g_noise()))
    assert util.relerr(pr.grad, g[f"{which}.noisenet.d_pts"]) < TOL and util.relerr(dr.grad, g[f"{which}.noisenet.d_dirs"]) < TOL
    assert float(pr.grad[:, :16].abs().max()) == 0 and float(pr.grad[:, 17:].abs().max()) == 0      # sample 16 only
    fx = _sub(g, f"{which}.noisenet.")
    assert not any("alpha_linear" in k for k in fx)      # dead in NeRF_Noise: the reference leaves its .grad at None
    util.check_grads({k: v.grad for k, v in p.items()}, fx, TOL)


@pytest.mark.mkl_reproducible
@pytest.mark.parametrize("case", [c[0] for c in FI.R2O_CASES])
def test_oracle_raw2outputs_matches_the_reference_on_free_z(case):
    g = util.golden("field_query")
    _, training, std, white = next(c for c in FI.R2O_CASES if c[0] == case)
    raw_np, z_np, noise_np = FI.r2o_inputs()
    up = FI.r2o_upstream()
    assert z_np.min() < FI.RMNEAR / 128 < z_np.max()
    for dt in (torch.float32, torch.float64):      # float64: the yardstick of the GPU tests, tied to the reference here
        raw, z, d = (torch.from_numpy(a).to(dt).requires_grad_(True) for a in (raw_np, z_np, FI.dirs()))
        res = O.raw2outputs(raw, z, d, std, white, torch.from_numpy(noise_np).to(dt) if std > 0 else None, training=training,
                            render_rmnearplane=FI.RMNEAR)
        torch.autograd.backward(list(res), [torch.from_numpy(up[k]).to(dt) for k in R2O_NAMES])
        for k, v in zip(R2O_NAMES, res):
            assert util.relerr(v, g[f"r2o.{case}.{k}"]) < TOL, (k, dt)
        for k, v in (("d_raw", raw), ("d_z", z), ("d_rays_d", d)):
            assert util.relerr(v.grad, g[f"r2o.{case}.{k}"]) < TOL, (k, dt)
    if not training:      # the near mask took some samples and left others
        dens = g["r2o.eval.density"]
        masked = z_np[:, 1:] <= FI.RMNEAR / 128
        assert masked.any() and (~masked).any() and float(np.abs(dens[masked]).max()) == 0 and float(dens[~masked].max()) > 1
    assert float(np.abs(g[f"r2o.{case}.d_raw"][:, -1, 3]).max()) == 0      # the last sample has alpha = 1 whatever its sigma


def _model(Ni=64):
    from lush_nerf_amd import model as M
    args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                              N_importance=Ni, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                              rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=80)
    return M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4))


def test_the_three_methods_keep_the_reference_signatures():
    g = util.golden("field_query")
    net = _model()
    for name in ("mlpforward", "mlpforward_noise", "raw2outputs"):
        ours = list(inspect.signature(getattr(net, name)).parameters)
        ref = [str(x) for x in g["sig." + name]]
        assert ours[:len(ref)] == ref, (name, ours, ref)
    assert list(inspect.signature(net.raw2outputs).parameters)[-1] == "noise"
    assert inspect.signature(net.mlpforward).parameters["netchunk"].default == 1024 * 64
    assert len(net.state_dict()) == 108      # no parameter or persistent buffer came with them


def test_the_three_methods_refuse_what_is_not_built():
    net = _model()
    pts, dirs = torch.zeros(4, 20, 3), torch.ones(4, 3)
    for fn in (net.mlpforward, net.mlpforward_noise):
        mlp = net.mlp_noise_coarse if fn == net.mlpforward_noise else net.mlp_coarse
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(pts, dirs, mlp, False, False)
        with pytest.raises(NotImplementedError, match="viewdirs"):
            fn(pts, None, mlp, False, False)
        with pytest.raises(ValueError, match="mlp must be"):
            fn(pts, dirs, _model().mlp_coarse, False, False)      # another model's network
        with pytest.raises(ValueError, match="mlp must be"):
            fn(pts, dirs, torch.nn.Linear(3, 4), False, False)
        with pytest.raises(ValueError, match="3"):
            fn(torch.zeros(4, 20, 2), dirs, mlp, False, False)
    with pytest.raises(IndexError):
        net.mlpforward_noise(torch.zeros(4, 16, 3), dirs, net.mlp_noise_coarse, False, False)
    with pytest.raises(ValueError, match="mlp must be"):
        _model(Ni=0).mlpforward(pts, dirs, None, False, False)      # (no fine network: None is no network of this model)
    raw, z = torch.zeros(4, 8, 4), torch.linspace(0, 1, 8).expand(4, 8)
    for kw in (dict(), dict(raw_noise_std=1.0), dict(raw_noise_std=1.0, noise=torch.zeros(4, 7)), dict(white_bkgd=True, pytest=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            net.raw2outputs(raw, z, dirs, **kw)
    assert net.hooks.draw_offset == 0      # a refused call draws nothing


def test_new_entry_points_are_declared_exported_and_refuse_on_the_host():
    header = open(os.path.join(ROOT, "include", "lush_march.h")).read()
    declared = set(re.findall(r"\b(lush_[a-z0-9_]+)\s*\(", header))
    lib.build()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in ("lush_points_pack", "lush_points_grad", "lush_composite_bwd_full"):
        assert name in declared and name in lib.EXPORTS and hasattr(so, name), name
    assert "lush_field.hip" in lib.SOURCES
    l = lib.load()
    assert l.lush_abi_version() == lib.ABI_VERSION == 10
    one = ctypes.c_void_p(8)        # any non-null pointer: the refusals come before it is looked at
    for S in (1, 257, 0, -3):
        rc = l.lush_composite_bwd_full(one, one, one, 4, S, None, 0., -1., 0, None, None, None, None, None, one, one, one, None)
        assert rc != 0 and b"lush_composite_bwd_full: S must be in [2,256]" in l.lush_last_error(), (S, l.lush_last_error())
    assert l.lush_composite_bwd_full(one, one, one, 0, 8, None, 0., -1., 0, None, None, None, None, None, one, one, one, None) != 0
    assert b"empty" in l.lush_last_error()
    assert l.lush_composite_bwd_full(None, one, one, 4, 8, None, 0., -1., 0, None, None, None, None, None, one, one, one, None) != 0
    assert b"required" in l.lush_last_error()
    for args in ((one, one, 0, 3, one, one), (one, one, 3, 0, one, one)):
        assert l.lush_points_pack(*args, None) != 0 and b"lush_points_pack: empty" in l.lush_last_error()
    assert l.lush_points_pack(one, None, 3, 3, one, one, None) != 0 and b"required" in l.lush_last_error()
    assert l.lush_points_pack(one, one, 1 << 20, 128, one, one, None) != 0 and b"2^27" in l.lush_last_error()
    assert l.lush_points_grad(one, 0, 3, one, one, None) != 0 and b"lush_points_grad: empty" in l.lush_last_error()
    assert l.lush_points_grad(one, 3, 3, None, one, None) != 0 and b"required" in l.lush_last_error()
    assert l.lush_points_grad(one, 1 << 20, 128, one, one, None) != 0 and b"2^27" in l.lush_last_error()
