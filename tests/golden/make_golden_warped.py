#!/usr/bin/env python3
"""Generate tests/golden/warped_path.npz from the REAL reference (build container only): NeRFAll.render_warped_path
(models/lushnerf.py:898-947), the sharp sub-frames of each training view and the warped rays of the centre pixel.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_warped.py

The reference is imported read-only through make_golden.py (bytecode writing off).  Its render_warped_path cannot run as
it stands: :925 unpacks the two values of Rigid_Blurring_Kernel.forward into three names.  The generator first makes that
call and records in the fixture that it raises (`unwrapped_error`); then, for the duration of ONE call of the reference's
own render_warped_path, Rigid_Blurring_Kernel.forward is wrapped to return (new_rays, ccw, None) -- a stand-in of the same
kind as the `.cuda()` identity make_golden.py uses for Render_Aligned_Pixel.  Every line of arithmetic is the reference's.

Only DATA is written: meta (H, W, seed, render_rmnearplane, chunk, N_samples, N_importance, rbk_scale), focal, images_idx,
the three outputs, that message and the method's parameter names.  Weights and poses are regenerated from the seed by
lush_nerf_amd/synth.py.  The generator refuses to write a fixture whose sub-frames are too alike for the tests' gates to
tell them apart (a missing or mis-ordered warp must not fit inside a tolerance).
"""
import contextlib
import inspect
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_ref, ROOT  # noqa: E402  (puts ROOT on sys.path; MKL's reproducible path)
import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lush_nerf_amd import synth  # noqa: E402

assert ROOT in sys.path

H, W, FOCAL, SEED, RMNEAR, CHUNK = 8, 12, 10.5, 21, 80, 128
RBK_SCALE = 2.0e4
IMAGES_IDX = [3, 17]
RGB_GATE, RAYS_GATE = 1e-4, 2e-5      # the GPU tests' gates (relative to max|.|): sub-frames differ by >= 10 x / 100 x these


def main():
    ref_model = MG.ref_model
    K = [[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]]
    net = build_ref(64, synth.all_weights(MG.NUM_IMG, SEED, sharp=True, rbk_scale=RBK_SCALE), rmnear=RMNEAR)
    net.eval()
    poses = torch.from_numpy(synth.poses(len(IMAGES_IDX), SEED))
    idx = torch.tensor(IMAGES_IDX)
    rk = dict(perturb=False, N_importance=64, N_samples=64, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.,
              inference=True, near=0., far=1.)      # render_kwargs_test (run_lushnerf.py:406-417)
    args = (H, W, K, CHUNK, poses, idx, rk)
    # 1. the reference as it stands
    err = ""
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            net.render_warped_path(*args)
    except ValueError as e:
        err = f"{type(e).__name__}: {e}"
    assert "not enough values to unpack" in err, err
    # 2. with Rigid_Blurring_Kernel.forward returning one more value
    keep = ref_model.Rigid_Blurring_Kernel.forward
    ref_model.Rigid_Blurring_Kernel.forward = lambda self, rays, rays_info: (*keep(self, rays, rays_info), None)
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            rgbs, depths, rays_save = net.render_warped_path(*args)
    finally:
        ref_model.Rigid_Blurring_Kernel.forward = keep
    rgbs, depths, rays_save = rgbs.numpy(), depths.numpy(), rays_save.numpy()
    M1 = rgbs.shape[1]
    assert rgbs.shape == (len(IMAGES_IDX), M1, H, W, 3) and depths.shape == (len(IMAGES_IDX), M1, H, W, 1) and rays_save.shape == (len(IMAGES_IDX), M1, 3, 2)
    # every pair of distinct sub-frames is further apart than any gate could hide
    need_rgb, need_rays = 10 * RGB_GATE * np.abs(rgbs).max(), 100 * RAYS_GATE * np.abs(rays_save).max()
    for v in range(len(IMAGES_IDX)):
        for a in range(M1):
            for b in range(a + 1, M1):
                d_rgb, d_rays = np.abs(rgbs[v, a] - rgbs[v, b]).max(), np.abs(rays_save[v, a] - rays_save[v, b]).max()
                print(f"pose {v} sub-frames {a},{b}: rgb {d_rgb:.2e} (need {need_rgb:.2e}), depth {np.abs(depths[v, a] - depths[v, b]).max():.2e}, "
                      f"centre rays {d_rays:.2e} (need {need_rays:.2e})")
                assert d_rgb >= need_rgb and d_rays >= need_rays, "sub-frames too alike: raise RBK_SCALE"
    # ... and the two views' kernels differ likewise (a wrong image index must not pass)
    w = np.abs((rays_save[0] - rays_save[0, :1]) - (rays_save[1] - rays_save[1, :1])).max()
    print(f"warp of view {IMAGES_IDX[0]} against view {IMAGES_IDX[1]}: centre rays {w:.2e}")
    assert w >= need_rays
    out = dict(meta=np.array([H, W, SEED, RMNEAR, CHUNK, 64, 64, RBK_SCALE]), focal=np.array(FOCAL), images_idx=np.array(IMAGES_IDX),
               rgbs=rgbs, depths=depths, rays_save=rays_save, unwrapped_error=np.array(err))
    out["sig.render_warped_path"] = np.array([p for p in inspect.signature(net.render_warped_path).parameters])
    path = os.path.join(HERE, "warped_path.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; rgb", rgbs.min(), "..", rgbs.max())
    for sub in ("", "models", "utils"):
        assert not os.path.isdir(os.path.join(MG.REF, sub, "__pycache__")), sub


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main()
