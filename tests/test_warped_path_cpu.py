"""NeRFAll.render_warped_path (models/lushnerf.py:898-947), the parts that need no GPU: the method's signature and refusals, the
second contract header include/lush_subframe.h and its binding, the host-side refusals of lush_warp_image_fwd, and the CPU oracle
against the reference's fixture (tests/golden/warped_path.npz, made by tests/golden/make_golden_warped.py)."""
import argparse
import ctypes
import inspect
import os

import pytest
import torch

from lush_nerf_amd import abi, lib
from oracle import lush_oracle as O
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5      # tests/test_oracle_golden.py: the oracle and the reference are both fp32 torch-CPU
ENTRY = "lush_warp_image_fwd"


def fixture_case():
    """(fixture, H, W, seed, rmnear, chunk, Ns, Ni, rbk_scale, focal, K)."""
    g = util.golden("warped_path")
    H, W, seed, rmnear, chunk, Ns, Ni = (int(x) for x in g["meta"][:7])
    focal = float(g["focal"])
    return g, H, W, seed, rmnear, chunk, Ns, Ni, float(g["meta"][7]), focal, [[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]


def _model(blur=True):
    from lush_nerf_amd import model as M
    args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                              N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                              rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=80)
    return M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4) if blur else None)


def test_render_warped_path_keeps_the_reference_signature():
    g = util.golden("warped_path")
    from lush_nerf_amd import model as M
    ref = [str(x) for x in g["sig.render_warped_path"]]
    assert ref == ["H", "W", "K", "chunk", "render_poses", "images_idx", "render_kwargs", "render_factor"]
    assert list(inspect.signature(M.NeRFAll.render_warped_path).parameters) == ["self"] + ref
    assert inspect.signature(M.NeRFAll.render_warped_path).parameters["render_factor"].default == 0
    assert "not enough values to unpack" in str(g["unwrapped_error"])      # the reference's own body, as it stands, raises
    assert len(_model().state_dict()) == 108                                 # no parameter or persistent buffer came with it


def test_second_header_is_bound_beside_the_first():
    text = open(os.path.join(ROOT, "include", "lush_subframe.h")).read()
    a = abi.parse(text, "lush_subframe.h")
    assert list(a.protos) == [ENTRY] and not a.structs and not a.consts
    args, res = a.protos[ENTRY]
    kinds = {"i": ctypes.c_int, "f": ctypes.c_float, "p": ctypes.c_void_p}
    assert res is ctypes.c_int and args == [kinds[k] for k in "p i i f f f f p i i p i f f f f p p p".split()]
    assert lib.EXPORTS_SUBFRAME == [ENTRY] and ENTRY not in lib.EXPORTS and ENTRY not in lib._SIGS
    # the first contract is what it was
    m = abi.parse(open(os.path.join(ROOT, "include", "lush_march.h")).read())
    assert (len(m.protos), len(m.structs), len(m.consts)) == (67, 9, 29) and list(m.protos) == lib.EXPORTS
    assert ENTRY + "(" not in open(os.path.join(ROOT, "include", "lush_march.h")).read().replace(" ", "")
    assert lib.HEADERS[-1].endswith("lush_march.h") and any(h.endswith("lush_subframe.h") for h in lib.HEADERS)      # needs_build() watches both
    with pytest.raises(ValueError, match=r"^lush_subframe\.h: unknown type"):      # the reader names the file it is reading
        abi.parse("int lush_x(wchar_t a);", "lush_subframe.h")
    lib.build()
    assert hasattr(ctypes.CDLL(lib.SO_PATH), ENTRY)      # the same liblush_march.so
    l = lib.load()
    assert list(getattr(l, ENTRY).argtypes) == args and getattr(l, ENTRY).restype is ctypes.c_int
    assert l.lush_abi_version() == lib.ABI_VERSION == 10


def test_warp_image_entry_refuses_on_the_host():
    lib.build()
    l = lib.load()
    one = ctypes.c_void_p(8)        # any non-null pointer: the refusals come before it is looked at

    def call(H=8, W=12, M=4, c2w=one, idx=one, num_img=30, acts=one, batch=one, centre=one):
        rc = l.lush_warp_image_fwd(c2w, H, W, 10.5, 10.5, 6., 4., idx, num_img, M, acts, 1, -1.75, -2.6, 0., 1., batch, centre, None)
        return rc, l.lush_last_error()

    for kw, msg in ((dict(H=0), b"empty image"), (dict(W=0), b"empty image"), (dict(H=-3), b"empty image"),
                    (dict(M=0), b"num_motion"), (dict(M=5), b"num_motion"),
                    (dict(H=1 << 15, W=1 << 15), b"2^31"), (dict(H=1 << 15, W=1 << 14, M=3), b"2^31"),
                    (dict(batch=None), b"required"), (dict(c2w=None), b"required"), (dict(idx=None), b"required"),
                    (dict(acts=None), b"required"), (dict(num_img=0), b"no images")):
        rc, err = call(**kw)
        assert rc != 0 and err.startswith(b"lush_warp_image_fwd: ") and msg in err, (kw, rc, err)


def test_render_warped_path_refuses_what_it_cannot_render():
    g, H, W, seed, rmnear, chunk, Ns, Ni, scale, focal, K = fixture_case()
    poses, idx = torch.zeros(2, 3, 4), torch.tensor([3, 17])
    rk = dict(perturb=False, N_importance=Ni, N_samples=Ns, use_viewdirs=True, white_bkgd=False, raw_noise_std=0., inference=True,
              near=0., far=1.)
    with pytest.raises(ValueError, match="blur-kernel network"):
        _model(blur=False).render_warped_path(H, W, K, chunk, poses, idx, rk)
    net = _model()
    with pytest.raises(NotImplementedError, match="use_viewdirs"):
        net.render_warped_path(H, W, K, chunk, poses, idx, dict(rk, use_viewdirs=False))
    with pytest.raises(NotImplementedError, match="c2w_staticcam"):
        net.render_warped_path(H, W, K, chunk, poses, idx, dict(rk, c2w_staticcam=poses[0]))
    with pytest.raises(ValueError, match="2 poses but 1 image"):
        net.render_warped_path(H, W, K, chunk, poses, idx[:1], rk)
    with pytest.raises(RuntimeError, match="no CPU path"):      # past the refusals: the kernels take device tensors only
        net.render_warped_path(H, W, K, chunk, poses, idx, rk)
    assert net.hooks.draw_offset == 0      # a refused call draws nothing


def _oracle_pose(p, H, W, K, focal, c2w, idx, Ns, Ni, rmnear, chunk, subframe_major):
    """One pose of render_warped_path from the oracle's pieces (:917-933) -> (rgb [5,H,W,3], depth [5,H,W,1], centre rays [5,3,2])."""
    ro, rd = O.get_rays(H, W, K, c2w)
    rays = torch.stack([ro, rd], -1).reshape(-1, 3, 2)
    warped, _ = O.rbk_forward(p, rays, idx.expand(H * W))
    M1 = warped.shape[0] // (H * W)
    centre = warped.reshape(H, W, M1, 3, 2)[int(H / 2), int(W / 2)]
    batch = O.pack_rays(H, W, focal, warped)
    if subframe_major:      # the rows the GPU kernel writes: m*H*W + n instead of n*(M+1) + m
        batch = batch.reshape(H * W, M1, 11).permute(1, 0, 2).reshape(-1, 11)
    outs = [O.render_rays(p, batch[i:i + chunk], Ns, perturb=0., N_importance=Ni, raw_noise_std=0., with_noise_branch=False,
                          training=False, render_rmnearplane=rmnear) for i in range(0, batch.shape[0], chunk)]
    rgb, depth = (torch.cat([o[k] for o in outs], 0) for k in ("rgb_map", "depth_map"))
    if subframe_major:      # plain views, as NeRFAll.render_warped_path takes them
        return rgb.view(M1, H, W, 3), depth.view(M1, H, W, 1), centre
    return rgb.reshape(H, W, M1, 3).permute(2, 0, 1, 3), depth.reshape(H, W, M1, 1).permute(2, 0, 1, 3), centre


@pytest.mark.mkl_reproducible
@pytest.mark.parametrize("order", ["ray_major", "subframe_major"])
def test_oracle_reproduces_the_reference_sub_frames(order):
    """The oracle's get_rays -> rbk_forward -> pack_rays -> render_rays in the reference's row order, and with the ray batch re-ordered
    to sub-frame-major rows (what lush_warp_image_fwd writes): a ray's result does not depend on its row."""
    g, H, W, seed, rmnear, chunk, Ns, Ni, scale, focal, K = fixture_case()
    p = util.params(seed, sharp=True, rbk_scale=scale)
    poses = torch.from_numpy(util.synth.poses(len(g["images_idx"]), seed))
    with torch.no_grad():
        res = [_oracle_pose(p, H, W, K, focal, poses[v], torch.tensor(int(i)), Ns, Ni, rmnear, chunk, order == "subframe_major")
               for v, i in enumerate(g["images_idx"])]
    errs = {k: util.relerr(torch.stack([r[j] for r in res], 0), g[k]) for j, k in enumerate(("rgbs", "depths", "rays_save"))}
    print(order, errs)
    assert all(e < TOL for e in errs.values()), errs
    # what the fixture can tell apart: every sub-frame differs from every other by far more than any gate of these tests
    rg = torch.from_numpy(g["rgbs"])
    assert min(float((rg[:, a] - rg[:, b]).abs().amax(dim=(1, 2, 3)).min()) for a in range(5) for b in range(a)) > 10 * 1e-4 * float(rg.abs().max())
