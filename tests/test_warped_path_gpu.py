"""NeRFAll.render_warped_path on the GPU (run with -m gpu on an MI355X): warp_image_fwd_kernel bit for bit against the kernels it
fuses, the method against the reference's fixture (tests/golden/warped_path.npz), against the piecewise public path and against
render_path, and one pose at full size.  Every figure is printed before it is asserted.

Gates (normalised max error, tests/util.relerr): rgbs 1e-4 and depths 1e-3 (t_eval_forward's, the project's output bound), warped
rays 2e-5 (t_rbk's), the packed ray batch against the oracle 2e-5 (t_warp_ndc's).  Everything else is equality of bit patterns: the
fused kernel runs the device functions of the kernels it replaces in fp32 under -ffp-contract=off, and a ray's result does not
depend on the row it is marched in (tests/test_gpu_parity.py::test_full_size_properties)."""
import argparse

import pytest
import torch

from oracle import lush_oracle as O
from tests import util
from tests.test_warped_path_cpu import fixture_case

pytestmark = pytest.mark.gpu

MODES = ["2,2", "h,h"]
RK = dict(perturb=False, N_importance=64, N_samples=64, use_viewdirs=True, white_bkgd=False, raw_noise_std=0., inference=True,
          near=0., far=1.)      # render_kwargs_test (run_lushnerf.py:406-417)
_NETS = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the HIP path has no CPU fallback")
    from lush_nerf_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _net(mode):
    """The fixture's model in eval mode (render_rmnearplane 80), one per precision mode for the whole file."""
    if mode not in _NETS:
        from lush_nerf_amd import model as M, ops, synth
        g, H, W, seed, rmnear, chunk, Ns, Ni, scale, focal, K = fixture_case()
        args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                                  N_importance=Ni, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                                  rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=rmnear)
        net = M.NeRFAll(args, M.RBK(util.NUM_IMG, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4),
                        precision=ops.Precision(*ops.parse_planes(mode)))
        M.load_reference_weights(net, synth.all_weights(util.NUM_IMG, seed, sharp=True, rbk_scale=scale))
        _NETS[mode] = net.to("cuda:0").eval()
    return _NETS[mode]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _poses(dev):
    g, H, W, seed = fixture_case()[:4]
    return torch.from_numpy(util.synth.poses(len(g["images_idx"]), seed)).to(dev), torch.from_numpy(g["images_idx"]).to(dev)


def _piecewise(net, H, W, K, chunk, c2w, idx, ops):
    """:917-933 from the public pieces: ray table, mlp_rbk, render_train_scene, the permuting copies -> (rgb, depth, centre rays)."""
    rays = ops.gen_rays_image(c2w, H, W, K).reshape(-1, 3, 2)
    with torch.no_grad():
        rays_w, _ = net.mlp_rbk(rays, {"images_idx": idx.reshape(1).expand(H * W)[:, None]})
        centre = rays_w.reshape(H, W, -1, 3, 2)[int(H / 2), int(W / 2)].clone()
        rgb, depth, acc, extras = net.render_train_scene(H, W, K, chunk, rays=rays_w, c2w=c2w[:3, :4], **RK)
    M1 = rgb.shape[0] // (H * W)
    return (rgb.reshape(H, W, M1, 3).permute(2, 0, 1, 3).contiguous(), depth.reshape(H, W, M1, 1).permute(2, 0, 1, 3).contiguous(), centre)


@pytest.mark.parametrize("which_idx", ["first", "last"])
@pytest.mark.parametrize("ndc", [True, False], ids=["ndc", "no_ndc"])
@pytest.mark.parametrize("size", [(8, 12), (5, 7), (1, 1), (3, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_writes_the_bits_of_the_kernels_it_fuses(dev, size, ndc, which_idx):
    """ops.warp_image against ops.gen_rays_image -> ops.RbkWarpNdc (rows n*5+m) and ops.RbkWarp (the un-packed rays of the centre
    pixel), as bit patterns, and against the oracle's rbk_forward -> pack_rays.  Sizes: a ragged last block, one pixel, rows longer than
    a wave; both ray prologues; the first and the last view's activation row."""
    from lush_nerf_amd import ops, synth
    from tests.gpu_diag import rbk_tensors
    H, W = size
    focal, seed, M = 10.5, 21, 4
    K = [[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]
    near, far = (0., 1.) if ndc else (2., 6.)
    p = util.params(seed, rbk_scale=3.0e5)      # rotations up to ~0.5 rad, as t_warp_ndc
    tens = [t.to(dev) for t in rbk_tensors(p)]
    c2w = torch.from_numpy(synth.poses(2, seed))[1]
    i = 0 if which_idx == "first" else util.NUM_IMG - 1
    idx = torch.tensor(i, device=dev)
    batch, centre, acts = ops.warp_image(c2w.to(dev), idx, H, W, K, ndc, near, far, M, 0.1, None, *tens)
    assert batch.shape == (5 * H * W, 11) and centre.shape == (5, 3, 2) and acts.shape == (util.NUM_IMG, ops.RBK_ACT)
    # ... a precomputed activation table gives the same rows, and a 1-element int32 index is the same index
    batch2, centre2, acts2 = ops.warp_image(c2w.to(dev), idx.reshape(1).int(), H, W, K, ndc, near, far, M, 0.1, None, *tens, acts=acts)
    assert acts2 is acts and _same_bits(batch2, batch) and _same_bits(centre2, centre)
    rays = ops.gen_rays_image(c2w.to(dev), H, W, K).reshape(-1, 3, 2)
    ref, _, _ = ops.RbkWarpNdc.apply(rays, idx.expand(H * W), M, 0.1, None, None, H, W, focal, ndc, near, far, *tens)
    ref = ref.view(H * W, 5, 11).permute(1, 0, 2)
    got = batch.view(5, H * W, 11)
    n_diff = int((_bits(got) != _bits(ref)).sum())
    warped, _ = ops.RbkWarp.apply(rays, idx.expand(H * W), M, 0.1, None, None, *tens)
    c_ref = warped.view(H, W, 5, 3, 2)[H // 2, W // 2]
    c_diff = int((_bits(centre) != _bits(c_ref)).sum())
    ro, rd = O.get_rays(H, W, K, c2w)
    with torch.no_grad():
        o_rays, _ = O.rbk_forward(p, torch.stack([ro, rd], -1).reshape(-1, 3, 2), torch.full((H * W,), i))
        o_batch = O.pack_rays(H, W, focal, o_rays, ndc=ndc, near=near, far=far).reshape(H * W, 5, 11).permute(1, 0, 2)
    e_batch = util.relerr(got, o_batch)
    e_centre = util.relerr(centre, o_rays.reshape(H, W, 5, 3, 2)[H // 2, W // 2])
    moved = float((got[1:] - got[:1]).abs().amax())
    print(f"warp_image {H}x{W} {'ndc' if ndc else 'no ndc'} view {i}: {n_diff} of {got.numel()} batch words differ from RbkWarpNdc, {c_diff} of 30 "
          f"centre-ray words from RbkWarp; against the oracle: batch {e_batch:.2e}, centre rays {e_centre:.2e}; sub-frames move the batch by {moved:.2e}")
    assert n_diff == 0 and c_diff == 0
    assert e_batch < 2e-5 and e_centre < 2e-5
    assert moved > 1e-2      # (the warp is there to be seen: 500 x the gate)


@pytest.mark.parametrize("mode", MODES)
def test_sub_frames_match_the_reference_fixture(dev, mode):
    g, H, W, seed, rmnear, chunk, Ns, Ni, scale, focal, K = fixture_case()
    assert chunk == 128 and H * W % chunk != 0      # chunk boundaries (128, 256, 384) fall inside sub-frames (96, 192, ...)
    net = _net(mode)
    poses, idx = _poses(dev)
    rgbs, depths, rays_save = net.render_warped_path(H, W, K, chunk, poses, idx, RK)
    assert rgbs.shape == (2, 5, H, W, 3) and depths.shape == (2, 5, H, W, 1) and rays_save.shape == (2, 5, 3, 2)
    assert not rgbs.requires_grad
    e = (util.relerr(rgbs, g["rgbs"]), util.relerr(depths, g["depths"]), util.relerr(rays_save, g["rays_save"]))
    print(f"render_warped_path [{mode}] against the reference: rgbs {e[0]:.2e}, depths {e[1]:.2e}, rays_save {e[2]:.2e}")
    assert e[0] < 1e-4 and e[1] < 1e-3 and e[2] < 2e-5
    assert net.read_faults() == 0
    # render_factor divides the image as in the reference (:902-905), and a key forward() pops from render_kwargs_test is ignored
    r2 = net.render_warped_path(2 * H, 2 * W, [[2 * focal, 0, W], [0, 2 * focal, H], [0, 0, 1]], chunk, poses, idx,
                                dict(RK, save_warped_ray_img=True), render_factor=2)
    assert r2[0].shape == (2, 5, H, W, 3) and r2[2].shape == (2, 5, 3, 2)


@pytest.mark.parametrize("mode", MODES)
def test_sub_frames_equal_the_piecewise_public_path(dev, mode):
    """mlp_rbk -> render_train_scene on the ray table, reshaped and permuted as :926-933 do: the same bits, whatever row a ray is in."""
    from lush_nerf_amd import ops
    g, H, W, seed, rmnear, chunk, Ns, Ni, scale, focal, K = fixture_case()
    net = _net(mode)
    poses, idx = _poses(dev)
    rgbs, depths, rays_save = net.render_warped_path(H, W, K, chunk, poses, idx, RK)
    for v in range(2):
        rgb, depth, centre = _piecewise(net, H, W, K, chunk, poses[v], idx[v], ops)
        d = [int((_bits(a) != _bits(b)).sum()) for a, b in ((rgbs[v], rgb), (depths[v], depth), (rays_save[v], centre))]
        print(f"render_warped_path [{mode}] pose {v} against mlp_rbk -> render_train_scene: {d[0]} of {rgb.numel()} rgb words, {d[1]} of "
              f"{depth.numel()} depth words, {d[2]} of 30 centre-ray words differ (relerr {util.relerr(rgbs[v], rgb):.1e}, {util.relerr(depths[v], depth):.1e})")
        assert d == [0, 0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_sub_frame_zero_is_the_unwarped_view(dev, mode):
    g, H, W, seed, rmnear, chunk, Ns, Ni, scale, focal, K = fixture_case()
    net = _net(mode)
    poses, idx = _poses(dev)
    rgbs, depths, rays_save = net.render_warped_path(H, W, K, chunk, poses, idx, RK)
    p_rgbs, _, p_depths = net.render_path(H, W, K, chunk, poses, RK)
    d = (int((_bits(rgbs[:, 0]) != _bits(p_rgbs)).sum()), int((_bits(depths[:, 0, ..., 0]) != _bits(p_depths)).sum()))
    big = net.render_warped_path(H, W, K, 1 << 20, poses, idx, RK)
    c = [int((_bits(a) != _bits(b)).sum()) for a, b in zip((rgbs, depths, rays_save), big)]
    print(f"render_warped_path [{mode}] sub-frame 0 against render_path: {d[0]} rgb words, {d[1]} depth words differ; chunk 128 against one "
          f"chunk: {c} words differ")
    assert d == (0, 0) and c == [0, 0, 0]
    # the un-warped centre ray is the pose's own: origin = c2w[:, 3]
    assert _same_bits(rays_save[:, 0, :, 0], poses[:, :3, 3])


def test_full_size_once(dev):
    """One pose at 640 x 1120 in the headline mode.  Time and peak memory are printed, not gated: nobody had measured this path; the
    expectation is about (M+1) x a render_path pose less the noise network."""
    from lush_nerf_amd import ops
    g, _, _, seed, rmnear, _, Ns, Ni, scale, _, _ = fixture_case()
    H, W, focal, chunk = 640, 1120, 900.0, 1024 * 32
    K = [[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]
    net = _net("h,h")
    poses, idx = _poses(dev)
    poses, idx = poses[:1], idx[:1]

    def measured(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1), (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    net.render_warped_path(8, 12, K, chunk, poses, idx, RK)      # (first-call work: packed weights)
    (rgbs, depths, rays_save), ms, mib = measured(lambda: net.render_warped_path(H, W, K, chunk, poses, idx, RK))
    assert rgbs.shape == (1, 5, H, W, 3) and depths.shape == (1, 5, H, W, 1) and rays_save.shape == (1, 5, 3, 2)
    assert bool(torch.isfinite(rgbs).all()) and bool(torch.isfinite(depths).all()) and bool(torch.isfinite(rays_save).all())
    assert net.read_faults() == 0
    (p_rgbs, _, p_depths), ms_path, mib_path = measured(lambda: net.render_path(H, W, K, chunk, poses, RK))
    d0 = (int((_bits(rgbs[:, 0]) != _bits(p_rgbs)).sum()), int((_bits(depths[:, 0, ..., 0]) != _bits(p_depths)).sum()))
    del p_rgbs, p_depths
    (rgb, depth, centre), ms_piece, mib_piece = measured(lambda: _piecewise(net, H, W, K, chunk, poses[0], idx[0], ops))
    d1 = (int((_bits(rgbs[0]) != _bits(rgb)).sum()), int((_bits(depths[0]) != _bits(depth)).sum()), int((_bits(rays_save[0]) != _bits(centre)).sum()))
    print(f"full size {H}x{W}, 5 sub-frames [h,h]: render_warped_path {ms:.1f} ms a pose, peak {mib:.0f} MiB above what was resident; the piecewise "
          f"route {ms_piece:.1f} ms, peak {mib_piece:.0f} MiB; a render_path pose {ms_path:.1f} ms, peak {mib_path:.0f} MiB.  Words that differ: sub-frame 0 "
          f"against render_path {d0}, all sub-frames and the centre rays against the piecewise route {d1}")
    assert d0 == (0, 0) and d1 == (0, 0, 0)
    assert net.read_faults() == 0
