"""GPU tests of NeRFAll.mlpforward / mlpforward_noise / raw2outputs (models/lushnerf.py:234-352) as public methods: the field at
points the caller chose, compositing on the caller's own z_vals, and their gradients.

Gates are the project's own, by source: tests/gpu_diag.py t_mlp_fwd (raw by plane code), t_mlp_bwd (gradients against the oracle
with the GPU's own ReLU decisions, by mode; input gradients twice that), t_composite (2e-6 forward, 2e-5 backward),
tests/test_dw_queue.py GATE (the same products in another order of the fp32 sums) and the 1e-4 output bound.  Errors are
util.relerr: the largest difference over the reference's largest entry.  Every figure is printed before it is asserted
(lines starting with "FIELD"; profiles/r11_field_query.md records a run)."""
import numpy as np
import pytest
import torch

from tests import field_inputs as FI
from tests import util

pytestmark = pytest.mark.gpu

H16 = 17                                     # ops.PLANES_F16
MODES = {"2,2": (2, 2), "h,h": (H16, H16)}
FWD_GATE = {3: 3e-6, 2: 3e-5, H16: 4e-3}     # tests/gpu_diag.py t_mlp_fwd
BWD_GATE = {(2, 2): 2e-4, (2, H16): 8e-3, (H16, H16): 2e-3}      # tests/gpu_diag.py t_mlp_bwd by (forward, backward) plane code (parameter gradients; input gradients 2 x)
SUM_GATE = 2e-5                              # tests/test_dw_queue.py GATE
COMP_FWD, COMP_BWD = 2e-6, 2e-5              # tests/gpu_diag.py t_composite
RAGGED = ((1, 1), (127, 1), (43, 3), (3, 100), (5, 129))
R2O_NAMES = ("rgb_map", "density", "acc_map", "weights", "depth_map")
NETS = (("mlp_coarse", 0, 8), ("mlp_fine", 0, 8), ("mlp_noise_coarse", 1, 4))
_CACHE = {}


def dev():
    return torch.device("cuda:0")


def gpu(a, grad=False):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev()).requires_grad_(grad)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def model(mode, which="default", train=True):
    """The mirror with the fixture's weights in one precision mode (one per (mode, weights): networks are only read)."""
    import argparse
    from lush_nerf_amd import model as M, ops
    key = ("model", mode, which)
    if key not in _CACHE:
        args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                                  N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                                  rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=FI.RMNEAR)
        net = M.NeRFAll(args, M.RBK(FI.NUM_IMG, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4), precision=ops.Precision(*MODES[mode]))
        M.load_reference_weights(net, FI.weights(which))
        _CACHE[key] = net.to(dev())
    net = _CACHE[key].train(train)
    net.hooks.keep = None
    net.zero_grad(set_to_none=True)
    return net


def params64(which):
    key = ("p64", which)
    if key not in _CACHE:
        _CACHE[key] = {k: torch.from_numpy(v).double() for k, v in FI.weights(which).items()}
    return _CACHE[key]


def free_points(R, S, seed):
    from lush_nerf_amd import synth
    pts = synth.uniform((R, S, 3), -1.2, 1.2, seed, 1)
    d = synth.normal((R, 3), seed, 2).astype(np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * synth.uniform((R, 1), 0.5, 2.0, seed, 3)
    return pts, d.astype(np.float32)


def pseudo_rays(pts, dirs):
    """What lush_points_pack must produce, built with torch: rows [pt, 0,0,0, 0, 1, dir], z = 0."""
    R, S = pts.shape[:2]
    rays = torch.zeros(R * S, 11, device=pts.device)
    rays[:, 0:3] = pts.reshape(-1, 3)
    rays[:, 7] = 1.0
    rays[:, 8:11] = dirs[:, None].expand(R, S, 3).reshape(-1, 3)
    return rays, torch.zeros(R * S, 1, device=pts.device)


def noise_planes(mode):
    from lush_nerf_amd import ops
    pr = ops.Precision(*MODES[mode]).noise()
    return pr.fwd, pr.bwd


def fwd_planes(mode, code):
    return noise_planes(mode)[0] if code == 1 else MODES[mode][0]


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("R,S", RAGGED)
def test_points_pack_bit_for_bit(R, S):
    from lush_nerf_amd import ops
    pts, dirs = (gpu(a) for a in free_points(R, S, 70 + S))
    pts[0, 0, 0] = -0.0      # (a sign bit must survive too)
    rays, z = ops.points_pack(pts, dirs)
    want_rays, want_z = pseudo_rays(pts, dirs)
    assert same_bits(rays, want_rays) and same_bits(z, want_z)


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("mode", list(MODES))
def test_mlpforward_is_the_direct_launch_bit_for_bit(mode):
    from lush_nerf_amd import ops
    net = model(mode)
    pts, dirs = (gpu(a) for a in free_points(43, 3, 71))
    rays, z = pseudo_rays(pts, dirs)
    with torch.no_grad():
        for name, code, _ in NETS:
            mlp = getattr(net, name)
            got = net.mlpforward(pts, dirs, mlp, False, False)
            tens = [t.detach() for t in mlp.tensors()]
            pf = fwd_planes(mode, code)
            raw, _ = ops.mlp_forward(code, pf, tens, ops.mlp_pack(code, pf, tens), rays, z, False)
            raw = raw.view(43, 3, 4)
            assert same_bits(got, raw[..., :3] if code == 1 else raw), name
            assert tuple(got.shape) == ((43, 3, 3) if code == 1 else (43, 3, 4))
        got = net.mlpforward_noise(gpu(FI.points_noise()), gpu(FI.dirs()), net.mlp_noise_coarse, False, False)
        want = net.mlpforward(gpu(FI.points_noise())[:, 16:17], gpu(FI.dirs()), net.mlp_noise_coarse, False, False)[:, 0]
        assert tuple(got.shape) == (FI.R, 3) and same_bits(got, want)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("mode", list(MODES))
def test_forward_parity_with_the_reference_and_float64(mode):
    from oracle import lush_oracle as O
    g = util.golden("field_query")
    errs, bad = [], []

    def check(tag, got, ref, tol):
        e = util.relerr(got, ref)
        print(f"FIELD fwd {mode} {tag}: {e:.3e} (gate {tol:.0e})")
        errs.append(e)
        if not e <= tol:
            bad.append((tag, e, tol))

    with torch.no_grad():
        for which in FI.WEIGHT_SETS:
            net = model(mode, which)
            for name in ("mlp_coarse", "mlp_fine"):
                got = net.mlpforward(gpu(FI.points()), gpu(FI.dirs()), getattr(net, name), False, False)
                ref = g[f"{which}.raw.{name}"]
                check(f"fixture {which} {name} rgb", got[..., :3], ref[..., :3], FWD_GATE[MODES[mode][0]])
                check(f"fixture {which} {name} sigma", got[..., 3], ref[..., 3], FWD_GATE[MODES[mode][0]])
            got = net.mlpforward_noise(gpu(FI.points_noise()), gpu(FI.dirs()), net.mlp_noise_coarse, False, False)
            check(f"fixture {which} noise", got, g[f"{which}.noise"], FWD_GATE[noise_planes(mode)[0]])
        net, p = model(mode), params64("default")
        for R, S in RAGGED:
            pts, dirs = free_points(R, S, 72 + R)
            ref = O.mlpforward(p, "mlp_coarse", torch.from_numpy(pts).double(), torch.from_numpy(dirs).double())
            got = net.mlpforward(gpu(pts), gpu(dirs), net.mlp_coarse, False, False)
            check(f"float64 ({R},{S}) mlp_coarse rgb", got[..., :3], ref[..., :3], FWD_GATE[MODES[mode][0]])
            check(f"float64 ({R},{S}) mlp_coarse sigma", got[..., 3], ref[..., 3], FWD_GATE[MODES[mode][0]])
            e = torch.cat([O.embed(torch.from_numpy(pts).double().reshape(-1, 3), 10),
                           O.embed(torch.from_numpy(dirs).double()[:, None].expand(R, S, 3).reshape(-1, 3), 4)], -1)
            refn = O.nerf_mlp(p, "mlp_noise_coarse", e, 63, 27, 4, return_alpha=False).reshape(R, S, 3)
            gotn = net.mlpforward(gpu(pts), gpu(dirs), net.mlp_noise_coarse, False, False)
            check(f"float64 ({R},{S}) mlp_noise_coarse", gotn, refn, FWD_GATE[noise_planes(mode)[0]])
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("mode", list(MODES))
def test_collinear_points_agree_with_the_rays_launch(mode):
    """Points o + d*z built with torch (multiply, then add) through the methods, against the rays + z launch of the same points.
    Bit-identity is reported, not required: a point sits in another tile row of the (P,1) launch."""
    from lush_nerf_amd import ops, synth
    from oracle import lush_oracle as O
    net = model(mode)
    R, S = 24, 40
    batch = gpu(O.pack_rays(util.H, util.W, util.FOCAL, torch.from_numpy(synth.ray_batch(R, 31, util.NUM_IMG)["rays"])))
    z = gpu(np.sort(synth.uniform((R, S), 0, 1, 81), -1))
    pts = batch[:, None, 0:3] + batch[:, None, 3:6] * z[:, :, None]
    bad = []
    with torch.no_grad():
        for name, code, _ in NETS:
            mlp = getattr(net, name)
            tens = [t.detach() for t in mlp.tensors()]
            pf = fwd_planes(mode, code)
            raw, _ = ops.mlp_forward(code, pf, tens, ops.mlp_pack(code, pf, tens), batch, z, False)
            raw = raw.view(R, S, 4)[..., :3 if code == 1 else 4]
            got = net.mlpforward(pts, batch[:, 8:11].contiguous(), mlp, False, False)
            e = util.relerr(got, raw)
            print(f"FIELD collinear {mode} {name}: {e:.3e} (gate {FWD_GATE[pf]:.0e}), bit for bit: {same_bits(got, raw)}")
            if not e <= FWD_GATE[pf]:
                bad.append((name, e))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 5
def _direct_backward(net, mlp, code, mode, pts, dirs, d_raw, stash):
    from lush_nerf_amd import ops
    pf, pb = (noise_planes(mode) if code == 1 else MODES[mode])
    tens = [t.detach() for t in mlp.tensors()]
    rays, z = pseudo_rays(pts.detach(), dirs.detach())
    draw = d_raw.reshape(-1, d_raw.shape[-1])
    if code == 1:
        draw = torch.cat([draw, torch.zeros_like(draw[:, :1])], -1)
    return ops.mlp_backward(code, ops.stash_code(pf, pb), pb, tens, ops.mlp_pack(code, pb, tens), rays, z, draw.contiguous(), stash)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("S", [1, 3, 65, 129])
def test_backward_is_the_direct_launch_and_a_fixed_order_sum(mode, S):
    from lush_nerf_amd import synth
    R = 7
    net = model(mode)
    pts_np, dirs_np = free_points(R, S, 90 + S)
    d_raw = gpu(synth.normal((R, S, 4), 91, S))
    bad = []
    runs = []
    for rep in range(2):
        net.zero_grad(set_to_none=True)
        net.hooks.keep = {}
        pts, dirs = gpu(pts_np, True), gpu(dirs_np, True)
        net.mlpforward(pts, dirs, net.mlp_coarse, False, False).backward(d_raw)
        runs.append((pts.grad.clone(), dirs.grad.clone(), [t.grad.clone() for t in net.mlp_coarse.tensors()], net.hooks.keep["stash_field"]))
    net.hooks.keep = None
    d_pts, d_dirs, grads, stash = runs[0]
    assert same_bits(d_pts, runs[1][0]) and same_bits(d_dirs, runs[1][1]), "two runs differ in d(points) / d(viewdirs)"
    ref_grads, dpts = _direct_backward(net, net.mlp_coarse, 0, mode, pts, dirs, d_raw, stash)
    assert same_bits(d_pts, dpts[:, 0:3].reshape(R, S, 3)), "d(points) is not the chain's d(point) rows"
    e = util.relerr(d_dirs, dpts[:, 4:7].double().reshape(R, S, 3).sum(1))
    print(f"FIELD bwd {mode} S={S} d(viewdirs) against the float64 sum: {e:.3e} (gate 2e-06)")
    if not e <= 2e-6:
        bad.append(("d_dirs", e))
    worst = max(util.relerr(a, b) for a, b in zip(grads, ref_grads))
    print(f"FIELD bwd {mode} S={S} parameter gradients against the direct launch: {worst:.3e} (gate {SUM_GATE:.0e})")
    if not worst <= SUM_GATE:
        bad.append(("params", worst))
    assert not bad, bad


def _names(D):
    return [f"pts_linears.{l}.{s}" for l in range(D) for s in ("weight", "bias")] + \
           [f"{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", list(FI.WEIGHT_SETS))
def test_backward_against_the_reference_gradients(mode, which):
    """The fixture's case (reference inputs, reference upstream gradient) in t_mlp_bwd's form: the reference is the oracle with the
    GPU's own ReLU decisions, which isolates arithmetic from kink flips; where the GPU took exactly the oracle's decisions that
    reference IS the fixture's (tests/test_field_query_cpu.py ties the oracle to it), and the fixture is then checked directly."""
    from lush_nerf_amd import ops
    from oracle import lush_oracle as O
    g = util.golden("field_query")
    net = model(mode, which)
    bad = []
    for prefix, code, D, pts_np, up_np, fx in (("mlp_coarse", 0, 8, FI.points(), FI.g_raw(), f"{which}.coarse."),
                                                ("mlp_noise_coarse", 1, 4, FI.points_noise(), FI.g_noise(), f"{which}.noisenet.")):
        pf, pb = (noise_planes(mode) if code == 1 else MODES[mode])
        tol = BWD_GATE[(pf, pb)]      # (the noise net of (h,h) runs as (2,h): ops.Precision.noise)
        net.zero_grad(set_to_none=True)
        net.hooks.keep = {}
        pts, dirs = gpu(pts_np, True), gpu(FI.dirs(), True)
        mlp = getattr(net, prefix)
        if code == 0:
            net.mlpforward(pts, dirs, mlp, False, False).backward(gpu(up_np))
            x_pts = torch.from_numpy(pts_np).requires_grad_(True)
            P, S = FI.R * FI.S, FI.S
        else:
            net.mlpforward_noise(pts, dirs, mlp, False, False).backward(gpu(up_np))
            x_pts = torch.from_numpy(pts_np).requires_grad_(True)
            P, S = FI.R, 1
        stash = net.hooks.keep["stash_field"]
        net.hooks.keep = None
        masks = util.stash_masks(code, ops.nplanes(ops.stash_code(pf, pb)), P, stash, f16=(pf == H16))
        p = {k: torch.from_numpy(v.copy()).requires_grad_(k.startswith(prefix + ".")) for k, v in FI.weights(which).items()}
        x_dirs = torch.from_numpy(FI.dirs()).requires_grad_(True)
        pp = x_pts if code == 0 else x_pts[:, 16:17]
        x = torch.cat([O.embed(pp.reshape(-1, 3), 10), O.embed(x_dirs[:, None].expand(FI.R, S, 3).reshape(-1, 3), 4)], -1)
        own = util.oracle_relu_decisions({k: v.detach() for k, v in p.items()}, prefix, x.detach(), D)
        flips = int(sum(float((a != b).sum()) for a, b in zip(own, masks)))
        out = util.nerf_mlp_masked(p, prefix, x, D, masks)
        up = torch.from_numpy(up_np).reshape(P, -1)
        (out[:, :up.shape[1]] * up).sum().backward()
        worst, wname = 0.0, ""
        for n, t in zip(_names(D), mlp.tensors()):
            ref = p[f"{prefix}.{n}"].grad
            if code == 1 and n.startswith("alpha_linear"):
                assert t.grad is None, "alpha_linear of the noise net must stay without a gradient"
                continue
            e = util.relerr(t.grad, ref)
            if e > worst:
                worst, wname = e, n
        e_pts, e_dirs = util.relerr(pts.grad, x_pts.grad), util.relerr(dirs.grad, x_dirs.grad)
        print(f"FIELD bwd-ref {mode} {which} {prefix}: ReLU decisions that differ from the oracle's {flips}; parameters {worst:.3e} [{wname}] "
              f"(gate {tol:.0e}); d(points) {e_pts:.3e}, d(viewdirs) {e_dirs:.3e} (gate {2 * tol:.0e})")
        if not worst <= tol:
            bad.append((prefix, "params", wname, worst))
        if not e_pts <= 2 * tol:
            bad.append((prefix, "d_pts", e_pts))
        if not e_dirs <= 2 * tol:
            bad.append((prefix, "d_dirs", e_dirs))
        if flips == 0:      # the masked oracle is then the reference run itself: the fixture's numbers, directly
            f_pts, f_dirs = util.relerr(pts.grad, g[fx + "d_pts"]), util.relerr(dirs.grad, g[fx + "d_dirs"])
            named = {f"{prefix}.{n}": t.grad for n, t in zip(_names(D), mlp.tensors()) if t.grad is not None}
            f_par = max(util.check_grads(named, {k[len(fx):]: v for k, v in g.items() if k.startswith(fx)}, tol).values())
            print(f"FIELD bwd-ref {mode} {which} {prefix}: against the fixture directly: parameters {f_par:.3e}, d(points) {f_pts:.3e}, d(viewdirs) {f_dirs:.3e}")
            if not (f_pts <= 2 * tol and f_dirs <= 2 * tol):
                bad.append((prefix, "fixture", f_pts, f_dirs))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 6, 7
R2O_S = (2, 3, 32, 64, 65, 128, 200, 256)
R2O_RUNS = [(S, train, 30) for S in R2O_S for train in (True, False)] + [(S, train, 3000) for S in R2O_S if S >= 32 for train in (True, False)]


def r2o_case(S, train, scale):
    """Inputs in t_composite's form (R = 70) and the float64 oracle's results and gradients under random upstream gradients on all
    five results, computed once and shared."""
    from lush_nerf_amd import synth
    from oracle import lush_oracle as O
    key = ("r2o", S, train, scale)
    if key not in _CACHE:
        R = 70
        raw = synth.normal((R, S, 4), 11, S) * np.array([1., 1., 1., scale], np.float32)
        z = np.sort(synth.uniform((R, S), 0, 1, 12, S), -1)
        d = O.pack_rays(util.H, util.W, util.FOCAL, torch.from_numpy(synth.ray_batch(R, 4, util.NUM_IMG)["rays"]))[:, 3:6].contiguous().numpy()
        noise = synth.normal((R, S - 1), 13, S)
        shapes = dict(rgb_map=(R, 3), density=(R, S - 1), acc_map=(R,), weights=(R, S), depth_map=(R,))
        up = {k: synth.normal(sh, 14, i) for i, (k, sh) in enumerate(shapes.items())}
        r64, z64, d64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (raw, z, d))
        res = O.raw2outputs(r64, z64, d64, 1. if train else 0., False, torch.from_numpy(noise).double() if train else None,
                            training=train, render_rmnearplane=FI.RMNEAR)
        torch.autograd.backward(list(res), [torch.from_numpy(up[k]).double() for k in R2O_NAMES])
        ref = {k: v.detach() for k, v in zip(R2O_NAMES, res)}
        ref.update(d_raw=r64.grad, d_z=z64.grad, d_rays_d=d64.grad)
        _CACHE[key] = (raw, z, d, noise, up, ref)
    return _CACHE[key]


def r2o_gpu(S, train, scale, up_keys=R2O_NAMES):
    raw, z, d, noise, up, ref = r2o_case(S, train, scale)
    net = model("2,2", train=train)
    r, zz, dd = gpu(raw, True), gpu(z, True), gpu(d, True)
    res = net.raw2outputs(r, zz, dd, raw_noise_std=1. if train else 0., noise=gpu(noise) if train else None)
    keep = [(v, gpu(up[k])) for k, v in zip(R2O_NAMES, res) if k in up_keys]
    torch.autograd.backward([a for a, _ in keep], [b for _, b in keep])
    return dict(zip(R2O_NAMES, res)), dict(d_raw=r.grad, d_z=zz.grad, d_rays_d=dd.grad), ref


@pytest.mark.parametrize("S,train,scale", R2O_RUNS)
def test_raw2outputs_forward_and_backward_against_float64(S, train, scale):
    from lush_nerf_amd import ops
    out, grads, ref = r2o_gpu(S, train, scale)
    tag = f"S={S} {'train' if train else 'eval'} x{scale}"
    bad = []
    for k in R2O_NAMES:
        e = util.relerr(out[k], ref[k])
        print(f"FIELD r2o fwd {tag} {k}: {e:.3e} (gate {COMP_FWD:.0e})")
        if not e <= COMP_FWD:
            bad.append((k, e))
    for k, v in grads.items():
        e = util.relerr(v, ref[k])
        print(f"FIELD r2o bwd {tag} {k}: {e:.3e} (gate {COMP_BWD:.0e})")
        if not (e <= COMP_BWD and bool(torch.isfinite(v).all())):
            bad.append((k, e))
    if scale == 3000:
        sat = float((out["weights"][:, :-1] > 0).float().mean())
        print(f"FIELD r2o {tag}: share of samples before the last with a weight: {sat:.3f}")
    # without upstream gradients on weights and density: the march's own compositing backward
    raw, z, d, noise, up, _ = r2o_case(S, train, scale)
    _, g3, _ = r2o_gpu(S, train, scale, up_keys=("rgb_map", "acc_map", "depth_map"))
    batch = torch.zeros(70, 11, device=dev())
    batch[:, 3:6] = gpu(d)
    cfg = ops.MarchCfg(S, 0, 0., 1. if train else 0., near_mask=-1. if train else FI.RMNEAR / 128)
    drays = torch.zeros(70, 11, device=dev())
    draw = ops.composite_bwd(gpu(raw).reshape(-1, 4), gpu(z), batch, gpu(noise) if train else None, cfg,
                             gpu(up["rgb_map"]), gpu(up["depth_map"]), gpu(up["acc_map"]), drays)
    e1, e2 = util.relerr(g3["d_raw"], draw.view(70, S, 4)), util.relerr(g3["d_rays_d"], drays[:, 3:6])
    print(f"FIELD r2o bwd {tag} against lush_composite_bwd: d_raw {e1:.3e}, d_rays_d {e2:.3e} (gate 2e-06)")
    if not (e1 <= 2e-6 and e2 <= 2e-6):
        bad.append(("lush_composite_bwd", e1, e2))
    assert not bad, bad


@pytest.mark.parametrize("case", [c[0] for c in FI.R2O_CASES])
def test_raw2outputs_fixture_cases(case):
    g = util.golden("field_query")
    _, training, std, white = next(c for c in FI.R2O_CASES if c[0] == case)
    raw_np, z_np, noise_np = FI.r2o_inputs()
    up = FI.r2o_upstream()
    net = model("2,2", train=training)
    raw, z, d = gpu(raw_np, True), gpu(z_np, True), gpu(FI.dirs(), True)
    res = net.raw2outputs(raw, z, d, raw_noise_std=std, white_bkgd=white, noise=gpu(noise_np) if std > 0 else None)
    torch.autograd.backward(list(res), [gpu(up[k]) for k in R2O_NAMES])
    bad = []
    for k, v in zip(R2O_NAMES, res):
        e = util.relerr(v, g[f"r2o.{case}.{k}"])
        print(f"FIELD r2o fixture {case} {k}: {e:.3e} (gate {COMP_FWD:.0e})")
        if not e <= COMP_FWD:
            bad.append((k, e))
    for k, v in (("d_raw", raw.grad), ("d_z", z.grad), ("d_rays_d", d.grad)):
        e = util.relerr(v, g[f"r2o.{case}.{k}"])
        print(f"FIELD r2o fixture {case} {k}: {e:.3e} (gate {COMP_BWD:.0e})")
        if not (e <= COMP_BWD and bool(torch.isfinite(v).all())):
            bad.append((k, e))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("mode", list(MODES))
def test_field_then_compositing_reproduces_the_coarse_render(mode):
    from lush_nerf_amd import ops, synth
    from oracle import lush_oracle as O
    net = model(mode, "trained", train=False)
    R, S = 48, 64
    batch = gpu(O.pack_rays(util.H, util.W, util.FOCAL, torch.from_numpy(synth.ray_batch(R, 33, util.NUM_IMG)["rays"])))
    with torch.no_grad():
        ret = net.render_rays_nonoise(batch, S, N_importance=0)
        z = ops.zgrid(batch, S, False, None)
    pts = batch[:, None, 0:3] + batch[:, None, 3:6] * z[:, :, None]
    raw = net.mlpforward(pts, batch[:, 8:11].contiguous(), net.mlp_coarse, False, False)
    rgb_map, density, acc_map, weights, depth_map = net.raw2outputs(raw, z, batch[:, 3:6].contiguous())
    bad = []
    for k, v in (("rgb_map", rgb_map), ("acc_map", acc_map), ("depth_map", depth_map), ("density_map", density)):
        e = util.relerr(v, ret[k])
        print(f"FIELD user {mode} {k} against render_rays_nonoise: {e:.3e} (bound 1e-04)")
        if not e <= 1e-4:
            bad.append((k, e))
    assert float(weights.detach()[:, :-1].max()) > 0.05     # the field has surfaces: compositing is more than the last sample
    (rgb_map.sum() + weights.var()).backward()
    for n, t in zip(_names(8), net.mlp_coarse.tensors()):
        if t.grad is None or not bool(torch.isfinite(t.grad).all()) or float(t.grad.abs().max()) == 0:
            bad.append((n, "no finite non-zero gradient"))
    assert all(t.grad is None for t in net.mlp_fine.tensors())
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 9
def test_raw2outputs_draws_its_noise_from_the_models_counter():
    from lush_nerf_amd import ops
    raw_np, z_np, _ = FI.r2o_inputs()
    net = model("2,2")
    raw, z, d = gpu(raw_np), gpu(z_np), gpu(FI.dirs())
    o0 = net.hooks.draw_offset
    a = net.raw2outputs(raw, z, d, raw_noise_std=1.)
    assert net.hooks.draw_offset == o0 + 1
    b = net.raw2outputs(raw, z, d, raw_noise_std=1.)
    assert net.hooks.draw_offset == o0 + 2
    assert not torch.equal(a[1], b[1])      # another draw, other densities
    noise = ops.march_draws(FI.R, FI.S, 0, 0., 1., dev(), stream_id=net.rng_stream, offset=o0 + 1)["noise_c"]
    c = net.raw2outputs(raw, z, d, raw_noise_std=1., noise=noise)
    assert net.hooks.draw_offset == o0 + 2      # an explicit draw takes none
    assert all(same_bits(x, y) for x, y in zip(a, c))
    e = net.raw2outputs(raw, z, d)
    assert net.hooks.draw_offset == o0 + 2 and not torch.equal(e[1], a[1])
