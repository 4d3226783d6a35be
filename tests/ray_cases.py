"""Case builders of tests/test_ray_kernels_cpu.py and tests/test_ray_kernels_gpu.py: the ray-level and image-tail kernels around
the MLP (fused blur-kernel warp, compositing backward, loss scale, image tail) at sizes past one workgroup and off the default
configuration.  Inputs come from lush_nerf_amd.synth seeds; every reference is the CPU oracle (oracle/lush_oracle.py) on the
same inputs, run in float64 (the reference) and in float32 (the yardstick: fp32's own distance from float64 on that case).

Error metric: the column-normalised maximum (colerr).  Gate of a quantity: max(the project's gate, 8 x its yardstick)."""
import numpy as np
import torch

from lush_nerf_amd import synth
from oracle import lush_oracle as O

H, W, FOCAL = synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF
# the project's gates, by quantity (tests/gpu_diag.py: t_warp_ndc / t_rbk, t_composite, t_mix / t_blur_mix)
GATES = {"warp_fwd": 2e-5, "d_rays": 2e-4, "warp_params": 3e-4, "comp_bwd": 2e-5, "tail_fwd": 2e-6, "tail_bwd": 2e-5}
PIECEWISE_FWD, PIECEWISE_BWD = 1e-6, 2e-5      # tests/gpu_diag.py t_warp_ndc: the fused kernels against RbkWarp -> PackRays
SUM_GATE = 2e-5                                # tests/test_dw_queue.py GATE: the same products in another order of the fp32 sums
WN_IMGS = 64                                   # csrc/lush_rbk.hip: images whose per-image sums rbk_warp_ndc_bwd_kernel keeps in LDS
_CACHE = {}


def gate(quantity, yardstick):
    return max(GATES[quantity], 8.0 * yardstick)


def _np64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def colerr(got, ref, ncol=None, exact=()):
    """Column-normalised maximum error: got and ref flattened to [rows, ncol] (ncol = None: the whole tensor is ONE column, a
    parameter gradient), per column max|got - ref| / max|ref|, the worst column.  A column whose reference is constant must be EQUAL, its
    error 0 or inf: the columns `exact` names (near, far) and every column of zeros (a ccw column of a one-image case is constant
    too, but computed: it is measured like any other)."""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    g, r = (g.reshape(-1, 1), r.reshape(-1, 1)) if ncol is None else (g.reshape(-1, ncol), r.reshape(-1, ncol))
    worst = 0.0
    for c in range(r.shape[1]):
        gc, rc = g[:, c], r[:, c]
        if c in exact or not np.any(rc):
            e = 0.0 if np.array_equal(gc, rc) else float("inf")
        else:
            d = np.abs(gc - rc)
            e = float(d.max() / np.abs(rc).max()) if np.all(np.isfinite(d)) else float("inf")
        worst = max(worst, e)
    return worst


def _t(a, dt, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).requires_grad_(grad)


def _grad(t):
    return torch.zeros_like(t) if t.grad is None else t.grad


# ------------------------------------------------------------------------------------------ (a) the fused warp
RBK_KEYS = ["mlp_rbk.view_embedding_layer.view_embed_layer.weight"] + \
           [f"mlp_rbk.view_embed_linears.{l}.{s}" for l in range(4) for s in ("weight", "bias")] + \
           [f"mlp_rbk.{n}.{s}" for n in ("r_branch.0", "v_branch.0", "w_branch.0", "r_linear", "v_linear", "w_linear") for s in ("weight", "bias")]
RBK_NAMES = ["embed"] + [f"trunk{l}.{s}" for l in range(4) for s in "wb"] + \
            [f"{n}.{s}" for n in ("r_branch", "v_branch", "w_branch", "r_linear", "v_linear", "w_linear") for s in "wb"]
RV_HEADS = [i for i, n in enumerate(RBK_NAMES) if n.split(".")[0] in ("r_branch", "v_branch", "r_linear", "v_linear")]
W_HEAD = [i for i, n in enumerate(RBK_NAMES) if n.split(".")[0] in ("w_branch", "w_linear")]
RV_WINDOW = 0.1
# (n_img, M, N, ndc): N = 51 / 52 straddle the rays per workgroup at M = 4 (256 / 5), n_img = 64 / 65 / 80 straddle WN_IMGS
WARP_SHAPES = [(30, 4, N, ndc) for N in (51, 52, 255) for ndc in (True, False)] + \
              [(80, 2, 300, True), (65, 1, 257, False), (64, 3, 130, True), (1, 3, 130, True), (5, 4, 1, True)]
WARP_VARIANTS = ("partial_mask", "zero_mask", "ccw_only")      # of (30, 4, 255, ndc on)
WARP_RUNS = [s + ("plain",) for s in WARP_SHAPES] + [(30, 4, 255, True, v) for v in WARP_VARIANTS]
BATCH_LIVE = np.array([1., 1., 1., 1., 1., 1., 0., 0., 1., 1., 1.], np.float32)      # near / far carry no gradient


def warp_id(run):
    n_img, M, N, ndc, variant = run
    return f"img{n_img}-M{M}-N{N}-{'ndc' if ndc else 'nondc'}-{variant}"


def warp_rpb(M, N):
    """Rays per workgroup of lush_rbk_warp_ndc_bwd."""
    return min(256 // (M + 1), N)


def warp_inputs(run):
    """rays [N,3,2], images_idx [N], mask [N] uint8 or None, the blur kernel's parameters, upstream gradients (gb None: on ccw only)."""
    key = ("warp_in",) + tuple(run)
    if key not in _CACHE:
        n_img, M, N, ndc, variant = run
        seed = 200 + n_img + 10 * M + N
        b = synth.ray_batch(N, seed, n_img)
        p = synth.rbk_weights(n_img, seed, num_motion=M)
        for k in ("mlp_rbk.r_linear.weight", "mlp_rbk.v_linear.weight"):      # as t_rbk: a warp that is not numerically the identity
            p[k] = p[k] * np.float32(3.0e5)
        mask = {"plain": None, "ccw_only": None, "partial_mask": b["fq_mask"], "zero_mask": np.zeros_like(b["fq_mask"])}[variant]
        gb = None if variant == "ccw_only" else synth.normal((N * (M + 1), 11), 65, N) * BATCH_LIVE
        gc = synth.normal((N, M + 1), 66, N)
        _CACHE[key] = dict(rays=b["rays"], idx=b["images_idx"].reshape(-1), mask=mask, params=p, gb=gb, gc=gc,
                           near=0. if ndc else 2., far=1. if ndc else 6.)
    return _CACHE[key]


def warp_oracle(run, dt):
    """O.rbk_forward(num_motion=M) -> O.pack_rays in dtype dt: batch, ccw, d(rays), the parameter gradients (in RBK_KEYS order)."""
    key = ("warp", dt) + tuple(run)
    if key not in _CACHE:
        n_img, M, N, ndc, variant = run
        x = warp_inputs(run)
        p = {k: _t(v, dt, True) for k, v in x["params"].items()}
        rays = _t(x["rays"], dt, True)
        new_rays, ccw = O.rbk_forward(p, rays, torch.from_numpy(x["idx"]), num_motion=M, rv_window=RV_WINDOW)
        if x["mask"] is not None:
            m = torch.from_numpy(x["mask"]).bool().repeat_interleave(M + 1)
            new_rays = torch.where(m[:, None, None], new_rays, new_rays.detach())
        batch = O.pack_rays(H, W, FOCAL, new_rays, ndc=ndc, near=x["near"], far=x["far"])
        loss = (ccw * _t(x["gc"], dt)).sum()
        if x["gb"] is not None:
            loss = loss + (batch * _t(x["gb"], dt)).sum()
        loss.backward()
        _CACHE[key] = dict(batch=batch.detach(), ccw=ccw.detach(), d_rays=_grad(rays), params=[_grad(p[k]) for k in RBK_KEYS])
    return _CACHE[key]


def warp_errors(got, ref, M):
    """{quantity: column-normalised error} of one warp result against another (batch: 11 columns, ccw: M + 1, d(rays): the 6 ray
    components, each parameter gradient one column)."""
    e = {"batch": colerr(got["batch"], ref["batch"], 11, exact=(6, 7)), "ccw": colerr(got["ccw"], ref["ccw"], M + 1),
         "d_rays": colerr(got["d_rays"], ref["d_rays"], 6)}
    for n, a, b in zip(RBK_NAMES, got["params"], ref["params"]):
        e["param." + n] = colerr(a, b)
    return e


def warp_quantity(name):
    return "warp_params" if name.startswith("param.") else ("d_rays" if name == "d_rays" else "warp_fwd")


# ------------------------------------------------------------------------------------------ (b) compositing backward
RMNEAR = 80
# (R, S, train, white_bkgd): R = 8262 = 2048 x 4 + 70 rays, so the first 18 workgroups walk a second trip of rays
COMP_RUNS = [(70, 64, True, 0), (70, 64, True, 1), (8262, 64, True, 0), (8262, 200, False, 0)]
COMP_ZERO_N, COMP_ZERO_TAIL = 70001, 37


def comp_id(run):
    R, S, train, white = run
    return f"R{R}-S{S}-{'train' if train else 'eval'}-white{white}"


def comp_inputs(run):
    """t_composite's inputs at (R, S): raw, z, the ray batch, the noise draw, the three upstream gradients."""
    key = ("comp_in",) + tuple(run)
    if key not in _CACHE:
        R, S, train, white = run
        raw = synth.normal((R, S, 4), 11, S) * np.array([1., 1., 1., 30.], np.float32)
        z = np.sort(synth.uniform((R, S), 0, 1, 12, S), -1)
        batch = O.pack_rays(H, W, FOCAL, torch.from_numpy(synth.ray_batch(R, 4, 30)["rays"])).numpy()
        noise = synth.normal((R, S - 1), 13, S) if train else None
        g = [synth.normal(s, 14, i) for i, s in enumerate(((R, 3), (R,), (R,)))]
        _CACHE[key] = dict(raw=raw, z=z, batch=batch, noise=noise, g=g, noise_std=1. if train else 0.,
                           near_mask=-1. if train else RMNEAR / 128)
    return _CACHE[key]


def comp_oracle(run, dt):
    key = ("comp", dt) + tuple(run)
    if key not in _CACHE:
        R, S, train, white = run
        x = comp_inputs(run)
        raw, d = _t(x["raw"], dt, True), _t(x["batch"][:, 3:6], dt, True)
        res = O.raw2outputs(raw, _t(x["z"], dt), d, x["noise_std"], bool(white), _t(x["noise"], dt) if train else None,
                            training=train, render_rmnearplane=RMNEAR)
        g = [_t(a, dt) for a in x["g"]]
        ((res[0] * g[0]).sum() + (res[4] * g[1]).sum() + (res[2] * g[2]).sum()).backward()
        _CACHE[key] = dict(d_raw=raw.grad, d_rays_d=d.grad)
    return _CACHE[key]


def comp_errors(got, ref):
    return {"d_raw": colerr(got["d_raw"], ref["d_raw"], 4), "d_rays_d": colerr(got["d_rays_d"], ref["d_rays_d"], 3)}


def comp_block_rays(R, blocks, b):
    """The rays workgroup b of composite_bwd_kernel walks: 4 per trip (one per wave), `blocks` workgroups apart."""
    r = np.arange(R)
    return r[(r // 4) % blocks == b]


# ------------------------------------------------------------------------------------------ (c) the loss scale
SCALE_NS = (1, 255, 256, 257, 2048)
SCALE_MAXIMA = [("1.0", 1.0), ("8.0", 8.0), ("15.999", 15.999), ("16.0", 16.0), ("3e-5", 3e-5), ("1e30", 1e30), ("2.9e38", 2.9e38),
                ("2^-123", 2.0 ** -123), ("1.5e-38", 1.5e-38), ("1e-42", 1e-42), ("zero", 0.0), ("inf", float("inf")), ("nan", float("nan"))]
SCALE_K_MAX = 126      # the clamp: scale <= 2^126, so that 1 / scale is a normal float


def scale_exponent(mx):
    """k of the unclamped rule for a float32 maximum: 2^k puts mx into [8, 16); None where the rule answers {1, 1}."""
    mx = np.float32(mx)
    if not (mx > 0 and mx < np.float32(3.0e38)):
        return None
    return 4 - int(np.frexp(mx)[1])


def scale_expected(mx):
    """(scale, 1 / scale) the kernels must give EXACTLY, or None for the small maxima (k > SCALE_K_MAX), where scale_small_ok holds."""
    k = scale_exponent(mx)
    if k is None:
        return (np.float32(1.0), np.float32(1.0))
    if k > SCALE_K_MAX:
        return None
    return (np.ldexp(np.float32(1.0), k), np.ldexp(np.float32(1.0), -k))


def scale_small_ok(mx, scale, inv):
    """What holds below 2^-122: scale a finite power of two, 1 / scale a non-zero NORMAL float and the exact reciprocal, and the
    scaled maximum at most 16."""
    scale, inv, mx = np.float32(scale), np.float32(inv), np.float32(mx)
    tiny = np.finfo(np.float32).tiny
    return bool(np.isfinite(scale) and scale > 0 and np.frexp(scale)[0] == 0.5 and np.isfinite(inv) and inv >= tiny
                and float(scale) * float(inv) == 1.0 and float(mx) * float(scale) <= 16.0)


def scale_cases():
    """[(tag, n, block_max [n] float32, the maximum)]: every maximum first, last and at index 256, the other entries below it."""
    out = []
    for n in SCALE_NS:
        for pos in sorted({0, n - 1} | ({256} if n > 256 else set())):
            for tag, mx in SCALE_MAXIMA:
                with np.errstate(invalid="ignore", over="ignore"):
                    mx32 = np.float32(mx)
                    if np.isfinite(mx32):
                        a = (np.float64(mx32) * synth.uniform((n,), 0.0, 0.9, 31, n + pos).astype(np.float64)).astype(np.float32)
                    else:
                        a = np.ones(n, np.float32)
                a[pos] = mx32
                out.append((f"n={n} at {pos} max {tag}", n, a, mx32))
    return out


SCALE_KS = (-100, -20, 20, 60)
SCALE_K_TINY = -130
# (net code, prefix, depth, R, S): the noise net, one workgroup of grad_scale_kernel, 19 of them, and past the 32 768 points where
# the chain kernels take over
MLP_LAUNCHES = [(1, "mlp_noise_coarse", 4, 100, 1), (0, "mlp_coarse", 8, 24, 40), (0, "mlp_coarse", 8, 300, 64), (0, "mlp_coarse", 8, 520, 64)]


def mlp_inputs(net, R, S):
    """t_mlp_bwd's inputs at (R, S): the ray batch, z, d_raw (column 3 zero for the noise net)."""
    seed = 41
    batch = O.pack_rays(H, W, FOCAL, torch.from_numpy(synth.ray_batch(R, seed, 30)["rays"])).numpy()
    z = np.sort(synth.uniform((R, S), 0, 1, seed + 50), -1)
    draw = synth.normal((R * S, 4), 43, R)
    if net == 1:
        draw[:, 3] = 0
    return batch, z, draw


def nerf_tensor_names(prefix, D):
    return [f"{prefix}.pts_linears.{l}.{s}" for l in range(D) for s in ("weight", "bias")] + \
           [f"{prefix}.{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]


# ------------------------------------------------------------------------------------------ (d) the image tail
TAIL_NS = (1, 85, 86, 4097)        # 3 N = 3 / 255 / 258 / 12 291 threads: one workgroup, its last thread, two, many
TAIL_M1 = (2, 3, 5)
TAIL_RUNS = [(N, M1, gamma) for N in TAIL_NS for M1 in TAIL_M1 for gamma in (True, False)]


def tail_inputs(N, M1):
    key = ("tail_in", N, M1)
    if key not in _CACHE:
        ccw = torch.softmax(torch.from_numpy(synth.normal((N, M1), 72, N).astype(np.float64)), -1).float().numpy()
        _CACHE[key] = dict(x=synth.uniform((N * M1, 3), 0.05, 1, 71, N), x0=synth.uniform((N * M1, 3), 0.05, 1, 75, N), ccw=ccw,
                           x1=synth.uniform((N * M1,), 0.05, 1, 76, N), nraw=synth.normal((N, 3), 73, N), pure=synth.uniform((N, 3), 0.05, 1, 77, N),
                           g3=[synth.normal((N, 3), 80 + i, N) for i in range(5)], g1=synth.normal((N,), 86, N))
    return _CACHE[key]


def tail_oracle(N, M1, gamma, dt):
    """The un-fused ops (WSum at C = 3 and C = 1, ToneMap with and without nraw, NoiseAct) and BlurMix (gradients on all five
    outputs: bm_*; on blur / blur0 only: bm2_*), forward and backward, in dtype dt."""
    key = ("tail", N, M1, gamma, dt)
    if key in _CACHE:
        return _CACHE[key]
    i = tail_inputs(N, M1)
    tm = O.tonemap if gamma else (lambda v: v)
    g3, out = [_t(a, dt) for a in i["g3"]], {}
    # WSum
    for tag, xa, g in (("wsum3", i["x"], g3[0]), ("wsum1", i["x1"], _t(i["g1"], dt))):
        x, ccw = _t(xa, dt, True), _t(i["ccw"], dt, True)
        y = O.rbk_weighted_sum(x, ccw)
        (y * g).sum().backward()
        out.update({tag + ".y": y.detach(), tag + ".dx": x.grad, tag + ".dccw": ccw.grad})
    # ToneMap
    for tag, with_n in (("tm", False), ("tmn", True)):
        x, n = _t(i["pure"], dt, True), _t(i["nraw"], dt, True)
        y = tm(x + 0.1 * torch.sigmoid(n)) if with_n else tm(x)
        (y * g3[1]).sum().backward()
        out.update({tag + ".y": y.detach(), tag + ".dx": x.grad})
        if with_n:
            out[tag + ".dn"] = n.grad
    # NoiseAct
    n = _t(i["nraw"], dt, True)
    y = 0.1 * torch.sigmoid(n)
    (y * g3[2]).sum().backward()
    out.update({"na.y": y.detach(), "na.dx": n.grad})
    # BlurMix
    for tag, used in (("bm", range(5)), ("bm2", (0, 1))):
        x, x0, ccw, n = _t(i["x"], dt, True), _t(i["x0"], dt, True), _t(i["ccw"], dt, True), _t(i["nraw"], dt, True)
        pure, pure0, nz = O.rbk_weighted_sum(x, ccw), O.rbk_weighted_sum(x0, ccw), 0.1 * torch.sigmoid(n)
        res = [tm(pure + nz), tm(pure0 + nz), nz, tm(pure), tm(pure0)]
        sum((res[k] * g3[k]).sum() for k in used).backward()
        if tag == "bm":
            out.update({f"bm.{nm}": r.detach() for nm, r in zip(BM_OUT, res)})
        out.update({tag + ".d_rgb": x.grad, tag + ".d_rgb0": x0.grad, tag + ".d_ccw": ccw.grad, tag + ".d_nraw": n.grad})
    _CACHE[key] = out
    return out


BM_OUT = ("blur", "blur0", "noise", "sharp", "sharp0")


def tail_columns(name, M1):
    """(quantity, columns) of a tail_oracle entry: colours have 3 columns, the weights M + 1, a depth or acc value one."""
    fwd = name.split(".")[1] in ("y",) + BM_OUT
    if name.endswith("ccw"):
        return ("tail_bwd", M1)
    if name.startswith("wsum1"):
        return ("tail_fwd" if fwd else "tail_bwd", 1)
    return ("tail_fwd" if fwd else "tail_bwd", 3)


def tail_errors(got, ref, M1):
    return {k: colerr(got[k], ref[k], tail_columns(k, M1)[1]) for k in ref}


LOSS_RUNS = [(N, same, scale) for N in TAIL_NS for same in (False, True) for scale in (1.0, 0.75)]


def loss_inputs(N):
    """a, b, target [N,3]; about 1 % of the entries of a equal the target (the gradient's sign term is 0 there)."""
    key = ("loss_in", N)
    if key not in _CACHE:
        a, b, tg = (synth.uniform((N, 3), 0, 1, s, N) for s in (91, 92, 74))
        hit = synth.uniform((N, 3), 0, 1, 93, N) < 0.01
        if N >= 85:
            hit[7, 1] = True
        a = np.where(hit, tg, a)
        _CACHE[key] = (a, b, tg, int(hit.sum()))
    return _CACHE[key]


def loss_oracle(N, same, scale, dt):
    key = ("loss", N, same, scale, dt)
    if key not in _CACHE:
        a, b, tg, _ = loss_inputs(N)
        ta, tb = _t(a, dt, True), _t(b, dt, True)
        loss = O.train_loss(ta, ta if same else tb, _t(tg, dt)) * scale
        loss.backward()
        _CACHE[key] = dict(loss=loss.detach().reshape(1), ga=ta.grad, gb=None if same else tb.grad)
    return _CACHE[key]


CONSIST_RUNS = [(1, 32), (5, 86), (12, 300)]
CONSIST_THR = float(np.float32(0.8))      # the kernel takes the threshold as a float: the same number in every precision
CONSIST_NONE, CONSIST_ONE = 3, 5      # pixel columns with no view / exactly one view (view 0) above the threshold


def consist_inputs(V, ns):
    rgb = synth.uniform((V, ns, 3), 0, 1, 77, ns)
    cert = synth.uniform((V, ns), 0.5, 1, 78, ns)
    cert[:, CONSIST_NONE] = 0.1
    cert[:, CONSIST_ONE] = 0.1
    cert[0, CONSIST_ONE] = 0.9
    return rgb, cert


def consist_oracle(V, ns, dt):
    key = ("consist", V, ns, dt)
    if key not in _CACHE:
        rgb, cert = consist_inputs(V, ns)
        r = _t(rgb, dt, True)
        loss = O.consist_loss(r, _t(cert, dt), CONSIST_THR)
        loss.backward()
        _CACHE[key] = dict(loss=loss.detach().reshape(1), grad=r.grad)
    return _CACHE[key]
