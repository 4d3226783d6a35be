"""GPU tests of the kernels around the MLP, past one workgroup and off the default configuration: the fused blur-kernel warp
(rbk_warp_ndc_fwd / _bwd_kernel), the side duties of composite_bwd_kernel, the loss scale of the fp16 gradient chain
(loss_scale_kernel directly, grad_scale_kernel through ops.mlp_backward) and the image tail (wsum_*, tonemap_*, noise_act_*,
blur_mix_*, loss_kernel, consist_loss_kernel).

References: the CPU oracle in float64 on the same inputs (tests/ray_cases.py builds the cases, for this file and for
tests/test_ray_kernels_cpu.py).  Errors are column-normalised maxima (ray_cases.colerr).  Gate of a quantity = max(the project's
gate from tests/gpu_diag.py, 8 x the fp32 oracle's own distance from float64 on that case); "exact" is equal bits.  Every figure
is printed before it is asserted (lines starting with "RAYK"; profiles/r18_ray_kernels.md records a run)."""
import numpy as np
import pytest
import torch

from tests import ray_cases as RC
from tests import util

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
H16 = 17                                     # ops.PLANES_F16


def dev():
    return torch.device("cuda:0")


def gpu(a, grad=False):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev()).requires_grad_(grad)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def _zeros_if_none(g, like):
    return torch.zeros_like(like) if g is None else g


class Report:
    """Prints `RAYK <tag> <name>: error (yardstick, gate)` and keeps what missed."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def gated(self, name, err, quantity, yardstick):
        g = RC.gate(quantity, yardstick)
        print(f"RAYK {self.tag} {name}: {err:.3e} (yardstick {yardstick:.3e}, gate {g:.1e})")
        if not err <= g:
            self.bad.append((name, err, g))

    def bound(self, name, err, tol):
        print(f"RAYK {self.tag} {name}: {err:.3e} (gate {tol:.1e})")
        if not err <= tol:
            self.bad.append((name, err, tol))

    def exact(self, name, ok):
        print(f"RAYK {self.tag} {name}: {'exact' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append((name, "not exact"))

    def done(self):
        assert not self.bad, self.bad


# ------------------------------------------------------------------------------------------ (a) the fused warp
def _warp_gpu(run, fused, retain=False):
    from lush_nerf_amd import ops
    n_img, M, N, ndc, variant = run
    x = RC.warp_inputs(run)
    tens = [gpu(x["params"][k], True) for k in RC.RBK_KEYS]
    rg = gpu(x["rays"], True)
    mask = None if x["mask"] is None else gpu(x["mask"])
    batch0 = None
    if fused:
        batch, ccw, batch0 = ops.RbkWarpNdc.apply(rg, gpu(x["idx"]), M, RC.RV_WINDOW, mask, None, RC.H, RC.W, RC.FOCAL, ndc, x["near"], x["far"], *tens)
    else:
        nr, ccw = ops.RbkWarp.apply(rg, gpu(x["idx"]), M, RC.RV_WINDOW, mask, None, *tens)
        batch = ops.PackRays.apply(nr, RC.H, RC.W, RC.FOCAL, ndc, x["near"], x["far"])
    loss = (ccw * gpu(x["gc"])).sum()
    if x["gb"] is not None:
        loss = loss + (batch * gpu(x["gb"])).sum()
    loss.backward(retain_graph=retain)
    out = dict(batch=batch.detach(), ccw=ccw.detach(), batch0=batch0, d_rays=_zeros_if_none(rg.grad, rg).clone(),
               params=[_zeros_if_none(t.grad, t).clone() for t in tens])
    return (out, loss, rg, tens) if retain else out


@pytest.mark.parametrize("run", RC.WARP_RUNS, ids=RC.warp_id)
def test_fused_warp_against_float64(run):
    n_img, M, N, ndc, variant = run
    rep = Report("warp " + RC.warp_id(run))
    ref = RC.warp_oracle(run, F64)
    yard = RC.warp_errors(RC.warp_oracle(run, F32), ref, M)
    got = _warp_gpu(run, fused=True)
    for k, e in RC.warp_errors(got, ref, M).items():
        rep.gated(k, e, RC.warp_quantity(k), yard[k])
    rep.exact("batch0 = the slot-0 rows of batch", same_bits(got["batch0"], got["batch"].view(N, M + 1, 11)[:, 0]))
    if n_img > RC.WN_IMGS:
        assert int(RC.warp_inputs(run)["idx"].max()) >= RC.WN_IMGS
    if variant == "zero_mask":
        rep.exact("d(rays) is zero", not bool(got["d_rays"].any()))
        rep.exact("r / v heads' gradients are zero", all(not bool(got["params"][i].any()) for i in RC.RV_HEADS))
        rep.exact("the weight head's gradients are not", all(bool(got["params"][i].any()) for i in RC.W_HEAD))
    # the piecewise ops on the same inputs (the fused kernels run the same device functions)
    pw = _warp_gpu(run, fused=False)
    for k, e in RC.warp_errors(got, pw, M).items():
        rep.bound("vs RbkWarp -> PackRays " + k, e, RC.PIECEWISE_FWD if k in ("batch", "ccw") else RC.PIECEWISE_BWD)
    rep.done()


def test_fused_warp_second_backward_over_a_retained_graph():
    """rbk_mlp_bwd_kernel leaves d_rvw (the tail of the activation rows the node keeps) zero: a second backward adds the same
    gradients again.  80 images: the per-image sums go to d_rvw by global atomics."""
    run = (80, 2, 300, True, "plain")
    rep = Report("warp retained " + RC.warp_id(run))
    first, loss, rg, tens = _warp_gpu(run, fused=True, retain=True)
    loss.backward()
    rep.bound("d(rays) after two backwards against 2 x the first", RC.colerr(rg.grad, 2 * first["d_rays"], 6), 2e-5)
    for n, t, g in zip(RC.RBK_NAMES, tens, first["params"]):
        rep.bound(f"param.{n} after two backwards against 2 x the first", RC.colerr(t.grad, 2 * g), 2e-5)
    rep.done()


# ------------------------------------------------------------------------------------------ (b) compositing backward side duties
def _composite_bwd(run, extras, init_drays):
    """lush_composite_bwd on the case; extras: block_max, zero_buf (inside a larger NaN buffer) and drays filled with 7.0 are passed,
    otherwise NULL, NULL, 0, 0 and zeroed drays."""
    from lush_nerf_amd import lib, ops
    R, S, train, white = run
    x = RC.comp_inputs(run)
    raw, z, batch = gpu(x["raw"].reshape(-1, 4)), gpu(x["z"]), gpu(x["batch"])
    noise = gpu(x["noise"]) if train else None
    g = [gpu(a) for a in x["g"]]
    draw = torch.full((R * S, 4), float("nan"), device=dev())
    blocks = int(lib.load().lush_composite_bwd_blocks(R))
    out = dict(blocks=blocks)
    if extras:
        bmax = torch.full((blocks,), float("nan"), device=dev())
        zbuf = torch.full((RC.COMP_ZERO_N + RC.COMP_ZERO_TAIL,), float("nan"), device=dev())
        drays = torch.full((R, 11), 7.0, device=dev())
        args = (lib.ptr(bmax), lib.ptr(zbuf), RC.COMP_ZERO_N, int(init_drays))
        out.update(block_max=bmax, zero_buf=zbuf)
    else:
        drays = torch.zeros(R, 11, device=dev())
        args = (None, None, 0, 0)
    lib.call("lush_composite_bwd", lib.ptr(raw), lib.ptr(z), lib.ptr(batch), R, S, lib.ptr(noise), float(x["noise_std"]), float(x["near_mask"]),
             int(white), lib.ptr(g[0]), lib.ptr(g[1]), lib.ptr(g[2]), lib.ptr(draw), lib.ptr(drays), *args, ops._stream())
    out.update(d_raw=draw.view(R, S, 4), drays=drays)
    return out


@pytest.mark.parametrize("run", RC.COMP_RUNS, ids=RC.comp_id)
def test_compositing_backward_side_duties(run):
    R, S, train, white = run
    rep = Report("composite " + RC.comp_id(run))
    ref = RC.comp_oracle(run, F64)
    yard = RC.comp_errors(RC.comp_oracle(run, F32), ref)
    a = _composite_bwd(run, True, 1)
    for k, e in RC.comp_errors(dict(d_raw=a["d_raw"], d_rays_d=a["drays"][:, 3:6]), ref).items():
        rep.gated(k, e, "comp_bwd", yard[k])
    # block_max: the maximum of |d_raw| over the rays each workgroup walked
    blocks = a["blocks"]
    assert blocks == min(-(-R // 4), 2048)
    ray_max = a["d_raw"].abs().reshape(R, -1).amax(1).cpu().numpy()
    want = np.zeros(blocks, np.float32)
    np.maximum.at(want, (np.arange(R) // 4) % blocks, ray_max)
    bmax = a["block_max"].cpu().numpy()
    rep.exact("block_max[b] = max|d_raw| over workgroup b's rays", bool(np.array_equal(want.view(np.int32), bmax.view(np.int32))))
    rep.exact("max(block_max) = max|d_raw|", float(bmax.max()) == float(a["d_raw"].abs().max()) and float(bmax.max()) > 0)
    zb = a["zero_buf"]
    rep.exact("zero_buf is all zero", not bool(bits(zb[:RC.COMP_ZERO_N]).any()))
    rep.exact("the buffer behind zero_buf keeps its NaN", bool(torch.isnan(zb[RC.COMP_ZERO_N:]).all()))
    # init_drays = 1: the whole row is written, zeros outside columns 3..5
    d1 = a["drays"]
    rep.exact("init_drays = 1: columns 0..2 and 6..10 are zero", not bool(bits(d1[:, [0, 1, 2, 6, 7, 8, 9, 10]]).any()) and bool(torch.isfinite(d1).all()))
    # init_drays = 0: columns 3..5 are added to, the others untouched
    b = _composite_bwd(run, True, 0)
    rep.exact("init_drays = 0: columns 3..5 = 7.0 + the gradient", same_bits(b["drays"][:, 3:6], 7.0 + d1[:, 3:6]))
    rep.exact("init_drays = 0: the other eight columns still hold 7.0", bool((b["drays"][:, [0, 1, 2, 6, 7, 8, 9, 10]] == 7.0).all()))
    rep.exact("init_drays = 0: the same d_raw bits", same_bits(b["d_raw"], a["d_raw"]))
    # without the side duties
    c = _composite_bwd(run, False, 0)
    rep.exact("NULL, NULL, 0, 0: the same d_raw bits", same_bits(c["d_raw"], a["d_raw"]))
    rep.gated("NULL, NULL, 0, 0: d_rays_d added to zeroed drays", RC.colerr(c["drays"][:, 3:6], ref["d_rays_d"], 3), "comp_bwd", yard["d_rays_d"])
    print(f"RAYK composite {RC.comp_id(run)} NULL, NULL, 0, 0: d_rays_d entries whose bits differ from the init_drays = 1 run's: "
          f"{int((bits(c['drays'][:, 3:6]) != bits(d1[:, 3:6])).sum())} of {3 * R}")
    rep.done()


# ------------------------------------------------------------------------------------------ (c) the loss scale
def test_loss_scale_kernel_against_frexp():
    from lush_nerf_amd import lib, ops
    cases = RC.scale_cases()
    out = torch.full((len(cases), 2), float("nan"), device=dev())
    keep = []
    for i, (tag, n, a, mx) in enumerate(cases):
        keep.append(gpu(a))
        lib.call("lush_loss_scale", lib.ptr(keep[-1]), n, lib.ptr(out[i]), ops._stream())
    got = out.cpu().numpy()
    bad = []
    for (tag, n, a, mx), (sc, inv) in zip(cases, got):
        want = RC.scale_expected(mx)
        if want is not None:
            ok = bool(np.float32(sc).view(np.int32) == want[0].view(np.int32) and np.float32(inv).view(np.int32) == want[1].view(np.int32))
            print(f"RAYK scale {tag}: {{{sc:.6e}, {inv:.6e}}} want {{{want[0]:.6e}, {want[1]:.6e}}}: {'exact' if ok else 'DIFFERS'}")
        else:
            ok = RC.scale_small_ok(mx, sc, inv)
            print(f"RAYK scale {tag}: {{{sc:.6e}, {inv:.6e}}} max x scale = {float(mx) * float(sc):.4g}: "
                  f"{'finite power of two, normal exact reciprocal' if ok else 'BROKEN'}")
        if not ok:
            bad.append((tag, float(sc), float(inv)))
    assert not bad, bad


def _nerf_tensors(seed, prefix, D):
    p = util.params(seed)
    return [gpu(p[k]) for k in RC.nerf_tensor_names(prefix, D)]


@pytest.mark.parametrize("net,prefix,D,R,S", RC.MLP_LAUNCHES, ids=[f"{m[1]}-{m[3]}x{m[4]}" for m in RC.MLP_LAUNCHES])
def test_mlp_backward_is_homogeneous_in_d_raw(net, prefix, D, R, S):
    """grad_scale_kernel through ops.mlp_backward in mode (h,h) (the noise net then runs as (2,h): ops.Precision.noise): d_raw x 2^k
    moves the loss scale by 2^-k, the fp16 chain sees the same numbers, d(point) comes back x 2^k exactly."""
    from lush_nerf_amd import ops
    rep = Report(f"homogeneous {prefix} ({R},{S})")
    pr = ops.Precision(H16, H16)
    pr = pr.noise() if net == ops.NET_NOISE else pr
    pf, pb = pr.fwd, pr.bwd
    batch_np, z_np, draw_np = RC.mlp_inputs(net, R, S)
    tens = _nerf_tensors(41, prefix, D)
    batch, z = gpu(batch_np), gpu(z_np)
    raw, stash = ops.mlp_forward(net, pf, tens, ops.mlp_pack(net, pf, tens), batch, z, True, ops.stash_code(pf, pb))
    pkb = ops.mlp_pack(net, pb, tens)

    def backward(draw):
        grads, dpts = ops.mlp_backward(net, ops.stash_code(pf, pb), pb, tens, pkb, batch, z, gpu(draw), stash)
        torch.cuda.synchronize()
        return grads, dpts
    g0, d0 = backward(draw_np)
    assert bool(torch.isfinite(d0).all()) and float(d0.abs().max()) > 0 and all(bool(torch.isfinite(g).all()) for g in g0)
    rep.exact("the pad columns 3 and 7 of d(point) are zero", not bool(bits(d0[:, [3, 7]]).any()))
    g0b, d0b = backward(draw_np)      # a second call: the work words the first one re-armed
    rep.exact("a second backward gives the same d(point) bits", same_bits(d0, d0b))
    for k in RC.SCALE_KS:
        gk, dk = backward((draw_np.astype(np.float64) * 2.0 ** k).astype(np.float32))
        diff = int((dk.double() != d0.double() * 2.0 ** k).sum())
        print(f"RAYK homogeneous {prefix} ({R},{S}) k={k}: d(point) entries that are not 2^k x the base run's: {diff} of {dk.numel()}")
        if diff:
            rep.bad.append((f"k={k} d(point)", diff))
        worst = max(util.relerr(a.double() * 2.0 ** -k, b) for a, b in zip(gk, g0) if bool(b.any()))
        rep.bound(f"k={k} weight gradients / 2^k against the base run's", worst, RC.SUM_GATE)
    with np.errstate(under="ignore"):
        tiny = (draw_np.astype(np.float64) * 2.0 ** RC.SCALE_K_TINY).astype(np.float32)
    assert 0 < float(np.abs(tiny).max()) < 2.0 ** -124
    gt, dt = backward(tiny)
    rep.exact(f"k={RC.SCALE_K_TINY}: every gradient is finite", bool(torch.isfinite(dt).all()) and all(bool(torch.isfinite(g).all()) for g in gt))
    rep.done()


# ------------------------------------------------------------------------------------------ (d) the image tail
def _tail_gpu(N, M1, gamma):
    from lush_nerf_amd import lib, ops
    i = RC.tail_inputs(N, M1)
    g3, out = [gpu(a) for a in i["g3"]], {}
    for tag, xa, g in (("wsum3", i["x"], g3[0]), ("wsum1", i["x1"], gpu(i["g1"]))):
        x, ccw = gpu(xa, True), gpu(i["ccw"], True)
        y = ops.WSum.apply(x, ccw)
        (y * g).sum().backward()
        out.update({tag + ".y": y.detach(), tag + ".dx": x.grad, tag + ".dccw": ccw.grad})
    for tag, with_n in (("tm", False), ("tmn", True)):
        x, n = gpu(i["pure"], True), gpu(i["nraw"], True)
        y = ops.ToneMap.apply(x, n if with_n else None, gamma)
        (y * g3[1]).sum().backward()
        out.update({tag + ".y": y.detach(), tag + ".dx": x.grad})
        if with_n:
            out[tag + ".dn"] = n.grad
    n = gpu(i["nraw"], True)
    y = ops.NoiseAct.apply(n)
    (y * g3[2]).sum().backward()
    out.update({"na.y": y.detach(), "na.dx": n.grad})
    for tag, used in (("bm", range(5)), ("bm2", (0, 1))):
        x, x0, ccw, n = gpu(i["x"], True), gpu(i["x0"], True), gpu(i["ccw"], True), gpu(i["nraw"], True)
        res = ops.BlurMix.apply(x, x0, ccw, n, gamma)
        sum((res[k] * g3[k]).sum() for k in used).backward()
        if tag == "bm":
            out.update({f"bm.{nm}": r.detach() for nm, r in zip(RC.BM_OUT, res)})
        out.update({tag + ".d_rgb": x.grad, tag + ".d_rgb0": x0.grad, tag + ".d_ccw": ccw.grad, tag + ".d_nraw": n.grad})
        # the kernel's own [N,4] rows of d(noise_raw): column 3 is the zero the noise MLP's backward reads as d(sigma)
        d4 = torch.full((N, 4), float("nan"), device=dev())
        dr, dr0, dc = torch.empty_like(x), torch.empty_like(x0), torch.empty_like(ccw)
        gs = [g3[k] if k in used else None for k in range(5)]
        lib.call("lush_blur_mix_bwd", lib.ptr(x.detach()), lib.ptr(x0.detach()), lib.ptr(ccw.detach()), lib.ptr(n.detach()), 3, N, M1, int(gamma),
                 *(lib.ptr(t) for t in gs), lib.ptr(dr), lib.ptr(dr0), lib.ptr(dc), lib.ptr(d4), ops._stream())
        out[tag + ".d_nraw4"] = d4
    return out


@pytest.mark.parametrize("N,M1,gamma", RC.TAIL_RUNS)
def test_image_tail_against_float64(N, M1, gamma):
    rep = Report(f"tail N={N} M1={M1} gamma={int(gamma)}")
    ref = RC.tail_oracle(N, M1, gamma, F64)
    yard = RC.tail_errors(RC.tail_oracle(N, M1, gamma, F32), ref, M1)
    got = _tail_gpu(N, M1, gamma)
    for k, e in RC.tail_errors(got, ref, M1).items():
        rep.gated(k, e, RC.tail_columns(k, M1)[0], yard[k])
    for tag in ("bm", "bm2"):
        d4 = got[tag + ".d_nraw4"]
        rep.exact(f"{tag}.d_nraw column 3 is zero", not bool(bits(d4[:, 3]).any()))
        rep.exact(f"{tag}.d_nraw columns 0..2 are the op's gradient", same_bits(d4[:, :3], got[tag + ".d_nraw"]))
    rep.done()


@pytest.mark.parametrize("N,same,scale", RC.LOSS_RUNS)
def test_train_loss_grads_against_float64(N, same, scale):
    from lush_nerf_amd import ops
    rep = Report(f"loss N={N} same={int(same)} scale={scale}")
    a_np, b_np, tg_np, hits = RC.loss_inputs(N)
    ref, o32 = RC.loss_oracle(N, same, scale, F64), RC.loss_oracle(N, same, scale, F32)
    a, b, tg = gpu(a_np), gpu(b_np), gpu(tg_np)
    if same:
        b = a
    work = torch.zeros(2, dtype=torch.float32, device=dev())
    for tag, w in (("work=None", None), ("work, first call", work), ("work, second call", work)):
        loss, ga, gb = ops.train_loss_grads(a, b, tg, scale, w)
        rep.gated(f"{tag} loss", RC.colerr(loss.reshape(1), ref["loss"]), "tail_fwd", RC.colerr(o32["loss"], ref["loss"]))
        rep.gated(f"{tag} d a", RC.colerr(ga, ref["ga"], 3), "tail_bwd", RC.colerr(o32["ga"], ref["ga"], 3))
        if same:
            assert gb is None
        else:
            rep.gated(f"{tag} d b", RC.colerr(gb, ref["gb"], 3), "tail_bwd", RC.colerr(o32["gb"], ref["gb"], 3))
        if hits:
            rep.exact(f"{tag} d a is zero where a equals the target", not bool(ga[gpu(a_np == tg_np)].any()))
        if w is not None:
            rep.exact(f"{tag} leaves the work words zero", not bool(bits(work).any()))
    rep.done()


@pytest.mark.parametrize("V,ns", RC.CONSIST_RUNS)
def test_consistency_loss_against_float64(V, ns):
    from lush_nerf_amd import ops
    rep = Report(f"consist V={V} ns={ns}")
    rgb, cert = RC.consist_inputs(V, ns)
    ref, o32 = RC.consist_oracle(V, ns, F64), RC.consist_oracle(V, ns, F32)
    rg = gpu(rgb, True)
    loss = ops.ConsistLoss.apply(rg, gpu(cert), RC.CONSIST_THR)
    loss.backward()
    rep.gated("loss", RC.colerr(loss.reshape(1), ref["loss"]), "tail_fwd", RC.colerr(o32["loss"], ref["loss"]))
    rep.gated("d rgb", RC.colerr(rg.grad, ref["grad"], 3), "tail_bwd", RC.colerr(o32["grad"], ref["grad"], 3))
    rep.exact("no gradient in the column without a view above the threshold", not bool(rg.grad[:, RC.CONSIST_NONE].any()))
    rep.exact("no gradient in the column with one view above the threshold", not bool(rg.grad[:, RC.CONSIST_ONE].any()))
    rep.done()
