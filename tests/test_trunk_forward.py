"""The training march whose final pass computes colour on live points only (include/lush_live_fwd.h, DESIGN.md sections 1
and 4): the trunk-only instantiation of mlp_wide_fwd_kernel, the forward's list, the live forward's raw output, and the two forms
of lush_march_bwd (on the forward's list with LUSH_MARCH_FWD_LIST_KEPT, on its own list without) against each other and against
the dense march (LUSH_VARIANT_DENSE_BWD).  The gradient gates are test_live_point_march_equals_the_dense_march's: L2 of all the
gradients < 1e-5, worst tensor < 2e-3 of its largest entry -- the forms sum the same products in other orders."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2_GATE, WORST_GATE = 1e-5, 2e-3
NAMES = [f"mlp_fine.pts_linears.{l}.{s}" for l in range(8) for s in ("weight", "bias")] + \
        [f"mlp_fine.{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]
ALPHA_BIAS = NAMES.index("mlp_fine.alpha_linear.bias")


# ----------------------------------------------------------------------------- CPU: the contract headers
def test_the_new_header_parses_and_binds():
    from lush_nerf_amd import abi, lib
    text = open(os.path.join(ROOT, "include", "lush_live_fwd.h")).read()
    a = abi.parse(text, "lush_live_fwd.h")
    assert sorted(a.protos) == sorted(["lush_march_trunk_form", "lush_mlp_fwd_trunk", "lush_live_list", "lush_mlp_fwd_live_raw", "lush_live_gather"])
    assert lib.EXPORTS_LIVE_FWD == list(a.protos) and not a.structs
    assert a.consts == {"LUSH_MARCH_FWD_LIST_KEPT": 65536, "LUSH_LIVE_LIST_COUNT_WORD": 8}
    # the permission bit selects no kernel, and the list's length lies behind the four LIVE_COUNTS words inside the 256-byte block
    assert lib.MARCH_FWD_LIST_KEPT & lib.VARIANT_KERNEL_BITS == 0 and 4 <= lib.LIVE_LIST_COUNT_WORD and (lib.LIVE_LIST_COUNT_WORD + 2) * 4 <= 256
    assert all(res is C.c_int for _, res in a.protos.values())
    # lush_march.h stays what it was
    m = abi.parse(open(os.path.join(ROOT, "include", "lush_march.h")).read())
    assert (len(m.protos), len(m.structs), len(m.consts)) == (67, 9, 29)
    assert lib.HEADERS[-1].endswith("lush_march.h") and lib.HEADERS[-2].endswith("lush_subframe.h") and lib.HEADERS[-3].endswith("lush_live_fwd.h")


def test_the_headline_workspace_is_the_parents():
    """The trunk form lives in the live-point march's workspace as it was: 24 666 312 704 bytes for the headline configuration (20 480
    rays, 64 + 64 samples, mode h,h, two nets), the figure lush_march_workspace_bytes of the parent commit's library returns; the
    list's length takes two spare words of the 256-byte count block.  And the predicate: the headline mode, no other."""
    from lush_nerf_amd import lib
    L = lib.load()
    cfg = lambda pf, pb, var=0, ni=64: lib.MarchCfgC(20480, 64, ni, 1.0, 1.0, 0, 0, -1.0, pf, pb, var, 0)
    h = lib.PLANES_F16
    assert L.lush_march_workspace_bytes(C.byref(cfg(h, h))) == PARENT_HEADLINE_WORKSPACE
    assert L.lush_march_workspace_bytes(C.byref(cfg(h, h, lib.MARCH_FWD_LIST_KEPT))) == PARENT_HEADLINE_WORKSPACE
    assert L.lush_march_trunk_form(C.byref(cfg(h, h))) == 1 and L.lush_march_trunk_form(C.byref(cfg(h, h, ni=0))) == 1
    assert L.lush_march_trunk_form(C.byref(cfg(h, h, lib.MARCH_FWD_LIST_KEPT))) == 1
    for pf, pb, var in ((h, 0, 0), (2, 2, 0), (2, h, 0), (3, 3, 0), (h, h, lib.VARIANT_DENSE_BWD), (h, h, lib.VARIANT_FWD_HALF),
                        (h, h, lib.VARIANT_FWD_512), (h, h, lib.VARIANT_PE_ROWS), (h, h, lib.VARIANT_DW_WALK)):
        assert L.lush_march_trunk_form(C.byref(cfg(pf, pb, var))) == 0, (pf, pb, var)


PARENT_HEADLINE_WORKSPACE = 24666312704      # from a build of the parent commit's sources, not from the code under test


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def diag():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the HIP path has no CPU fallback")
    from lush_nerf_amd import lib
    lib.load()
    from tests import gpu_diag
    return gpu_diag


def _points(R, S, trained_like=False, alpha_bias=None, seed=3):
    """(parameter tensors of one NeRF net, packed fp16 fragments, packed ray batch [R, 11], z [R, S])"""
    from lush_nerf_amd import ops, synth
    from oracle import lush_oracle as O       # (test infrastructure: ray packing of the synthetic batch only)
    dev = torch.device("cuda:0")
    w = synth.all_weights(30, seed, trained_like=trained_like)
    tens = [torch.from_numpy(w[n].copy()).to(dev) for n in NAMES]
    if alpha_bias is not None:
        tens[ALPHA_BIAS].fill_(alpha_bias)
    b = synth.ray_batch(R, 5)
    batch = O.pack_rays(synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, torch.from_numpy(b["rays"])).to(dev)
    z = torch.sort(torch.rand(R, S, generator=torch.Generator().manual_seed(11)), -1)[0].to(dev)
    return tens, ops.mlp_pack(0, ops.PLANES_F16, tens), batch, z


# 7 x 128: a ragged single tile; 520 x 128 = 66 560 points = 260 tiles on 256 workgroups: four workgroups run a second tile (the
# stream jump over the feature layer, the wrap behind the alpha head and the tile-boundary wait counts); 523 x 88: ragged, several tiles
@pytest.mark.gpu
@pytest.mark.parametrize("trained_like", [False, True])
@pytest.mark.parametrize("R,S", [(7, 128), (520, 128), (523, 88)])
def test_trunk_kernel_sigma_is_the_full_kernels(diag, R, S, trained_like):
    from lush_nerf_amd import ops
    tens, pk, batch, z = _points(R, S, trained_like)
    full, _ = ops.mlp_forward(0, ops.PLANES_F16, tens, pk, batch, z, False)
    trunk = ops.mlp_forward_trunk(ops.PLANES_F16, pk, batch, z)
    torch.cuda.synchronize()
    assert torch.isfinite(full).all() and float(full[:, 3].abs().max()) > 0
    assert torch.equal(trunk[:, 3], full[:, 3])
    assert bool((trunk[:, :3] == 0).all())


def _torch_list(raw, z, noise, noise_std, near_mask):
    R, S = z.shape
    pre = raw[:, 3].view(R, S)[:, :-1]
    if noise is not None and noise_std > 0:
        pre = pre + noise * noise_std
    live = pre > 0
    if near_mask >= 0:
        live = live & (z[:, 1:] > near_mask)
    live = torch.cat([live, torch.ones(R, 1, dtype=torch.bool, device=z.device)], 1)
    idx = live.reshape(-1).nonzero().reshape(-1).to(torch.int32)
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device=z.device), live.sum(1).cumsum(0)]).to(torch.int32)
    return idx, start


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["noise-1", "all-live", "last-sample-only", "near-mask"])
def test_forward_list_is_the_compositing_predicate(diag, case):
    """The list against the predicate in torch on the same raw and noise; then the live forward on that list: the rows it writes
    are the full kernel's bit for bit, the rows it leaves keep the trunk-only pass's (0, 0, 0, sigma)."""
    from lush_nerf_amd import ops
    R, S = 523, 88
    kw = {"noise-1": dict(std=1.0), "all-live": dict(std=0.0, alpha_bias=5.0), "last-sample-only": dict(std=0.0, alpha_bias=-50.0),
          "near-mask": dict(std=1.0, near_mask=0.4)}[case]
    tens, pk, batch, z = _points(R, S, alpha_bias=kw.get("alpha_bias"))
    std, near_mask = kw["std"], kw.get("near_mask", -1.0)
    noise = torch.randn(R, S - 1, generator=torch.Generator().manual_seed(5)).to(z.device) if std > 0 else None
    full, _ = ops.mlp_forward(0, ops.PLANES_F16, tens, pk, batch, z, False)
    raw = ops.mlp_forward_trunk(ops.PLANES_F16, pk, batch, z)
    lidx, ray_start, cnt = ops.live_list(raw, z, noise, std, near_mask)
    idx, start = _torch_list(raw, z, noise, std, near_mask)
    n = int(cnt[0])
    assert int(cnt[1]) == R * S and n == idx.numel()
    assert torch.equal(lidx[:n], idx) and torch.equal(ray_start, start)
    last = torch.arange(R, device=z.device, dtype=torch.int32) * S + (S - 1)
    assert bool(torch.isin(last, lidx[:n]).all())                      # the last sample of every ray is always listed
    if case == "all-live":
        assert n == R * S
    elif case == "last-sample-only":
        assert n == R and torch.equal(lidx[:n], last)
    else:
        assert R < n < R * S
    ops.mlp_forward_live(0, ops.PLANES_F16, tens, pk, batch, z, lidx, cnt, ops.PLANES_F16, raw=raw)
    torch.cuda.synchronize()
    listed = torch.zeros(R * S, dtype=torch.bool, device=z.device)
    listed[idx.long()] = True
    assert torch.equal(raw[listed], full[listed])
    assert torch.equal(raw[~listed][:, 3], full[~listed][:, 3]) and bool((raw[~listed][:, :3] == 0).all())
    # the rows of the forward's list in list order, zero rows behind them, the count of the non-zero ones
    draw = torch.randn(R * S, 4, generator=torch.Generator().manual_seed(6)).to(z.device)
    draw[idx[::3].long()] = 0
    draw_c, gcnt = ops.live_gather(draw, R, S, lidx, cnt)
    assert torch.equal(draw_c[:n], draw[idx.long()]) and bool((draw_c[n:] == 0).all())
    assert [int(x) for x in gcnt] == [int((draw[idx.long()] != 0).any(1).sum()), R * S]


# ----------------------------------------------------------------------------- the march, form against form
CASES = {"default-init": dict(n=96), "default-init-large": dict(n=1536), "ragged": dict(n=7), "ragged-samples": dict(n=21, ns=48, ni=40),
         "all-live": dict(n=48, alpha_bias=5.0, noise=0.), "all-dead": dict(n=48, zero_upstream=True), "sharp": dict(n=48, sharp=True)}
_RUNS = {}


def _run(diag, case, form):
    """(outputs, gradients, live counts) of one training step in mode h,h: form 'kept' (the first backward works on the forward's
    list), 'own' (lush_march_bwd without the bit) or 'dense'.  Each (case, form) runs once per session."""
    if (case, form) not in _RUNS:
        from lush_nerf_amd import lib, ops
        from tests.test_gpu_parity import _march_grads
        ops.March.fwd_list_kept = form == "kept"
        try:
            _RUNS[(case, form)] = _march_grads(diag, lib.VARIANT_DENSE_BWD if form == "dense" else 0, **CASES[case])
        finally:
            ops.March.fwd_list_kept = True
    return _RUNS[(case, form)]


def _grads_agree(case, g_a, g_b, what):
    num = den = worst = 0.0
    wk = ""
    for k, a in g_a.items():
        b = g_b[k]
        assert (a is None) == (b is None), k
        if a is None:
            continue
        assert torch.isfinite(a).all(), k
        if case == "all-dead":
            assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0, k
            continue
        e = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        if e > worst:
            worst, wk = e, k
        num += float((a.double() - b.double()).pow(2).sum())
        den += float(b.double().pow(2).sum())
    if case != "all-dead":
        l2 = (num / den) ** 0.5
        print(f"{what} [{case}]: L2 {l2:.1e}, worst tensor {wk} {worst:.1e}")
        assert l2 < L2_GATE and worst < WORST_GATE, (what, l2, wk, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_trunk_form_equals_the_dense_march(diag, case):
    out_k, g_k, cnt = _run(diag, case, "kept")
    out_d, g_d, cnt_d = _run(diag, case, "dense")
    assert cnt_d == [0, 0, 0, 0]
    assert all(torch.equal(a, b) for a, b in zip(out_k, out_d))
    kw = CASES[case]
    assert cnt[1] == kw["n"] * 5 * (kw.get("ns", 64) + kw.get("ni", 64)) and cnt[3] == kw["n"] * 5 * kw.get("ns", 64), cnt
    _grads_agree(case, g_k, g_d, "trunk form against the dense march")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_backward_on_the_forwards_list_equals_the_backward_on_its_own(diag, case):
    out_k, g_k, cnt_k = _run(diag, case, "kept")
    out_o, g_o, cnt_o = _run(diag, case, "own")
    assert all(torch.equal(a, b) for a, b in zip(out_k, out_o))
    assert cnt_k == cnt_o, (cnt_k, cnt_o)                       # LIVE_COUNTS: rows whose d_raw is non-zero, whichever list was chained
    share = (cnt_k[0] + cnt_k[2]) / max(cnt_k[1] + cnt_k[3], 1)
    if case == "all-dead":
        assert share == 0.0, share
    elif case == "all-live":
        assert share > 0.999, share
    _grads_agree(case, g_k, g_o, "forward's list against the backward's own")
    _grads_agree(case, g_o, g_k, "the backward's own list against the forward's")


@pytest.mark.gpu
def test_second_backward_does_not_carry_the_bit(diag, monkeypatch):
    """A retained graph backpropagated twice: the same gradients both times; the first lush_march_bwd of a node carries
    LUSH_MARCH_FWD_LIST_KEPT, the second does not (the first one's coarse pass re-used the stash region)."""
    from lush_nerf_amd import lib, ops
    dev = torch.device("cuda:0")
    n, seed = 48, 17
    net = diag._nerf_all(64, seed, sharp=False, precision=ops.Precision(*ops.parse_planes("h,h"), 0), rbk_scale=2.0e4)
    b = diag.batch_of(n, seed)
    draws = {k: v.to(dev) for k, v in diag.util.tdraws(n * 5, 64, 64, seed).items()}
    seen = []
    call = lib.call

    def spy(name, *args):
        if name == "lush_march_bwd":
            seen.append(bool(args[0]._obj.variant & lib.MARCH_FWD_LIST_KEPT))
        return call(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    out = net(diag.H, diag.W, [[diag.F, 0, diag.W / 2], [0, diag.F, diag.H / 2], [0, 0, 1]], chunk=1 << 20, rays=diag.gpu(b["rays"]),
              rays_info={"images_idx": diag.gpu(b["images_idx"])}, retraw=True, force_naive=False, allkernel=True,
              kernel_pixel=diag.gpu(b["fq_mask"]), perturb=1., N_importance=64, N_samples=64, use_viewdirs=True, white_bkgd=False,
              raw_noise_std=1., inference=False, near=0., far=1., draws=draws)
    loss = ops.TrainLoss.apply(out[0], out[1], diag.gpu(b["target"]))
    mlps = {k: v for k, v in net.named_parameters() if k.startswith(("mlp_fine.", "mlp_coarse."))}
    loss.backward(retain_graph=True)
    first = {k: v.grad.clone() for k, v in mlps.items()}
    n_first = len(seen)
    for v in mlps.values():
        v.grad = None
    loss.backward()
    second = {k: v.grad.clone() for k, v in mlps.items()}
    assert n_first >= 1 and len(seen) == 2 * n_first and all(seen[:n_first]) and not any(seen[n_first:]), seen
    assert net.read_faults() == 0
    _grads_agree("retained", second, first, "second backward against the first")


@pytest.mark.gpu
def test_c_abi_alone_twice_on_one_workspace(diag):
    """lush_march_fwd then lush_march_bwd with variant = 0 (no permission bit: what a plain C caller passes), twice on one workspace:
    both give the gradients of the dense form."""
    from lush_nerf_amd import lib, synth
    L = lib.load()
    dev = torch.device("cuda:0")
    n, Ns, Ni, seed = 96, 64, 64, 3
    w = synth.all_weights(30, seed)
    names = lambda net: [k.replace("mlp_fine", net) for k in NAMES]
    coarse = [torch.from_numpy(w[k].copy()).to(dev) for k in names("mlp_coarse")]
    fine = [torch.from_numpy(w[k].copy()).to(dev) for k in names("mlp_fine")]
    rays = torch.from_numpy(synth.ray_batch(n, seed, 30)["rays"]).to(dev).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W, F = synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF
    cx = float(torch.tensor(-1. / (W / (2. * F)), dtype=torch.float32))
    cy = float(torch.tensor(-1. / (H / (2. * F)), dtype=torch.float32))
    batch = torch.empty(n, 11, device=dev)
    lib.call("lush_pack_rays_fwd", lib.ptr(rays), n, 1, cx, cy, 0.0, 1.0, lib.ptr(batch), stream)
    d = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in synth.draws(n, Ns, Ni, seed).items()}
    up = torch.randn(n, 3, generator=torch.Generator().manual_seed(9)).to(dev)

    def march(variant, times):
        cfg = lib.MarchCfgC(n, Ns, Ni, 1.0, 1.0, 0, 0, -1.0, lib.PLANES_F16, lib.PLANES_F16, variant, 0)
        ws = torch.empty(L.lush_march_workspace_bytes(C.byref(cfg)), dtype=torch.uint8, device=dev)
        f = lambda *s: torch.empty(*s, device=dev)
        o = dict(rgb=f(n, 3), depth=f(n), acc=f(n), density=f(n, Ns + Ni - 1), rgb0=f(n, 3), depth0=f(n), acc0=f(n), density0=f(n, Ns - 1), z_std=f(n))
        out = lib.MarchOut(*(o[k].data_ptr() for k in ("rgb", "depth", "acc", "density", "rgb0", "depth0", "acc0", "density0", "z_std")))
        dr = lib.MarchDraws(*(d[k].data_ptr() for k in ("t_rand", "noise_c", "u", "noise_f")))
        pc, pfn = lib.mlp_struct(coarse, 8), lib.mlp_struct(fine, 8)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        lib.call("lush_march_fwd", C.byref(cfg), lib.ptr(batch), C.byref(pc), C.byref(pfn), C.byref(dr), C.byref(out), lib.ptr(ws), lib.ptr(flags), stream)
        assert int(flags.item()) == 0
        res = []
        for _ in range(times):
            gc, gf = [torch.zeros_like(t) for t in coarse], [torch.zeros_like(t) for t in fine]
            go = lib.MarchGout(up.data_ptr(), None, None, up.data_ptr(), None, None)
            drays = torch.full((n, 11), float("nan"), device=dev)
            sgc, sgf = lib.mlp_struct(gc, 8), lib.mlp_struct(gf, 8)
            lib.call("lush_march_bwd", C.byref(cfg), lib.ptr(batch), C.byref(pc), C.byref(pfn), C.byref(dr), C.byref(go), lib.ptr(ws),
                     C.byref(sgc), C.byref(sgf), lib.ptr(drays), stream)
            torch.cuda.synchronize()
            res.append({**{f"c{i}": t for i, t in enumerate(gc)}, **{f"f{i}": t for i, t in enumerate(gf)}, "d rays": drays})
        return o, res
    o_t, (first, second) = march(0, 2)
    o_d, (dense,) = march(lib.VARIANT_DENSE_BWD, 1)
    assert all(torch.equal(o_t[k], o_d[k]) for k in o_t)
    _grads_agree("c-abi", first, dense, "C ABI, first lush_march_bwd against the dense form")
    _grads_agree("c-abi", second, dense, "C ABI, second lush_march_bwd on the same workspace against the dense form")


@pytest.mark.gpu
def test_captured_step_in_the_trunk_form_replays_agree():
    """tests/test_dw_queue.py's captured live step, at its size and to its gate: step_graph captures first backwards, so its replays
    run lush_march_bwd on the forward's list; the same steps run eagerly here run it on the backward's own list (no permission bit)."""
    import argparse
    import numpy as np
    from lush_nerf_amd import model as M, ops, synth
    from lush_nerf_amd.trainer import Trainer
    from tests.test_dw_queue import GATE, _rel
    dev = torch.device("cuda:0")

    def make():
        args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                                  N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                                  rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=80)
        net = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4),
                        precision=ops.Precision(*ops.parse_planes("h,h")))
        M.load_reference_weights(net, synth.all_weights(30, 3, sharp=True))
        return Trainer(net.to(dev), synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, 64, 64, lrate=0.0, kernel_start_iter=0, allkernel_start_iter=0)

    n, steps = 2048, 5
    bs = []
    for s in range(steps):
        b = {k: torch.from_numpy(v).to(dev) for k, v in synth.ray_batch(n, 5, 30, step=s).items()}
        b["target"] = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(100 + s))
        bs.append(b)

    def grads(tr):
        return {k: p.grad.detach().cpu().numpy().copy() for k, p in tr.model.named_parameters()
                if k.startswith(("mlp_fine.", "mlp_coarse.")) and p.grad is not None}

    ga, gb = [], []
    ops.March.fwd_list_kept = False
    try:
        torch.manual_seed(1)
        A = make()
        for s, b in enumerate(bs):
            A.step(b, s)
            ga.append(grads(A))
    finally:
        ops.March.fwd_list_kept = True
    torch.manual_seed(1)
    B = make()
    for s, b in enumerate(bs):
        B.step_graph(b, s)
        gb.append(grads(B))
    assert B._graph is not None                                   # the capture happened: steps 3 and 4 are replays
    assert A.live_counts() == B.live_counts()                     # rows whose d_raw is non-zero, whichever list was chained
    worst = 0.0
    for s in (3, 4):
        assert set(ga[s]) == set(gb[s]) and len(ga[s]) >= 48
        for k in ga[s]:
            err = _rel(gb[s][k], ga[s][k])
            worst = max(worst, err)
            assert np.isfinite(gb[s][k]).all() and float(np.abs(ga[s][k]).max()) > 0 and err < GATE, (s, k, err)
    print(f"replays of the captured trunk-form step against eager steps on the backward's own list: NeRF gradients within {worst:.1e}")


@pytest.mark.gpu
def test_piecewise_path_runs_the_same_form(diag):
    """With a kernel-group timer set (bench.py --full) the march runs through the piecewise entry points: the same form -- the fine
    launch over all points trunk-only under mlp_fwd_all, the live forward with stash under mlp_fwd in the forward, chain and weight
    gradients on the forward's list -- with the one-call march's outputs bit for bit and its gradients to the gates."""
    from lush_nerf_amd import ops
    dev = torch.device("cuda:0")
    n, seed = 96, 17

    def run(timer):
        net = diag._nerf_all(64, seed, sharp=False, precision=ops.Precision(*ops.parse_planes("h,h"), 0), rbk_scale=2.0e4)
        if timer:
            net.hooks.timer = ops.KernelTimer()
        b = diag.batch_of(n, seed)
        draws = {k: v.to(dev) for k, v in diag.util.tdraws(n * 5, 64, 64, seed).items()}
        out = net(diag.H, diag.W, [[diag.F, 0, diag.W / 2], [0, diag.F, diag.H / 2], [0, 0, 1]], chunk=1 << 20, rays=diag.gpu(b["rays"]),
                  rays_info={"images_idx": diag.gpu(b["images_idx"])}, retraw=True, force_naive=False, allkernel=True,
                  kernel_pixel=diag.gpu(b["fq_mask"]), perturb=1., N_importance=64, N_samples=64, use_viewdirs=True, white_bkgd=False,
                  raw_noise_std=1., inference=False, near=0., far=1., draws=draws)
        ops.TrainLoss.apply(out[0], out[1], diag.gpu(b["target"])).backward()
        torch.cuda.synchronize()
        assert net.read_faults() == 0
        grads = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
        return [o.detach().clone() for o in (out[0], out[1], out[3], out[5])], grads, (net.hooks.timer.summary() if timer else None)
    out_f, g_f, _ = run(False)
    out_p, g_p, groups = run(True)
    assert all(torch.equal(a, b) for a, b in zip(out_f, out_p))
    assert set(g_f) == set(g_p)
    _grads_agree("piecewise", g_p, g_f, "piecewise path against the one-call march")
    P_c, P_f = n * 5 * 64, n * 5 * 128
    assert groups["mlp_fwd_all"]["launches"] == 2 and groups["mlp_fwd_all"]["points"] == P_c + P_f
    live = groups["mlp_fwd"]["points"]
    assert groups["mlp_fwd"]["launches"] == 2 and 0 < live < P_c + P_f
    # the backward's launches run on the lists the live forwards ran on: the fine pass's is the forward's own
    assert groups["mlp_bwd_chain"]["points"] == live and groups["mlp_bwd_weights"]["points"] == live


_CROSS_INPUTS = {}


def _cross_inputs():
    """7 rays x (64 + 64) samples on the default-init field, noise and perturb on: (coarse tensors, fine tensors, ray batch, draws,
    upstream gradients of rgb, depth, acc, rgb0, depth0, acc0).  Made once per session; nobody writes to them."""
    if not _CROSS_INPUTS:
        from lush_nerf_amd import ops, synth
        dev = torch.device("cuda:0")
        R, S, Ni, seed = 7, 64, 64, 3
        w = synth.all_weights(30, seed)
        names = lambda net: [k.replace("mlp_fine", net) for k in NAMES]
        rays = torch.from_numpy(synth.ray_batch(R, seed, 30)["rays"]).to(dev)
        g = torch.Generator().manual_seed(9)
        _CROSS_INPUTS.update(
            coarse=[torch.from_numpy(w[k].copy()).to(dev) for k in names("mlp_coarse")],
            fine=[torch.from_numpy(w[k].copy()).to(dev) for k in names("mlp_fine")],
            batch=ops.PackRays.apply(rays, synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, True, 0., 1.).detach(),
            draws={k: torch.from_numpy(v).to(dev) for k, v in synth.draws(R, S, Ni, seed).items()},
            up=[torch.randn(*s, generator=g).to(dev) for s in ((R, 3), (R,), (R,), (R, 3), (R,), (R,))])
    return _CROSS_INPUTS


@pytest.mark.gpu
@pytest.mark.parametrize("into", ["both", "main", "coarse"])
@pytest.mark.parametrize("nets", [1, 2])
@pytest.mark.parametrize("planes", ["h,h", "2,h"])
def test_one_call_march_equals_the_piecewise_path_across_forms(diag, planes, nets, into):
    """The one-call march (lush_march_fwd / lush_march_bwd) against the piecewise path, which composes the same kernels on its own
    in ops.March: the backward's fragments of the forward's plane code or of another one (2,h: packed for the backward), one net
    for both passes or two, and output gradients into both passes, the final pass alone or the coarse pass alone.  Outputs bit for
    bit, gradients to the form-against-form gates, and the net of a pass that received no gradient gets None from both.  Written
    against the library as it stood before lush_march_abi.hip was laid out per pass, where all twelve cases passed with the figures
    they have since: identical gradients except with one net and gradients into both passes (L2 4e-08, worst tensor 2e-07)."""
    from lush_nerf_amd import ops
    x = _cross_inputs()
    prec = ops.Precision(*ops.parse_planes(planes))
    main, coarse_out = (0, 1, 2), (7, 8, 9)
    used = {"both": main + coarse_out, "main": main, "coarse": coarse_out}[into]

    def run(timer):
        coarse = [t.clone().requires_grad_(True) for t in x["coarse"]]
        fine = [t.clone().requires_grad_(True) for t in x["fine"]] if nets == 2 else []
        batch = x["batch"].clone().requires_grad_(True)
        cfg = ops.MarchCfg(64, 64, 1., 1., precision=prec, want_grad=True, hooks=ops.Hooks(timer=ops.KernelTimer() if timer else None))
        out = ops.March.apply(batch, cfg, x["draws"], len(coarse), *coarse, *fine)
        up = dict(zip(main + coarse_out, x["up"]))
        sum((out[i] * up[i]).sum() for i in used).backward()
        torch.cuda.synchronize()
        grads = {**{f"c{i}": t.grad for i, t in enumerate(coarse)}, **{f"f{i}": t.grad for i, t in enumerate(fine)}, "d rays": batch.grad}
        return [o.detach().clone() for o in out], grads
    out_f, g_f = run(False)
    out_p, g_p = run(True)
    assert len(out_f) == len(out_p) == 12
    for k, (a, b) in enumerate(zip(out_f, out_p)):
        assert torch.isfinite(a).all() and torch.equal(a, b), k
    # which nets received gradients: with one net every case reaches it; with two, only the pass whose outputs were used
    for g in (g_f, g_p):
        assert g["d rays"] is not None and all(float(t.abs().max()) > 0 for t in g.values() if t is not None)
        assert all((g[f"c{i}"] is None) == (nets == 2 and into == "main") for i in range(len(NAMES)))
        assert nets == 1 or all((g[f"f{i}"] is None) == (into == "coarse") for i in range(len(NAMES)))
    _grads_agree("cross", g_f, g_p, f"one-call march against the piecewise path [{planes}, {nets} net(s), gradients into {into}]")
    _grads_agree("cross", g_p, g_f, f"piecewise path against the one-call march [{planes}, {nets} net(s), gradients into {into}]")
