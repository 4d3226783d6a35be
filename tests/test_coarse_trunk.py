"""The training march whose COARSE pass, too, computes colour on live points only (include/lush_live_coarse.h, DESIGN.md sections
1, 4 and 10): the configuration bit LUSH_MARCH_COARSE_TRUNK gives the coarse pass a stash, a list and per-ray ranges of its own in
the workspace; lush_march_fwd then runs it trunk-only over all its points and in full on the points of non-zero alpha, and
lush_march_bwd works on that list and stash.  Without the bit nothing moves.  The march with the bit against the march without:
outputs bit for bit, gradients to the form-against-form gates of tests/test_trunk_forward.py (L2 of all the gradients < 1e-5,
worst tensor < 2e-3 of its largest entry: the forms sum the same products in other orders)."""
import ctypes as C
import os

import pytest
import torch

from tests.test_trunk_forward import NAMES, PARENT_HEADLINE_WORKSPACE, _grads_agree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = ("VIEW_Z", "VIEW_RAW", "VIEW_WEIGHTS", "VIEW_Z_COARSE", "VIEW_STASH_COARSE", "VIEW_STASH_FINE", "VIEW_LIVE_COUNTS")


def _al256(x):
    return (x + 255) & ~255


def _cfg(pf, pb, var=0, R=20480, S=64, ni=64, same=0, noise=1.0, perturb=1.0):
    from lush_nerf_amd import lib
    return lib.MarchCfgC(R, S, ni, perturb, noise, 0, 0, -1.0, pf, pb, var, same)


def _view(cfg, which):
    """(return code, offset, bytes) of lush_march_view: a view a configuration does not have answers non-zero."""
    from lush_nerf_amd import lib
    off, nb = C.c_size_t(0), C.c_size_t(0)
    rc = lib.load().lush_march_view(C.byref(cfg), getattr(lib, which), C.byref(off), C.byref(nb))
    return (rc, off.value, nb.value) if rc == 0 else (rc, 0, 0)


# ----------------------------------------------------------------------------- CPU: header and layout
def test_the_fourth_header_parses_and_binds():
    from lush_nerf_amd import abi, lib
    a = abi.parse(open(os.path.join(ROOT, "include", "lush_live_coarse.h")).read(), "lush_live_coarse.h")      # the closed typing table
    assert list(a.protos) == ["lush_march_coarse_trunk_form"] == lib.EXPORTS_LIVE_COARSE and not a.structs
    assert a.protos["lush_march_coarse_trunk_form"] == ([C.c_void_p], C.c_int)
    assert a.consts == {"LUSH_MARCH_COARSE_TRUNK": 131072, "LUSH_LIVE_COARSE_LIST_COUNT_WORD": lib.LIVE_COARSE_LIST_COUNT_WORD}
    bit, word = lib.MARCH_COARSE_TRUNK, lib.LIVE_COARSE_LIST_COUNT_WORD
    assert bit == 131072 and bit & lib.VARIANT_KERNEL_BITS == 0 and bit != lib.MARCH_FWD_LIST_KEPT and bit & lib.MARCH_FWD_LIST_KEPT == 0
    # a spare pair of the 256-byte count block: not the four LIVE_COUNTS words, not the final pass's pair
    used = {0, 1, 2, 3, lib.LIVE_LIST_COUNT_WORD, lib.LIVE_LIST_COUNT_WORD + 1}
    assert not {word, word + 1} & used and 0 <= word and (word + 2) * 4 <= 256
    # the last three contract headers keep their places
    assert [os.path.basename(h) for h in lib.HEADERS[-3:]] == ["lush_live_fwd.h", "lush_subframe.h", "lush_march.h"]
    assert os.path.basename(lib.HEADERS[-4]) == "lush_live_coarse.h"
    assert all(hasattr(lib.load(), n) for n in lib.EXPORTS_LIVE_COARSE)


def test_without_the_bit_the_workspace_is_the_parents():
    from lush_nerf_amd import lib
    L, h = lib.load(), lib.PLANES_F16
    for var in (0, lib.MARCH_FWD_LIST_KEPT):
        c = _cfg(h, h, var)
        assert L.lush_march_workspace_bytes(C.byref(c)) == PARENT_HEADLINE_WORKSPACE
        assert L.lush_march_coarse_trunk_form(C.byref(c)) == 0 and L.lush_march_trunk_form(C.byref(c)) == 1
        sc, sf = _view(c, "VIEW_STASH_COARSE"), _view(c, "VIEW_STASH_FINE")
        assert sc[0] == 0 and sf[0] == 0 and sc[1] == sf[1]


@pytest.mark.parametrize("R,S,ni,same", [(20480, 64, 64, 0), (20480, 64, 64, 1), (40960, 64, 64, 0), (523, 44, 44, 0), (7, 64, 64, 0)])
def test_with_the_bit_the_workspace_grows_by_the_three_regions(R, S, ni, same):
    from lush_nerf_amd import lib
    L, h = lib.load(), lib.PLANES_F16
    for kept in (0, lib.MARCH_FWD_LIST_KEPT):
        plain, bit = _cfg(h, h, kept, R, S, ni, same), _cfg(h, h, kept | lib.MARCH_COARSE_TRUNK, R, S, ni, same)
        assert L.lush_march_coarse_trunk_form(C.byref(bit)) == 1 and L.lush_march_trunk_form(C.byref(bit)) == 1
        stash = L.lush_mlp_stash_bytes(0, h, h, C.c_longlong(R * S))
        assert stash > 0
        grown = _al256(stash) + _al256(R * S * 4) + _al256((R + 1) * 4)      # the coarse stash, its list, its per-ray ranges
        assert L.lush_march_workspace_bytes(C.byref(bit)) == L.lush_march_workspace_bytes(C.byref(plain)) + grown
        (rc_c, off_c, n_c), (rc_f, off_f, n_f) = _view(bit, "VIEW_STASH_COARSE"), _view(bit, "VIEW_STASH_FINE")
        assert rc_c == 0 and rc_f == 0 and n_c == stash and n_f == _view(plain, "VIEW_STASH_FINE")[2]
        assert off_c + n_c <= off_f or off_f + n_f <= off_c                    # disjoint
        assert off_c % 256 == 0 and off_c + n_c <= L.lush_march_workspace_bytes(C.byref(bit))
        assert _view(bit, "VIEW_LIVE_COUNTS")[0] == 0


def _not_the_form():
    from lush_nerf_amd import lib
    h = lib.PLANES_F16
    return {"2,2": (dict(pf=2, pb=2), 0), "2,h": (dict(pf=2, pb=h), 0), "DENSE_BWD": (dict(pf=h, pb=h, var=lib.VARIANT_DENSE_BWD), 0),
            "FWD_HALF": (dict(pf=h, pb=h, var=lib.VARIANT_FWD_HALF), 0), "FWD_512": (dict(pf=h, pb=h, var=lib.VARIANT_FWD_512), 0),
            "PE_ROWS": (dict(pf=h, pb=h, var=lib.VARIANT_PE_ROWS), 0), "ni=0": (dict(pf=h, pb=h, ni=0), 1),
            "planes_bwd=0": (dict(pf=h, pb=0), 0)}


@pytest.mark.parametrize("case", ["2,2", "2,h", "DENSE_BWD", "FWD_HALF", "FWD_512", "PE_ROWS", "ni=0", "planes_bwd=0"])
def test_the_bit_is_ignored_where_the_form_does_not_apply(case):
    """Bytes and every view as without the bit; the coarse predicate says 0; lush_march_trunk_form answers as it did."""
    from lush_nerf_amd import lib
    L = lib.load()
    kw, trunk = _not_the_form()[case]
    var = kw.pop("var", 0)
    plain, bit = _cfg(var=var, **kw), _cfg(var=var | lib.MARCH_COARSE_TRUNK, **kw)
    assert L.lush_march_workspace_bytes(C.byref(plain)) > 0
    assert L.lush_march_workspace_bytes(C.byref(bit)) == L.lush_march_workspace_bytes(C.byref(plain))
    for which in VIEWS:
        assert _view(bit, which) == _view(plain, which), which
    assert L.lush_march_coarse_trunk_form(C.byref(bit)) == 0 and L.lush_march_coarse_trunk_form(C.byref(plain)) == 0
    assert L.lush_march_trunk_form(C.byref(bit)) == trunk and L.lush_march_trunk_form(C.byref(plain)) == trunk


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def diag():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the HIP path has no CPU fallback")
    from lush_nerf_amd import lib
    lib.load()
    from tests import gpu_diag
    return gpu_diag


FIELDS = {"default-init": {}, "sharp": dict(sharp=True), "trained-like": dict(trained_like=True)}
OUT_KEYS = ("rgb", "depth", "acc", "density", "rgb0", "depth0", "acc0", "density0", "z_std")
_ABI_RUNS = {}


def _abi_march(R, S, Ni, field, bit, kept=(True, False), noise=1.0, perturb=1.0, same=0, seed=3):
    """lush_march_fwd, then one lush_march_bwd per entry of `kept` (with / without LUSH_MARCH_FWD_LIST_KEPT) on the same workspace,
    through the C ABI alone, in mode h,h: a dict of the outputs, the final pass's weights, the coarse pass's raw rows and weights, and per
    backward the gradients (coarse net, fine net, d rays) and the LIVE_COUNTS words.  Each configuration runs once per session."""
    key = (R, S, Ni, field, bit, kept, noise, perturb, same, seed)
    if key in _ABI_RUNS:
        return _ABI_RUNS[key]
    from lush_nerf_amd import lib, synth
    L = lib.load()
    dev = torch.device("cuda:0")
    w = synth.all_weights(30, seed, **FIELDS[field])
    names = lambda net: [k.replace("mlp_fine", net) for k in NAMES]
    coarse = [torch.from_numpy(w[k].copy()).to(dev) for k in names("mlp_coarse")]
    fine = None if same else [torch.from_numpy(w[k].copy()).to(dev) for k in names("mlp_fine")]
    rays = torch.from_numpy(synth.ray_batch(R, seed, 30)["rays"]).to(dev).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W, F = synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF
    cx = float(torch.tensor(-1. / (W / (2. * F)), dtype=torch.float32))
    cy = float(torch.tensor(-1. / (H / (2. * F)), dtype=torch.float32))
    batch = torch.empty(R, 11, device=dev)
    lib.call("lush_pack_rays_fwd", lib.ptr(rays), R, 1, cx, cy, 0.0, 1.0, lib.ptr(batch), stream)
    d = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in synth.draws(R, S, Ni, seed).items()}
    use = {"t_rand": perturb > 0, "u": perturb > 0, "noise_c": noise > 0, "noise_f": noise > 0}
    dr = lib.MarchDraws(*(d[k].data_ptr() if use[k] else None for k in ("t_rand", "noise_c", "u", "noise_f")))
    g = torch.Generator().manual_seed(9)
    up = [torch.randn(*s, generator=g).to(dev) for s in ((R, 3), (R,), (R,), (R, 3), (R,), (R,))]      # d rgb, depth, acc, rgb0, depth0, acc0
    var = lib.MARCH_COARSE_TRUNK if bit else 0
    mk = lambda v: lib.MarchCfgC(R, S, Ni, perturb, noise, 0, 0, -1.0, lib.PLANES_F16, lib.PLANES_F16, v, same)
    cfg = mk(var)
    assert L.lush_march_coarse_trunk_form(C.byref(cfg)) == (1 if bit else 0)
    ws = torch.empty(L.lush_march_workspace_bytes(C.byref(cfg)), dtype=torch.uint8, device=dev)
    f = lambda *s: torch.empty(*s, device=dev)
    o = dict(rgb=f(R, 3), depth=f(R), acc=f(R), density=f(R, S + Ni - 1), rgb0=f(R, 3), depth0=f(R), acc0=f(R), density0=f(R, S - 1), z_std=f(R))
    out = lib.MarchOut(*(o[k].data_ptr() for k in OUT_KEYS))
    pc = lib.mlp_struct(coarse, 8)
    pfn = pc if same else lib.mlp_struct(fine, 8)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.call("lush_march_fwd", C.byref(cfg), lib.ptr(batch), C.byref(pc), C.byref(pfn), C.byref(dr), C.byref(out), lib.ptr(ws), lib.ptr(flags), stream)
    assert int(flags.item()) == 0

    def region(off, count, shape):
        return ws[off:off + count * 4].view(torch.float32).view(*shape).clone()

    def view(which, shape):
        rc, off, nb = _view(cfg, which)
        assert rc == 0
        return ws[off:off + nb].view(torch.float32).view(*shape).clone()
    res = dict(out=o, weights=view("VIEW_WEIGHTS", (R, S + Ni)), z=view("VIEW_Z", (R, S + Ni)), z_c=view("VIEW_Z_COARSE", (R, S)))
    # the workspace begins, in every form, with the coarse pass's z, weights and raw rows, each rounded up to 256 bytes
    # (csrc/lush_march_abi.hip layout(): zc, wc, rawc)
    zc_off = _view(cfg, "VIEW_Z_COARSE")[1]
    res["weights_c"] = region(zc_off + _al256(R * S * 4), R * S, (R, S))
    res["raw_c"] = region(zc_off + 2 * _al256(R * S * 4), R * S * 4, (R * S, 4))
    res["noise_c"] = d["noise_c"] if noise > 0 else None
    res["grads"], res["counts"] = [], []
    cnt_off = _view(cfg, "VIEW_LIVE_COUNTS")[1]
    for k in kept:
        gc = [torch.zeros_like(t) for t in coarse]
        gf = None if same else [torch.zeros_like(t) for t in fine]
        go = lib.MarchGout(*(t.data_ptr() for t in up))
        drays = torch.full((R, 11), float("nan"), device=dev)
        sgc = lib.mlp_struct(gc, 8)
        sgf = None if same else lib.mlp_struct(gf, 8)
        cb = mk(var | (lib.MARCH_FWD_LIST_KEPT if k else 0))
        lib.call("lush_march_bwd", C.byref(cb), lib.ptr(batch), C.byref(pc), C.byref(pfn), C.byref(dr), C.byref(go), lib.ptr(ws),
                 C.byref(sgc), None if same else C.byref(sgf), lib.ptr(drays), stream)
        torch.cuda.synchronize()
        res["grads"].append({**{f"c{i}": t for i, t in enumerate(gc)}, **({} if same else {f"f{i}": t for i, t in enumerate(gf)}), "d rays": drays})
        res["counts"].append([int(x) for x in ws[cnt_off:cnt_off + 16].view(torch.int32).tolist()])
    _ABI_RUNS[key] = res
    return res


def _bit_against_plain(R, S, Ni, field, **kw):
    """Every comparison the form with the bit owes the form without, on one shape and field."""
    plain = _abi_march(R, S, Ni, field, False, **kw)
    bit = _abi_march(R, S, Ni, field, True, **kw)
    for k in OUT_KEYS:
        assert torch.isfinite(plain["out"][k]).all() and torch.equal(bit["out"][k], plain["out"][k]), k
    for k in ("weights", "z", "z_c", "weights_c"):
        assert torch.equal(bit[k], plain[k]), k
    # the coarse raw rows: sigma complete; colour the other form's on the rows the compositing gives a non-zero alpha (sigma + noise
    # > 0, and the last sample of every ray), exactly 0 elsewhere
    raw_p, raw_b = plain["raw_c"], bit["raw_c"]
    assert torch.equal(raw_b[:, 3], raw_p[:, 3])
    pre = raw_p[:, 3].view(R, S)[:, :-1]
    if plain["noise_c"] is not None:
        pre = pre + plain["noise_c"] * kw.get("noise", 1.0)
    listed = torch.cat([pre > 0, torch.ones(R, 1, dtype=torch.bool, device=pre.device)], 1).reshape(-1)
    assert torch.equal(raw_b[listed], raw_p[listed])
    assert bool((raw_b[~listed][:, :3] == 0).all())
    n_listed = int(listed.sum())
    assert R <= n_listed <= R * S
    # LIVE_COUNTS: the rows whose d_raw is non-zero, whichever list was chained -- both slots, after the backward on the forward's
    # lists and after the second one, which lists for itself
    assert bit["counts"] == plain["counts"], (bit["counts"], plain["counts"])
    cnt = bit["counts"][0]
    assert cnt[1] == R * (S + Ni) and cnt[3] == R * S and 0 < cnt[2] <= n_listed, (cnt, n_listed)
    what = f"{R} x ({S}+{Ni}) {field} {kw}"
    _grads_agree("coarse-trunk", bit["grads"][0], plain["grads"][0], f"with the bit against without, first backward [{what}]")
    _grads_agree("coarse-trunk", bit["grads"][1], plain["grads"][0], f"with the bit, second backward (lists for itself) against without [{what}]")
    _grads_agree("coarse-trunk", bit["grads"][1], bit["grads"][0], f"with the bit, second backward against its first [{what}]")
    return n_listed / (R * S)


# 7 x (64+64): one partial coarse tile of 256 points; 480 x (64+64): 120 coarse / 240 fine tiles; 1 045 x (64+64): 261.25 coarse tiles
# on 256 workgroups -- a second tile per workgroup and a partial last one; 523 x (44+44): rays do not align with the tiles
SHAPES = [(7, 64, 64), (480, 64, 64), (1045, 64, 64), (523, 44, 44)]


@pytest.mark.gpu
@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("R,S,Ni", SHAPES)
def test_march_with_the_bit_equals_the_march_without(diag, R, S, Ni, field):
    share = _bit_against_plain(R, S, Ni, field)
    print(f"{R} x ({S}+{Ni}) {field}: {share:.3f} of the coarse points listed")
    if field == "trained-like":
        assert share < 0.5, share              # most of the volume is dead: the rows the list leaves out are the many


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["default-init", "sharp"])
@pytest.mark.parametrize("kw", [dict(noise=0.0), dict(perturb=0.0), dict(same=1)], ids=["no-noise", "no-perturb", "same-net"])
def test_further_configurations_with_the_bit(diag, kw, field):
    """raw_noise_std = 0 (no noise pointer: the list is sigma > 0), perturb = 0 (no jitter, no u), and one net for both passes (the
    coarse and the fine gradients land in one buffer)."""
    _bit_against_plain(523, 44, 44, field, **kw)
    _bit_against_plain(480, 64, 64, field, **kw)


@pytest.mark.gpu
def test_c_abi_alone_twice_on_one_workspace_with_the_bit(diag):
    """lush_march_fwd with the bit, then lush_march_bwd twice on the same workspace: the first with LUSH_MARCH_FWD_LIST_KEPT (both
    passes on the forward's lists), the second without (both list by d_raw and re-run the live forward; the coarse pass into its own
    region).  Both give the gradients of the form without the bit, and of the dense form."""
    from lush_nerf_amd import lib
    R, S, Ni = 480, 64, 64
    bit = _abi_march(R, S, Ni, "default-init", True)
    plain = _abi_march(R, S, Ni, "default-init", False)
    assert len(bit["grads"]) == 2 and bit["counts"][0] == bit["counts"][1] == plain["counts"][0]
    _grads_agree("c-abi", bit["grads"][0], plain["grads"][0], "first lush_march_bwd (kept) against the form without the bit")
    _grads_agree("c-abi", bit["grads"][1], plain["grads"][0], "second lush_march_bwd (not kept) against the form without the bit")
    assert lib.load().lush_march_coarse_trunk_form(C.byref(_cfg(lib.PLANES_F16, lib.PLANES_F16, lib.MARCH_COARSE_TRUNK, R, S, Ni))) == 1


# ----------------------------------------------------------------------------- through ops.March
_OPS_RUNS = {}


def _ops_run(diag, n, sharp, bit):
    """(outputs, gradients, live counts) of one training step of the model in mode h,h with March.coarse_trunk = bit."""
    if (n, sharp, bit) not in _OPS_RUNS:
        from lush_nerf_amd import ops
        from tests.test_gpu_parity import _march_grads
        ops.March.coarse_trunk = bit
        try:
            _OPS_RUNS[(n, sharp, bit)] = _march_grads(diag, 0, n=n, sharp=sharp)
        finally:
            ops.March.coarse_trunk = True
    return _OPS_RUNS[(n, sharp, bit)]


@pytest.mark.gpu
@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("n", [96, 209])      # 480 and 1 045 marched rays
def test_the_products_march_sets_the_bit(diag, monkeypatch, n, sharp):
    """ops.March asks for the form by default: lush_march_fwd and lush_march_bwd see the same word with the bit; outputs, LIVE_COUNTS and
    gradients against March.coarse_trunk = False."""
    from lush_nerf_amd import lib, ops
    seen = []
    call = lib.call

    def spy(name, *args):
        if name in ("lush_march_fwd", "lush_march_bwd"):
            seen.append((name, int(args[0]._obj.variant)))
        return call(name, *args)
    assert ops.March.coarse_trunk is True
    _OPS_RUNS.pop((n, sharp, True), None)
    monkeypatch.setattr(lib, "call", spy)
    out_b, g_b, cnt_b = _ops_run(diag, n, sharp, True)
    monkeypatch.setattr(lib, "call", call)
    fwd, bwd = ([v for k, v in seen if k == name] for name in ("lush_march_fwd", "lush_march_bwd"))
    assert len(fwd) == len(bwd) >= 1 and all(v & lib.MARCH_COARSE_TRUNK for v in fwd + bwd), seen
    assert not any(v & lib.MARCH_FWD_LIST_KEPT for v in fwd) and all(v & lib.MARCH_FWD_LIST_KEPT for v in bwd), seen
    out_p, g_p, cnt_p = _ops_run(diag, n, sharp, False)
    assert all(torch.equal(a, b) for a, b in zip(out_b, out_p))
    assert cnt_b == cnt_p and cnt_b[3] == n * 5 * 64 and cnt_b[2] > 0, (cnt_b, cnt_p)
    _grads_agree("ops", g_b, g_p, f"ops.March with the bit against without [{n * 5} rays, sharp={sharp}]")


@pytest.mark.gpu
def test_second_backward_with_the_bit_lists_for_itself(diag, monkeypatch):
    """A retained graph backpropagated twice: both lush_march_bwd calls lay the workspace out with the bit, only the first carries
    LUSH_MARCH_FWD_LIST_KEPT; the second one's gradients within the gates of the first."""
    from lush_nerf_amd import lib, ops
    dev = torch.device("cuda:0")
    n, seed = 96, 17
    net = diag._nerf_all(64, seed, sharp=False, precision=ops.Precision(*ops.parse_planes("h,h"), 0), rbk_scale=2.0e4)
    b = diag.batch_of(n, seed)
    draws = {k: v.to(dev) for k, v in diag.util.tdraws(n * 5, 64, 64, seed).items()}
    seen = []
    call = lib.call

    def spy(name, *args):
        if name == "lush_march_bwd":
            seen.append(int(args[0]._obj.variant))
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
    assert n_first >= 1 and len(seen) == 2 * n_first and all(v & lib.MARCH_COARSE_TRUNK for v in seen), seen
    assert all(v & lib.MARCH_FWD_LIST_KEPT for v in seen[:n_first]) and not any(v & lib.MARCH_FWD_LIST_KEPT for v in seen[n_first:]), seen
    assert net.read_faults() == 0
    _grads_agree("retained", second, first, "second backward against the first, with the bit")


@pytest.mark.gpu
def test_captured_step_with_the_bit_replays_agree():
    """tests/test_dw_queue.py's captured live step, at its size and to its gate: two replays of a step_graph captured in the coarse trunk
    form against the same steps run eagerly with March.coarse_trunk = False."""
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
    ops.March.coarse_trunk = False
    try:
        torch.manual_seed(1)
        A = make()
        for s, b in enumerate(bs):
            A.step(b, s)
            ga.append(grads(A))
    finally:
        ops.March.coarse_trunk = True
    torch.manual_seed(1)
    B = make()
    for s, b in enumerate(bs):
        B.step_graph(b, s)
        gb.append(grads(B))
    assert B._graph is not None                                   # the capture happened: steps 3 and 4 are replays
    assert A.live_counts() == B.live_counts()
    worst = 0.0
    for s in (3, 4):
        assert set(ga[s]) == set(gb[s]) and len(ga[s]) >= 48
        for k in ga[s]:
            err = _rel(gb[s][k], ga[s][k])
            worst = max(worst, err)
            assert np.isfinite(gb[s][k]).all() and float(np.abs(ga[s][k]).max()) > 0 and err < GATE, (s, k, err)
    print(f"replays of the captured coarse-trunk step against eager steps without the bit: NeRF gradients within {worst:.1e}")


@pytest.mark.gpu
def test_piecewise_path_runs_the_coarse_trunk_form(diag):
    """With a kernel-group timer set (bench.py --full) the march runs piece by piece in the same form: both launches over all points
    trunk-only under mlp_fwd_all, both live forwards with the stash under mlp_fwd in the forward, chain and weight gradients on the
    forward's lists -- the one-call march's outputs bit for bit and its gradients to the gates."""
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
    assert ops.March.coarse_trunk is True
    out_f, g_f, _ = run(False)
    out_p, g_p, groups = run(True)
    assert all(torch.equal(a, b) for a, b in zip(out_f, out_p))
    assert set(g_f) == set(g_p)
    _grads_agree("piecewise", g_p, g_f, "piecewise path against the one-call march, coarse trunk form")
    P_c, P_f = n * 5 * 64, n * 5 * 128
    assert groups["mlp_fwd_all"]["launches"] == 2 and groups["mlp_fwd_all"]["points"] == P_c + P_f
    live = groups["mlp_fwd"]["points"]
    assert groups["mlp_fwd"]["launches"] == 2 and 0 < live < P_c + P_f
    assert groups["mlp_bwd_chain"]["points"] == live and groups["mlp_bwd_weights"]["points"] == live
    assert groups["mlp_bwd_chain"]["launches"] == 2 and groups["mlp_bwd_weights"]["launches"] == 2
