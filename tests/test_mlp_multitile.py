"""GPU tests of the MLP kernels PER POINT in the regime where a workgroup runs several tiles (persistent kernels: grid = n_cu or
2 n_cu workgroups, `for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)`, with hand-counted waits that differ between a
workgroup's first tile and its later ones; on 256 CUs a second tile exists only above 65 536 / 32 768 points).

The launch is PERIODIC: a short period of rays (1 280 .. 6 400 points) repeated k times plus a ragged tail, the same for z and for
the upstream d_raw.  A point's result depends on its own row only, so the float64 reference of the whole launch is the reference of
one period, tiled, and no float64 evaluation is larger than 6 400 points.  The period is a multiple of 256 points (a repeated
point sits at the same place of its tile: repeats must agree BIT FOR BIT) and divides none of n_cu x 256, n_cu x 128 and 1 024, so
a read from the wrong tile, slice or queue chunk lands on other data.

Per case and mode (each check on the whole array, on every repeat alone and on the last 256 points alone, each normalised by its
own largest entry, so that a wrong tail or a wrong single tile cannot hide behind the launch's largest entry):
  1. raw against float64 oracle.nerf_mlp at t_mlp_fwd's gate of the plane code;
  2. repeats bit-identical: raw, every stashed h_l / hv row, the ReLU decision words;
  3. d(point) bit-identical between repeats, and against the float64 oracle with the GPU's own ReLU decisions under the rule of
     gpu_diag.masked_grad_check; the per-ray reduction of it at 2 x t_mlp_bwd's gate;
  4. weight gradients count every point once: full launch = k x (launch of one period) + (launch of the tail) to 2e-5 of a
     tensor's largest entry -- a dropped or doubled 32-point stage is 1.2e-4 in case A, a 1 024-point queue chunk 3.9e-3 -- with
     the one-period launch tied to the float64 reference at t_mlp_bwd's gate;
  5. case L: the live-point kernels against the dense launch -- stash rows and d(point) bit for bit in list order, parameter
     gradients to 2e-5;
  6. a second backward on the same stash gives the same d(point) bit for bit.
Every check of a run is evaluated and printed before the test fails, with the place of the first differing row (repeat, tile,
tile modulo the grid, wave, lane), so one run locates a fault."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

H16 = 17                                     # ops.PLANES_F16
# tests/gpu_diag.py t_mlp_fwd: normalised max error of raw by plane code
FWD_GATE = {2: 3e-5, H16: 4e-3, 1: 3e-2}
# tests/gpu_diag.py t_mlp_bwd: parameter gradients against the masked reference by (forward, backward) plane code; d(rays) there is
# 2 x this.  t_mlp_bwd has no (1,1) row: its (2,1) row is 3e-2 for ONE 8-bit operand (dZ) in the weight-gradient products, (1,1)
# makes the stashed activations 8-bit too, so twice that -- the ratio gpu_diag.MASKED_FLOOR has between the same two modes.
BWD_GATE = {(2, 2): 2e-4, (2, H16): 8e-3, (H16, H16): 2e-3, (1, 1): 6e-2}
# tests/gpu_diag.py MASKED_FLOOR / MASKED_FACTOR / MASKED_FACTOR_F16_FWD / MASKED_CAP (masked_grad_check's allowance), by value
MASKED_FLOOR = {(2, 2): 2e-4, (1, 1): 8e-2, (2, H16): 1e-2, (H16, H16): 5e-3}
MASKED_FACTOR, MASKED_FACTOR_F16_FWD, MASKED_CAP = 32.0, 2048.0, 1e-1
SUM_GATE = 2e-5                              # tests/test_dw_queue.py GATE: the same products, another order of the fp32 sums
PERJOB_MAX_PTS = 262144                      # csrc/lush_mlp.h LUSH_DW_PERJOB_MAX_PTS: the chunk queue serves launches above it
DP_COLS = [0, 1, 2, 4, 5, 6]                 # d(point) rows [P][8]: d/d point, pad, d/d view direction, pad

# id: (net, rays, samples, rays per period, every n-th d_raw row of the period zero)
CASES = {"A": (0, 2058, 128, 10, 0),         # 4+ tiles per workgroup; dense dW on the chunk queue, last chunk a quarter
         "B": (0, 1311, 100, 64, 0),         # tiles straddle rays; the last tile holds 28 points; dense dW one job per workgroup
         "C": (1, 81957, 1, 768, 0),         # the noise net: 2.5 tiles per workgroup, ragged tail of 37
         "L": (0, 3430, 128, 10, 4)}         # live list of 3/4 of the points: > 2^18 live points
RUNS = [("A", "h,h", ""), ("A", "2,2", ""), ("A", "2,h", ""), ("A", "1,1", ""),
        ("A", "h,h", "FWD_HALF"), ("A", "h,h", "FWD_512"), ("A", "h,h", "BWD_HALF"), ("A", "h,h", "BWD_512"),
        ("B", "h,h", ""), ("B", "2,2", ""), ("B", "2,h", ""),
        ("C", "2,2", ""), ("C", "noise(h,h)", ""),
        ("L", "h,h", ""), ("L", "2,2", "")]
_CACHE = {}


def nerf_tensors(p, prefix, D):
    t = []
    for l in range(D):
        t += [p[f"{prefix}.pts_linears.{l}.weight"], p[f"{prefix}.pts_linears.{l}.bias"]]
    for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear"):
        t += [p[f"{prefix}.{n}.weight"], p[f"{prefix}.{n}.bias"]]
    return t


def tensor_names(D):
    return [f"pts_linears.{l}.{s}" for l in range(D) for s in ("weight", "bias")] + \
           [f"{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]


class Case:
    """One periodic launch: the period's rays / z / d_raw on the CPU, the counts, and the period's float64 forward per weight set."""

    def __init__(self, cid, n_cu):
        from lush_nerf_amd import synth
        from oracle import lush_oracle as O
        net, R, S, pr, zero_every = CASES[cid]
        if n_cu > 256:                       # the counts of the table are for 256 CUs: keep as many tiles per workgroup on a larger device
            R = -(-R * n_cu // 256)
        seed = 60 + ord(cid)
        self.cid, self.net, self.R, self.S, self.pr, self.n_cu = cid, net, R, S, pr, n_cu
        self.prefix, self.D = ("mlp_fine", 8) if net == 0 else ("mlp_noise_coarse", 4)
        self.pp, self.P = pr * S, R * S
        self.k, self.tail_rays = divmod(R, pr)
        self.tail = self.tail_rays * S
        rays = torch.from_numpy(synth.ray_batch(pr, seed, util.NUM_IMG)["rays"])
        self.batch_p = O.pack_rays(util.H, util.W, util.FOCAL, rays).float().contiguous()
        self.z_p = torch.sort(torch.from_numpy(synth.uniform((pr, S), 0, 1, seed + 50)), -1)[0].contiguous()
        d = torch.from_numpy(np.asarray(synth.normal((self.pp, 4), seed + 7), dtype=np.float32)) * 1e-2
        if net == 1:
            d[:, 3] = 0                      # the noise net has no density output (t_mlp_bwd)
        i = int(d.abs().amax(1).argmax())    # the largest entry goes to row 0: the period, the tail and the whole launch then
        d[[0, i]] = d[[i, 0]]                # choose the same power-of-two loss scale
        if zero_every:
            d[zero_every - 1::zero_every] = 0
        self.draw_p = d.contiguous()
        # the encoder's inputs as the kernels define them: fp32 o + d z, fp32 view direction per point
        self.pts = (self.batch_p[:, None, 0:3] + self.batch_p[:, None, 3:6] * self.z_p[:, :, None]).reshape(-1, 3)
        self.vd = self.batch_p[:, None, 8:11].expand(pr, S, 3).reshape(-1, 3).contiguous()
        self.fwd64 = {}

    def conditions(self):
        n, pp = self.n_cu, self.pp
        c = {f"period {pp} % 256 == 0": pp % 256 == 0, f"{n} x 256 % period = {n * 256 % pp} != 0": n * 256 % pp != 0,
             f"{n} x 128 % period = {n * 128 % pp} != 0": n * 128 % pp != 0, f"period % 1024 = {pp % 1024} != 0": pp % 1024 != 0,
             f"period {pp} <= 6400 points": pp <= 6400, f"{self.k} repeats >= 2": self.k >= 2}
        return c

    def tiled(self, dev, rays=None):
        """(ray batch, z, d_raw) of the whole launch, or of its first `rays` rays, on the device."""
        R = self.R if rays is None else rays
        reps = -(-R // self.pr)
        return (self.batch_p.repeat(reps, 1)[:R].contiguous().to(dev), self.z_p.repeat(reps, 1)[:R].contiguous().to(dev),
                self.draw_p.repeat(reps, 1)[:R * self.S].contiguous().to(dev))

    def forward64(self, p, sharp):
        """float64 oracle.nerf_mlp of one period [pp, 4] (computed once per weight set)."""
        from oracle import lush_oracle as O
        if sharp not in self.fwd64:
            pd = {k: v.double() for k, v in p.items() if k.startswith(self.prefix)}
            x = torch.cat([O.embed(self.pts.double(), 10), O.embed(self.vd.double(), 4)], -1)
            with torch.no_grad():
                self.fwd64[sharp] = O.nerf_mlp(pd, self.prefix, x, 63, 27, self.D)
        return self.fwd64[sharp]

    def masked(self, p, masks, dtype, rows=None):
        """The oracle with the given ReLU decisions in `dtype`, upstream draw_p: (d(point) [rows, 6], {tensor name: gradient}) of
        the period's first `rows` points."""
        from oracle import lush_oracle as O
        n = self.pp if rows is None else rows
        pd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items() if k.startswith(self.prefix)}
        pts, vd = self.pts[:n].to(dtype).requires_grad_(True), self.vd[:n].to(dtype).requires_grad_(True)
        x = torch.cat([O.embed(pts, 10), O.embed(vd, 4)], -1)
        out = util.nerf_mlp_masked(pd, self.prefix, x, self.D, [m[:n].to(dtype) for m in masks])
        (out * self.draw_p[:n].to(dtype)).sum().backward()
        return torch.cat([pts.grad, vd.grad], -1).detach(), {k[len(self.prefix) + 1:]: v.grad.detach() for k, v in pd.items()}

    def ray_grads(self, dp):
        """d(ray batch) [rays, 11] of per-point gradients dp [rays x S, 6] (float64): what lush_ray_grad_reduce sums."""
        n = dp.shape[0] // self.S
        g = dp.reshape(n, self.S, 6)
        out = torch.zeros(n, 11, dtype=dp.dtype)
        out[:, 0:3] = g[..., 0:3].sum(1)
        out[:, 3:6] = (g[..., 0:3] * self.z_p[:n].to(dp.dtype)[:, :, None]).sum(1)
        out[:, 8:11] = g[..., 3:6].sum(1)
        return out


def _case(cid):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if cid not in _CACHE:
        _CACHE[cid] = Case(cid, n_cu)
    return _CACHE[cid]


class Checks:
    """Every check of a run is evaluated and printed; the test fails at the end with all of them."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def gate(self, what, value, gate):
        ok = bool(value <= gate)            # (NaN fails)
        print(f"{'ok  ' if ok else 'FAIL'} {self.tag} {what}: {value:.3e} (gate {gate:.1e})", flush=True)
        if not ok:
            self.bad.append(f"{what}: {value:.3e} > {gate:.1e}")

    def true(self, what, ok, detail=""):
        print(f"{'ok  ' if ok else 'FAIL'} {self.tag} {what}{' -- ' + detail if detail and not ok else ''}", flush=True)
        if not ok:
            self.bad.append(f"{what} {detail}")

    def finish(self):
        assert not self.bad, f"{self.tag}: {len(self.bad)} checks failed:\n  " + "\n  ".join(self.bad)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _where(bad, c, unit=1):
    """Where the rows flagged in bad [P / unit] (one flag per `unit` points) lie: what a fault in a later-tile path is located by."""
    idx = torch.nonzero(bad).flatten() * unit
    p0, p1 = int(idx[0]), int(idx[-1])
    t = p0 // 256
    return (f"{idx.numel()} of {bad.numel()} rows differ; first {p0}: repeat {p0 // c.pp}, row {p0 % c.pp} of the period, 256-point tile {t} "
            f"(tile % {c.n_cu} = {t % c.n_cu}, round {t // c.n_cu}), 128-point tile {p0 // 128} (% {c.n_cu} = {p0 // 128 % c.n_cu}), "
            f"wave {p0 % 256 // 64}, lane {p0 % 64}; last {p1} (repeat {p1 // c.pp}); repeats touched: "
            f"{sorted(set((idx // c.pp).tolist()))[:12]}")


def _repeats_differ(t, c, unit=1):
    """t [planes, rows, cols], one row per `unit` points (whole units of the tail only): row p must hold the bits of row
    p % period.  None, or where it does not."""
    t = _bits(t)
    pp, tail = c.pp // unit, c.tail // unit
    n = c.k * pp
    body = t[:, :n].unflatten(1, (c.k, pp))
    first = body[:, :1]
    if torch.equal(body, first.expand_as(body)) and (tail == 0 or torch.equal(t[:, n:n + tail], t[:, :tail])):
        return None
    bad = torch.zeros(n + tail, dtype=torch.bool, device=t.device)
    bad[:n] = (body != first).any(-1).any(0).flatten()
    if tail:
        bad[n:] = (t[:, n:n + tail] != t[:, :tail]).any(-1).any(0)
    return _where(bad, c, unit)


def _errors(got, ref_p, c):
    """got [P, C] on the device against ref_p [period, C] float64, tiled: normalised max error of (the whole array, the worst
    single repeat and which, the last 256 points), each by the largest reference entry of the SLICE it covers (every whole repeat
    holds the period's entries, so its largest is the period's)."""
    g = got.double()
    n = c.k * c.pp
    nrm = ref_p.abs().max().clamp_min(1e-30)
    e_rep = (g[:n].unflatten(0, (c.k, c.pp)) - ref_p).abs().amax((1, 2)) / nrm
    whole = e_rep.max()
    if c.tail:
        whole = torch.maximum(whole, (g[n:] - ref_p[:c.tail]).abs().max() / nrm)
    idx = torch.arange(c.P - 256, c.P, device=got.device) % c.pp
    last = (g[c.P - 256:] - ref_p[idx]).abs().max() / ref_p[idx].abs().max().clamp_min(1e-30)
    return float(whole), float(e_rep.max()), int(e_rep.argmax()), float(last)


class Layout:
    """Where the forward stash of P points keeps the ReLU words and the h_l / hv rows (lush_debug_stash_layout)."""

    def __init__(self, net, ns, P):
        import ctypes as C
        from lush_nerf_amd import lib
        off = (C.c_longlong * 16)()
        lib.call("lush_debug_stash_layout", net, ns, P, off)
        self.ns, self.Ppad, self.HW, self.NL = ns, off[12], off[14], off[15]
        self.arrays = [(f"h{l}", off[2 + l], self.HW) for l in range(self.NL)] + [("hv", off[11], self.HW // 2)]
        self.mask = off[0]
        words = off[2] - off[0] - 4096       # [ReLU words][4 KiB nobody reads][h_0 ...]: the words of one 32-point block are contiguous
        self.block_bytes = words // (self.Ppad // 32)
        assert self.block_bytes * (self.Ppad // 32) == words and self.block_bytes % 8 == 0, (words, self.Ppad)

    def rows(self, stash, i):
        """Array i of the stash as int16 [planes, Ppad, cols] (a view)."""
        _, off, cols = self.arrays[i]
        return stash[off:off + self.ns * self.Ppad * cols * 2].view(torch.int16).view(self.ns, self.Ppad, cols)

    def words(self, stash, blocks):
        """The ReLU decision words of the first `blocks` 32-point blocks as int64 [1, blocks, words]: per block [layer][row block of
        32 units][16 words], NL + 1 layers of HW / 32 row blocks each.  The views layer has HW / 64 row blocks: the other half of
        its words is never written and is left out."""
        nrb = self.HW // 32
        assert self.block_bytes == (self.NL + 1) * nrb * 128, (self.block_bytes, self.NL, nrb)
        w = stash[self.mask:self.mask + blocks * self.block_bytes].view(torch.int64).view(blocks, self.NL + 1, nrb * 16)
        return torch.cat([w[:, :self.NL].flatten(1), w[:, self.NL, :nrb * 8]], 1)[None]

    def decisions(self, stash, n, f16):
        """util.stash_masks of the first n points, decoded from those rows only (the whole stash stays on the device)."""
        out = []
        for i, (_, _, cols) in enumerate(self.arrays):
            b = self.rows(stash, i)[:, :n].contiguous().view(torch.uint8).flatten().cpu().numpy()
            out.append(torch.from_numpy((util.stash_planes(b, 0, self.ns, n, cols, f16) > 0).astype(np.float32)))
        return out


def _launch(c, ops, lib, pf, pb, variant, tens, pk, pkb, dev, rays=None):
    """Forward with the stash + backward of the whole launch (or of its first `rays` rays)."""
    batch, z, draw = c.tiled(dev, rays)
    sc = ops.stash_code(pf, pb)
    # whatever the kernels leave unwritten must not look written: the allocations of the two workspaces most likely get these blocks back
    for n in (lib.load().lush_mlp_stash_bytes(c.net, pf, ops.nplanes(sc), batch.shape[0] * c.S), lib.load().lush_mlp_dstash_bytes(c.net, pb, batch.shape[0] * c.S)):
        torch.empty(n // 8, dtype=torch.int64, device=dev).random_()
    raw, stash = ops.mlp_forward(c.net, pf, tens, pk, batch, z, True, sc, variant)
    grads, dpts = ops.mlp_backward(c.net, sc, pb, tens, pkb, batch, z, draw, stash, variant=variant)
    torch.cuda.synchronize()
    return batch, z, draw, raw, stash, grads, dpts


def _forward_checks(ck, c, ops, raw, ref64, pf, what="raw"):
    ncol = 4 if c.net == 0 else 3
    for name, cols in [("rgb", slice(0, 3))] + ([("sigma", slice(3, 4))] if c.net == 0 else []):
        whole, rep, irep, last = _errors(raw[:, cols], ref64[:, cols], c)
        g = FWD_GATE[pf]
        ck.gate(f"1 {what} {name} against float64, whole launch", whole, g)
        ck.gate(f"1 {what} {name} against float64, worst repeat alone (repeat {irep} of {c.k})", rep, g)
        ck.gate(f"1 {what} {name} against float64, last 256 points alone", last, g)
    why = _repeats_differ(raw[None, :, :ncol], c)
    ck.true(f"2 {what} of every repeat bit-identical", why is None, why or "")


def _planes(ops, planes):
    if planes == "noise(h,h)":
        pr = ops.Precision(*ops.parse_planes("h,h")).noise()
        return pr.fwd, pr.bwd
    return ops.parse_planes(planes)


def _setup(cid, planes, variant):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the HIP path has no CPU fallback")
    from lush_nerf_amd import lib, ops
    lib.load()
    dev = torch.device("cuda:0")
    c = _case(cid)
    pf, pb = _planes(ops, planes)
    var = getattr(lib, "VARIANT_" + variant) if variant else 0
    sharp = H16 in (pf, pb)                  # default init for the bf16 modes, the sharp density field for the fp16 ones
    p = util.params(3, sharp=sharp)
    tens = [t.to(dev) for t in nerf_tensors(p, c.prefix, c.D)]
    ck = Checks(f"[{cid} {planes}{' ' + variant if variant else ''}]")
    print(f"\n{ck.tag} {'noise' if c.net else 'NeRF'} net, {c.R} x {c.S} = {c.P} points = {c.k} x {c.pp} + {c.tail}; {c.n_cu} CUs: "
          f"{c.P / 256 / c.n_cu:.2f} 256-point tiles, {c.P / 128 / c.n_cu:.2f} 128-point tiles per CU; weights: {'sharp' if sharp else 'default init'}")
    for what, ok in c.conditions().items():
        print(f"     period condition: {what}: {ok}")
        assert ok, what
    return lib, ops, dev, c, pf, pb, var, p, tens, ck


@pytest.mark.parametrize("cid,planes,variant", RUNS, ids=[f"{a}-{b}{'-' + v if v else ''}" for a, b, v in RUNS])
def test_multitile_launch_per_point(cid, planes, variant):
    lib, ops, dev, c, pf, pb, var, p, tens, ck = _setup(cid, planes, variant)
    mode = (pf, pb)
    f16 = pf == H16
    pk = ops.mlp_pack(c.net, pf, tens)
    pkb = pk if pb == pf else ops.mlp_pack(c.net, pb, tens)
    batch, z, draw, raw, stash, grads, dpts = _launch(c, ops, lib, pf, pb, var, tens, pk, pkb, dev)
    ref64 = c.forward64(p, H16 in mode).to(dev)

    # 1, 2: the forward
    _forward_checks(ck, c, ops, raw, ref64, pf)
    L = Layout(c.net, ops.nplanes(ops.stash_code(pf, pb)), c.P)
    for i, (name, _, _) in enumerate(L.arrays):
        why = _repeats_differ(L.rows(stash, i), c)       # (rows at and beyond P are never written: not compared)
        ck.true(f"2 stash {name} rows of every repeat bit-identical", why is None, why or "")
    why = _repeats_differ(L.words(stash, c.P // 32), c, unit=32)      # (the words of whole 32-point blocks)
    ck.true("2 ReLU decision words of every repeat bit-identical", why is None, why or "")
    masks = L.decisions(stash, c.pp, f16)

    # 3: the gradient chain per point
    dp = dpts[:, DP_COLS]
    why = _repeats_differ(dp[None], c)
    ck.true("3 d(point) of every repeat bit-identical", why is None, why or "")
    d64, g64 = c.masked(p, masks, torch.float64)
    d32, _ = c.masked(p, masks, torch.float32)
    floor, factor = MASKED_FLOOR[mode], (MASKED_FACTOR_F16_FWD if f16 else MASKED_FACTOR)
    allow = lambda e32: max(floor, min(MASKED_CAP, factor * e32))
    e32 = util.relerr(d32, d64)
    i_last = torch.arange(c.P - 256, c.P) % c.pp
    e32_last = util.relerr(d32[i_last], d64[i_last])
    whole, rep, irep, last = _errors(dp, d64.to(dev), c)
    print(f"     {ck.tag} fp32 run of the masked reference against float64: d(point) {e32:.2e}, on the last 256 points {e32_last:.2e}; "
          f"d/d point alone {_errors(dp[:, :3], d64[:, :3].to(dev), c)[0]:.2e}, d/d view direction alone {_errors(dp[:, 3:], d64[:, 3:].to(dev), c)[0]:.2e}")
    ck.gate("3 d(point) against masked float64, whole launch", whole, allow(e32))
    ck.gate(f"3 d(point) against masked float64, worst repeat alone (repeat {irep} of {c.k})", rep, allow(e32))
    ck.gate("3 d(point) against masked float64, last 256 points alone", last, allow(e32_last))
    drays = torch.zeros(c.R, 11, device=dev)
    lib.call("lush_ray_grad_reduce", lib.ptr(dpts), lib.ptr(z), c.R, c.S, lib.ptr(drays), ops._stream())
    dr_p = c.ray_grads(d64)
    ck.gate("3 d(rays) = lush_ray_grad_reduce of d(point) against masked float64", util.relerr(drays, dr_p.repeat(c.k + 1, 1)[:c.R]), 2 * BWD_GATE[mode])

    # 4: the weight gradients count every point once
    names = tensor_names(c.D)
    dead = ("alpha_linear.weight", "alpha_linear.bias") if c.net == 1 else ()      # NeRF_Noise has no density head: column 3 of d_raw is zero
    full = [g.double().cpu() for g in grads]
    _, _, _, _, stash_p, grads_p, _ = _launch(c, ops, lib, pf, pb, var, tens, pk, pkb, dev, rays=c.pr)
    masks_p = util.stash_masks(c.net, L.ns, c.pp, stash_p, f16=f16)
    same = all(torch.equal(a, b) for a, b in zip(masks, masks_p))
    print(f"     {ck.tag} the one-period launch took {'the same' if same else 'OTHER'} ReLU decisions as the first period of the whole launch")
    g64_p = g64 if same else c.masked(p, masks_p, torch.float64)[1]
    worst, wname = max((util.relerr(g, g64_p[n]), n) for n, g in zip(names, grads_p) if n not in dead)
    ck.gate(f"4 weight gradients of ONE period against masked float64 (worst: {wname})", worst, BWD_GATE[mode])
    gp = [g.double().cpu() for g in grads_p]
    gt = [torch.zeros_like(g) for g in gp]
    if c.tail:
        gt = [g.double().cpu() for g in _launch(c, ops, lib, pf, pb, var, tens, pk, pkb, dev, rays=c.tail_rays)[5]]
    del stash_p, grads_p
    worst, wname, alive = 0.0, "", True
    for n, g, a, b in zip(names, full, gp, gt):
        want = c.k * a + b
        alive = alive and bool(torch.isfinite(g).all()) and (n in dead or float(g.abs().max()) > 0)
        e = util.relerr(g, want) if n not in dead else float(g.abs().max())
        if not e <= worst:
            worst, wname = e, n
    ck.gate(f"4 weight gradients = {c.k} x one period + the tail (worst: {wname})", worst, SUM_GATE)
    ck.true("4 every weight gradient finite and non-zero", alive)

    # 6: a second backward on the same stash
    if cid == "A" and planes == "h,h" and not variant:
        _, dpts2 = ops.mlp_backward(c.net, ops.stash_code(pf, pb), pb, tens, pkb, batch, z, draw, stash, variant=var)
        torch.cuda.synchronize()
        bad = (_bits(dpts2[:, DP_COLS]) != _bits(dp)).any(-1)
        ck.true("6 second backward on the same stash: d(point) bit-identical", not bool(bad.any()), _where(bad, c) if bool(bad.any()) else "")
        del dpts2

    # 5: the live-point kernels against the dense launch
    if cid == "L":
        lidx, draw_c, ray_start, cnt = ops.live_compact(draw, c.R, c.S)
        n_live = int(cnt[0].item())
        ck.true(f"5 live_compact counts 3/4 of the points ({n_live} of {c.P}), above {PERJOB_MAX_PTS}",
                n_live == 3 * c.P // 4 and n_live > PERJOB_MAX_PTS and int(cnt[1].item()) == c.P)
        want_idx = torch.nonzero(draw.abs().amax(1) > 0).flatten().to(torch.int32)
        ck.true("5 the live list holds the points with a non-zero d_raw row, in order", want_idx.numel() == n_live and torch.equal(lidx[:n_live], want_idx))
        li = lidx[:n_live].long()
        stash_l = ops.mlp_forward_live(c.net, pf, tens, pk, batch, z, lidx, cnt, ops.stash_code(pf, pb), var)
        for i, (name, _, _) in enumerate(L.arrays):
            bad = (L.rows(stash_l, i)[:, :n_live] != L.rows(stash, i).index_select(1, li)).any(-1).any(0)
            ck.true(f"5 live stash {name}: list position i holds the dense launch's row of point lidx[i], bit for bit", not bool(bad.any()),
                    f"list positions: {_where(bad, c)}" if bool(bad.any()) else "")
        grads_l, dpts_l = ops.mlp_backward(c.net, ops.stash_code(pf, pb), pb, tens, pkb, batch, z, draw_c, stash_l, variant=var, live=(lidx, cnt))
        torch.cuda.synchronize()
        bad = (_bits(dpts_l[:n_live][:, DP_COLS]) != _bits(dp.index_select(0, li))).any(-1)
        ck.true("5 live d(point) in list order, bit-identical to the dense launch's", not bool(bad.any()),
                f"list positions: {_where(bad, c)}" if bool(bad.any()) else "")
        worst, wname = max((util.relerr(gl, g), n) for n, gl, g in zip(names, grads_l, full))
        ck.gate(f"5 live weight gradients against the dense launch (worst: {wname})", worst, SUM_GATE)
        ck.true("5 every live weight gradient finite", all(bool(torch.isfinite(g).all()) for g in grads_l))
        del stash_l, grads_l, dpts_l
    del stash, grads, dpts, dp, raw
    torch.cuda.empty_cache()
    ck.finish()


@pytest.mark.parametrize("planes", ["h,h", "2,2"])
def test_multitile_inference_forward_per_point(planes):
    """The forward without the stash (the inference kernels) on case A: raw against float64 and bit-identical repeats."""
    lib, ops, dev, c, pf, pb, var, p, tens, ck = _setup("A", planes, "")
    batch, z, _ = c.tiled(dev)
    raw, stash = ops.mlp_forward(c.net, pf, tens, ops.mlp_pack(c.net, pf, tens), batch, z, False)
    torch.cuda.synchronize()
    assert stash is None
    _forward_checks(ck, c, ops, raw, c.forward64(p, H16 in (pf, pb)).to(dev), pf, what="raw (no stash)")
    del raw
    torch.cuda.empty_cache()
    ck.finish()
