"""GPU tests of the weight gradients' chunk queue (dw_group_kernel, DwGroup::per_job == 3: DESIGN.md section 5) against the walk it
replaced, which LUSH_VARIANT_DW_WALK keeps reachable.  The two sum the same products; which of them share an fp32 accumulator
before the atomics differs (a 1/256 slice of the points against whatever chunks a workgroup claimed), so every parameter gradient
is held to 2e-5 of its tensor's largest entry, the gate of test_weight_gradient_split_agrees_with_the_walk, and the launches in
front of the weight gradients (forward, chain) to bit equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 2e-5
THRESHOLD = 262144          # csrc/lush_mlp.h LUSH_DW_PERJOB_MAX_PTS: the queue serves launches above it
CHUNK = 1024                # csrc/lush_mlp.h LUSH_DW_QUEUE_CHUNK


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)


# 2 056 x 128 = 263 168 points: just above the threshold (257 whole chunks); 2 058 x 128 = 263 424: the last chunk is a quarter
# (256 points); 20 480 x 128: the fine pass of the timed configuration
@pytest.mark.parametrize("planes", ["h,h", "2,2"])
@pytest.mark.parametrize("rays", [2056, 2058, 20480])
def test_queue_agrees_with_the_walk(tmp_path, planes, rays):
    from lush_nerf_amd import lib
    assert rays * 128 > THRESHOLD and (rays == 2058) == ((rays * 128 + 255) // 256 * 256 % CHUNK != 0)
    outs = []
    for var in (0, lib.VARIANT_DW_WALK):
        env = dict(os.environ, LUSH_PLANES=planes, LUSH_VARIANT=str(var), LUSH_AB_R=str(rays), LUSH_AB_S="128")
        out = str(tmp_path / f"dw_{var}.npz")
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ab_worker.py"), out], check=True, env=env, timeout=600)
        outs.append(np.load(out))
    a, b = outs
    assert set(a.files) == set(b.files)
    worst = 0.0
    for k in a.files:
        if k in ("raw", "dpts"):
            assert np.array_equal(a[k], b[k]), k           # the forward and the chain are the same launches
            continue
        err = _rel(a[k], b[k])
        worst = max(worst, err)
        print(f"{planes} {rays} x 128 {k}: {err:.2e}")
        assert np.isfinite(a[k]).all() and float(np.abs(b[k]).max()) > 0 and err < GATE, (k, err)
    print(f"chunk queue against the walk ({planes}, {rays} x 128): parameter gradients within {worst:.1e}")


@pytest.mark.parametrize("planes", ["h,h", "2,2"])
def test_two_backward_calls_on_one_workspace_agree(planes):
    """The cursors live in the dstash header and every call has to find them zero: two calls in a row on ONE dstash, which starts
    out filled with ones bits, give the same gradients (to the gate) as each other and as the walk."""
    from lush_nerf_amd import lib, ops, synth
    from oracle import lush_oracle as O       # (test infrastructure: ray packing of the synthetic batch only)
    dev = torch.device("cuda:0")
    R, S = 2058, 128
    pf, pb = ops.parse_planes(planes)
    w = synth.all_weights(30, 3, sharp=True)
    names = [f"mlp_fine.pts_linears.{l}.{s}" for l in range(8) for s in ("weight", "bias")] + \
            [f"mlp_fine.{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]
    tens = [torch.from_numpy(w[n]).to(dev) for n in names]
    b = synth.ray_batch(R, 5)
    batch = O.pack_rays(synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, torch.from_numpy(b["rays"])).to(dev)
    g = torch.Generator().manual_seed(11)
    z = torch.sort(torch.rand(R, S, generator=g), -1)[0].to(dev)
    draw = (torch.randn(R * S, 4, generator=g) * 1e-2).to(dev)
    pk = ops.mlp_pack(0, pf, tens)
    sc = ops.stash_code(pf, pb)
    raw, stash = ops.mlp_forward(0, pf, tens, pk, batch, z, True, sc, 0)
    dstash = torch.full((lib.load().lush_mlp_dstash_bytes(0, pb, R * S),), 255, dtype=torch.uint8, device=dev)
    st = lib.mlp_struct(tens, 8)

    def run(variant):
        grads = [torch.zeros_like(t) for t in tens]
        gs = lib.mlp_struct(grads, 8)
        dpts = torch.empty(R * S, 8, dtype=torch.float32, device=dev)
        lib.call("lush_mlp_bwd", 0, sc, pb, lib.ptr(batch), lib.ptr(z), R, S, lib.ptr(pk), C.byref(st), lib.ptr(draw), lib.ptr(stash),
                 lib.ptr(dstash), C.byref(gs), lib.ptr(dpts), int(variant), ops._stream())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in grads]

    first, second, walk = run(0), run(0), run(lib.VARIANT_DW_WALK)
    worst = 0.0
    for n_, a, b_, c in zip(names, first, second, walk):
        e1, e2 = _rel(a, b_), _rel(b_, c)
        worst = max(worst, e1, e2)
        print(f"{planes} {n_}: second call against the first {e1:.2e}, against the walk {e2:.2e}")
        assert np.isfinite(a).all() and float(np.abs(c).max()) > 0 and e1 < GATE and e2 < GATE, (n_, e1, e2)
    print(f"two calls on one workspace ({planes}): within {worst:.1e}")


def test_captured_live_step_replays_agree():
    """The headline step (live points, mode h,h) captured in a HIP graph: the cursors are re-armed by launches of the step itself, so
    every replay finds them zero.  With a learning rate of zero the parameters stand still and step s has the same draws in both
    trainers: the NeRF networks' gradients of two replays against the same steps run eagerly."""
    import argparse
    from lush_nerf_amd import model as M, ops, synth
    from lush_nerf_amd.trainer import Trainer
    dev = torch.device("cuda:0")

    def make():
        args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                                  N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                                  rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=80)
        net = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4),
                        precision=ops.Precision(*ops.parse_planes("h,h")))
        M.load_reference_weights(net, synth.all_weights(30, 3, sharp=True))
        return Trainer(net.to(dev), synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, 64, 64, lrate=0.0, kernel_start_iter=0, allkernel_start_iter=0)

    n, steps = 2048, 5          # x 5 rays per pixel of the blur kernel: 10 240 rays, 1.31 M points in the fine pass
    bs = []
    for s in range(steps):
        b = {k: torch.from_numpy(v).to(dev) for k, v in synth.ray_batch(n, 5, 30, step=s).items()}
        b["target"] = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(100 + s))
        bs.append(b)

    def grads(tr):
        return {k: p.grad.detach().cpu().numpy().copy() for k, p in tr.model.named_parameters()
                if k.startswith(("mlp_fine.", "mlp_coarse.")) and p.grad is not None}

    torch.manual_seed(1)
    A = make()
    ga = []
    for s, b in enumerate(bs):
        A.step(b, s)
        ga.append(grads(A))
    live = A.live_counts()
    torch.manual_seed(1)
    B = make()
    gb = []
    for s, b in enumerate(bs):
        B.step_graph(b, s)
        gb.append(grads(B))
    assert B._graph is not None                                   # the capture happened: steps 3 and 4 are replays
    print("live counts of the eager run {fine live, fine, coarse live, coarse}:", live)
    assert live[1] > 0 and live[0] / live[1] * (n * 5 * 128) > THRESHOLD, live      # the fine pass's live launch is a queue launch
    worst = 0.0
    for s in (3, 4):
        assert set(ga[s]) == set(gb[s]) and len(ga[s]) >= 48
        for k in ga[s]:
            err = _rel(gb[s][k], ga[s][k])
            worst = max(worst, err)
            print(f"step {s} {k}: {err:.2e}")
            assert np.isfinite(gb[s][k]).all() and float(np.abs(ga[s][k]).max()) > 0 and err < GATE, (s, k, err)
    print(f"replays of the captured live step against the eager steps: NeRF gradients within {worst:.1e}")
