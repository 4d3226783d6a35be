#!/usr/bin/env python3
"""Developer tool (needs a GPU): lush_mlp_bwd_weights, mode h,h, over the seven point counts of profiles/r07_dw_queue.md in ONE
process per library (LUSH_SO names a build of tools/build_variant.py; none: the product), with the timing of tools/bench_mlp.py
WHAT=weights REPS=10: one warm call, best of ten event-timed calls.  One JSON line per size; TAG labels the lines."""
import ctypes as C
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from lush_nerf_amd import lib, ops, synth
if os.environ.get("LUSH_SO"):
    lib.use_library(os.environ["LUSH_SO"])
from oracle import lush_oracle as O

dev = torch.device("cuda:0")
variant = int(os.environ.get("VARIANT", 0))
tag = os.environ.get("TAG", "")
w = synth.all_weights(30, 0)
names = [f"mlp_fine.pts_linears.{l}.{s}" for l in range(8) for s in ("weight", "bias")] + \
        [f"mlp_fine.{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]
tens = [torch.from_numpy(w[n]).to(dev) for n in names]
H = ops.PLANES_F16
pk = ops.mlp_pack(0, H, tens)
st = lib.mlp_struct(tens, 8)
for R in (4096, 8192, 12288, 20480):
    b = synth.ray_batch(R, 1)
    batch = O.pack_rays(synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, torch.from_numpy(b["rays"])).to(dev)
    for S in (64, 128):
        z = torch.sort(torch.rand(R, S, device=dev), -1)[0]
        draw = torch.randn(R * S, 4, device=dev) * 1e-3
        raw, stash = ops.mlp_forward(0, H, tens, pk, batch, z, True, H, variant)
        dstash = torch.empty(lib.load().lush_mlp_dstash_bytes(0, H, R * S), dtype=torch.uint8, device=dev)
        grads = [torch.zeros_like(t) for t in tens]
        dpts = torch.empty(R * S, 8, device=dev)
        gs = lib.mlp_struct(grads, 8)
        lib.call("lush_mlp_bwd_chain", 0, H, H, lib.ptr(batch), lib.ptr(z), R, S, lib.ptr(pk), C.byref(st), lib.ptr(draw), lib.ptr(stash),
                 lib.ptr(dstash), lib.ptr(dpts), variant, ops._stream())

        def weights():
            lib.call("lush_mlp_bwd_weights", 0, H, H, R, S, C.byref(st), lib.ptr(draw), lib.ptr(stash), lib.ptr(dstash), C.byref(gs), variant, ops._stream())
        weights(); torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); weights(); e.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(e))
        print(json.dumps({"tag": tag, "variant": variant, "R": R, "S": S, "points": R * S, "weights_ms": round(min(ts), 4)}), flush=True)
        del stash, dstash, dpts, raw
