#!/usr/bin/env python3
"""Developer tool (needs a GPU and a -DLUSH_CLOCK build named by LUSH_SO): per-job workgroup time per point of the grouped
weight-gradient launch as one job per workgroup (LUSH_VARIANT_DW_SPLIT), the way profiles/r05_dw_jobs.md took it: fine-pass shape,
the stamps of the last launch after SECONDS of back-to-back launches, workgroups grouped by the job the host's plan gave them
(lush_debug_dw_plan).  One JSON line per job; TAG labels the lines.

  python tools/build_variant.py --out build/clock.so --flags=-DLUSH_CLOCK
  LUSH_SO=build/clock.so TAG=new python tools/dw_jobs_probe.py            >> profiles/r12_dw_jobs.jsonl"""
import ctypes as C
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from lush_nerf_amd import lib, ops, synth
lib.use_library(os.environ["LUSH_SO"])
from oracle import lush_oracle as O

dev = torch.device("cuda:0")
R, S = 20480, 128
SECONDS = float(os.environ.get("SECONDS", 1.5))
variant = lib.VARIANT_DW_SPLIT
tag = os.environ.get("TAG", "")
w = synth.all_weights(30, 0)
names = [f"mlp_fine.pts_linears.{l}.{s}" for l in range(8) for s in ("weight", "bias")] + \
        [f"mlp_fine.{n}.{s}" for n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear") for s in ("weight", "bias")]
tens = [torch.from_numpy(w[n]).to(dev) for n in names]
b = synth.ray_batch(R, 1)
batch = O.pack_rays(synth.H_DEF, synth.W_DEF, synth.FOCAL_DEF, torch.from_numpy(b["rays"])).to(dev)
z = torch.sort(torch.rand(R, S, device=dev), -1)[0]
draw = torch.randn(R * S, 4, device=dev) * 1e-3
H = ops.PLANES_F16
so = C.CDLL(lib.SO_PATH)
L = lib.load()
pk = ops.mlp_pack(0, H, tens)
raw, stash = ops.mlp_forward(0, H, tens, pk, batch, z, True, H)
dstash = torch.empty(L.lush_mlp_dstash_bytes(0, H, R * S), dtype=torch.uint8, device=dev)
grads = [torch.zeros_like(t) for t in tens]
dpts = torch.empty(R * S, 8, device=dev)
st, gs = lib.mlp_struct(tens, 8), lib.mlp_struct(grads, 8)
lib.call("lush_mlp_bwd_chain", 0, H, H, lib.ptr(batch), lib.ptr(z), R, S, lib.ptr(pk), C.byref(st), lib.ptr(draw), lib.ptr(stash),
         lib.ptr(dstash), lib.ptr(dpts), 0, ops._stream())


def weights():
    lib.call("lush_mlp_bwd_weights", 0, H, H, R, S, C.byref(st), lib.ptr(draw), lib.ptr(stash), lib.ptr(dstash), C.byref(gs), variant, ops._stream())


def stamps():
    out = (C.c_ulonglong * 4096)()
    assert so.lush_debug_clock_dw(out) == 0
    return np.frombuffer(out, dtype=np.uint64).reshape(1024, 4).astype(np.float64)


cus = torch.cuda.get_device_properties(0).multi_processor_count
o = (C.c_longlong * 80)()
assert L.lush_debug_dw_plan(0, H, H, R * S, variant, 0, cus, o) == 0
n, per_job = o[0], o[1]
jobs = [list(o)[7 + 6 * i:13 + 6 * i] for i in range(n)]      # n_out, k_in, k2_in, pe_mode, pps, first
first = [j[5] for j in jobs] + [o[79]]
weights(); torch.cuda.synchronize(); stamps()
t0 = time.perf_counter()
while time.perf_counter() - t0 < SECONDS:
    for _ in range(8):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); weights(); e.record()
    torch.cuda.synchronize()
ms = a.elapsed_time(e)
s = stamps()
us = (s[:, 3] - s[:, 1]) / 100.0
print(json.dumps({"tag": tag, "per_job": per_job, "cus": cus, "launch_ms": round(ms, 3), "workgroups": int((us > 0).sum())}), flush=True)
for i, j in enumerate(jobs):
    u = us[first[i]:first[i + 1]]
    u = u[u > 0]
    pps = j[4]
    print(json.dumps({"tag": tag, "job": i, "n_out": j[0], "k_in": j[1], "k2_in": j[2], "pe_mode": j[3], "pps": pps, "wgs": int(u.size),
                      "wg_us_median": round(float(np.median(u)), 1), "wg_us_min": round(float(u.min()), 1), "wg_us_max": round(float(u.max()), 1),
                      "ns_per_point": round(float(np.median(u)) * 1000.0 / pps, 2)}), flush=True)
