"""CPU-side tests: C-ABI exports, host logic, deterministic generator, 2-rank gloo data-parallel plumbing.
No compute call into the HIP library is made here (there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from lush_nerf_amd import lib, synth
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_every_declared_symbol():
    lib.build()
    so = ctypes.CDLL(lib.SO_PATH)
    header = open(os.path.join(ROOT, "include", "lush_march.h")).read()
    declared = set(re.findall(r"\b(lush_[a-z0-9_]+)\s*\(", header))
    declared -= {"lush_stream_t"}
    assert len(declared) >= 30
    missing = [n for n in sorted(declared) if not hasattr(so, n)]
    assert not missing, missing
    assert set(lib.EXPORTS) == declared      # nothing is bound that is not declared, nothing declared is left unbound
    l = lib.load()
    assert all(list(getattr(l, n).argtypes) == lib._SIGS[n][0] and getattr(l, n).restype is lib._SIGS[n][1] for n in declared)
    assert l.lush_abi_version() == lib.ABI_VERSION == 10
    # pure host queries (no device work)
    p1, p3 = l.lush_mlp_packed_bytes(0, 1), l.lush_mlp_packed_bytes(0, 3)
    assert p1 > 2 * 593408 * 2 and 2.9 * p1 < p3 < 3 * p1      # fragments scale with planes, the fp32 bias block does not
    assert l.lush_mlp_packed_bytes(7, 1) == 0
    assert l.lush_mlp_stash_bytes(0, 2, 2, 64) > 0 and l.lush_mlp_stash_bytes(0, 2, 1, 65) == l.lush_mlp_stash_bytes(0, 2, 1, 128)
    assert 0 < l.lush_mlp_stash_bytes(0, 2, 0, 128) < l.lush_mlp_stash_bytes(0, 2, 1, 128) < l.lush_mlp_stash_bytes(0, 2, 2, 128)


def _pinned_abi():
    import json
    return json.load(open(os.path.join(ROOT, "tests", "abi_signatures.json")))


def test_binding_read_from_the_header_is_the_hand_written_one():
    """lib.py binds what abi.py reads from include/lush_march.h.  tests/abi_signatures.json is the table, the constants and the
    struct layouts that lib.py and ops.py stated by hand before that (dumped from them, letter by letter): the derived binding
    equals it entry for entry -- the hand-written POINTER(c_size_t / c_longlong / c_int) of host out-parameters count as `p`, and
    the `jobs` of lush_pack_plan_build is the one struct pointer the table had left untyped."""
    pin = _pinned_abi()
    a = lib._abi                             # abi.parse(include/lush_march.h), read once at import
    assert (len(a.protos), len(a.structs), len(a.consts)) == (67, 9, 29)
    assert a.protos is lib._SIGS and list(a.protos) == lib.EXPORTS
    kind = {"i": ctypes.c_int, "f": ctypes.c_float, "d": ctypes.c_double, "ll": ctypes.c_longlong, "ull": ctypes.c_ulonglong,
            "sz": ctypes.c_size_t, "p": ctypes.c_void_p, "str": ctypes.c_char_p}
    kind.update({n: ctypes.POINTER(c) for n, c in a.structs.items()})
    assert set(a.protos) == set(pin["prototypes"])
    # ONE entry is typed where the hand-written table had a plain `p`: `const lush_pack_job* jobs` is a pointer to a struct of the
    # header.  Its only caller (ops.PackPlan) passes a PackJobC array, which the typed pointer takes; a float or a tensor address no longer passes
    assert pin["prototypes"]["lush_pack_plan_build"][0][0] == "p"
    pin["prototypes"]["lush_pack_plan_build"][0][0] = "lush_pack_job"
    ctypes.POINTER(lib.PackJobC).from_param((lib.PackJobC * 2)())
    for name, (args, res) in pin["prototypes"].items():
        got_args, got_res = a.protos[name]
        assert len(got_args) == len(args) and all(g is kind[k] for g, k in zip(got_args, args)), name
        assert got_res is kind[res], name
    # constants: the literals lib.py / ops.py carried (and the three only the header and csrc/ had), under the public names
    want = {**pin["constants"], **pin["constants_header_only"]}
    assert a.consts == want and len(pin["constants_header_only"]) == 3
    assert all(getattr(lib, k[len("LUSH_"):]) == v for k, v in want.items())
    assert lib.FAULT_NAMES == {int(b): n for b, n in pin["fault_names"].items()} and list(lib.FAULT_NAMES) == sorted(lib.FAULT_NAMES)
    from lush_nerf_amd import ops
    assert ops.PLANES_F16 == lib.PLANES_F16 == 17 and ops.RBK_RVW_OFFSET == lib.RBK_RVW_OFFSET == 480


def test_structs_read_from_the_header_have_the_hand_written_layout():
    """Each of the header's 9 structs: field names in header order, sizeof and every field's offset and size as the hand-written
    classes had them (tests/abi_signatures.json); a *_grads struct and its *_params twin differ in `const` alone and are ONE class,
    so lib.mlp_struct / rbk_struct serve both roles and byref() of one is accepted for either pointer type."""
    pin = _pinned_abi()
    structs = lib._abi.structs
    assert list(structs) == list(pin["structs"]) and len(structs) == 9
    for name, want in pin["structs"].items():
        cls = structs[name]
        assert ctypes.sizeof(cls) == want["size"], name
        assert [[f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size] for f in cls._fields_] == want["fields"], name
    for a, b in pin["aliases"]:
        assert structs[a] is structs[b], (a, b)
    assert len(set(structs.values())) == 7
    assert (lib.MlpParams, lib.RbkParams, lib.MarchCfgC, lib.PackJobC, lib.MarchDraws, lib.MarchOut, lib.MarchGout) == tuple(
        structs[n] for n in ("lush_mlp_grads", "lush_rbk_grads", "lush_march_cfg", "lush_pack_job", "lush_march_draws", "lush_march_out", "lush_march_gout"))
    assert lib.PackJobC.prm.size == 8 and dict(lib.PackJobC._fields_)["prm"] is ctypes.POINTER(lib.MlpParams)


def test_header_reader_refuses_rather_than_guesses():
    """abi.parse on small header strings: what the typing rule does not cover raises and names the declaration; comments inside a
    parameter list and several declarators on one struct line are read."""
    from lush_nerf_amd import abi
    for text, word in (("int lush_f(int n, uint8_t flag, lush_stream_t s);", "lush_f"),               # unknown parameter type
                       ("int lush_f(float** rows);", "lush_f"),
                       ("float* lush_f(int n);", "lush_f"),
                       ("#define LUSH_SCALE 1.5f\n", "LUSH_SCALE"),
                       ("#define LUSH_BOTH (LUSH_A | LUSH_B)\n", "LUSH_BOTH"),
                       ("#define LUSH_MAX(a, b) ((a) > (b) ? (a) : (b))\n", "LUSH_MAX"),
                       ("typedef struct { int n; short tag; } lush_s;", "lush_s"),                    # unknown field type
                       ("typedef struct { int n; float m[2][2]; } lush_s;", "lush_s"),
                       ("typedef int lush_handle;", "lush_handle"),
                       ("extern int lush_counter;", "lush_counter")):
        with pytest.raises(ValueError, match=word):
            abi.parse(text)
    a = abi.parse('''/* a header */
#ifndef LUSH_T_H
#define LUSH_T_H
#ifdef __cplusplus
extern "C" {
#endif
typedef void* lush_stream_t;
#define LUSH_A 7      /* a comment that goes on
#define LUSH_GONE 1
                       * over several lines */
#define LUSH_B 0x1F
typedef struct lush_p { const float* w[8]; const float *w_rb, *b_rb; int n, m; float x; } lush_p;
typedef struct { float* w[8]; float *w_rb, *b_rb; int n, m; float x; } lush_g;
const char* lush_why(void);
size_t lush_f(void* state, const int* adam_steps /* host, 3 */, const lush_g* g, unsigned long long seed,   // trailing
              long long n, double lr, size_t* bytes, lush_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
''')
    assert a.consts == {"LUSH_A": 7, "LUSH_B": 31}
    P = a.structs["lush_p"]
    assert a.structs["lush_g"] is P and [f[0] for f in P._fields_] == ["w", "w_rb", "b_rb", "n", "m", "x"]
    assert [f[1] for f in P._fields_] == [ctypes.c_void_p * 8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    v = ctypes.c_void_p
    assert a.protos == {"lush_why": ([], ctypes.c_char_p),
                        "lush_f": ([v, v, ctypes.POINTER(P), ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_double, v, v], ctypes.c_size_t)}


def test_product_refuses_cpu_tensors():
    from lush_nerf_amd import ops
    with pytest.raises(RuntimeError):
        ops.PackRays.apply(torch.zeros(4, 3, 2), 8, 8, 10.0, True, 0., 1.)


def test_product_does_not_import_the_oracle():
    for dp, dn, fn in os.walk(os.path.join(ROOT, "lush_nerf_amd")):
        for f in fn:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle|import_module\(.oracle|__import__\(.oracle", src, re.M), f


def test_generator_is_deterministic_and_reference_shaped():
    a, b = synth.all_weights(30, 5), synth.all_weights(30, 5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.size for v in a.values()) == 1301993          # flat gradient size
    assert a["mlp_coarse.pts_linears.5.weight"].shape == (256, 319)
    assert a["mlp_coarse.views_linears.0.weight"].shape == (128, 283)
    assert a["mlp_noise_coarse.pts_linears.0.weight"].shape == (128, 63)
    assert float(np.abs(a["mlp_rbk.r_linear.weight"]).max()) < 1.5e-6
    r1, r2 = synth.ray_batch(64, 1, step=0), synth.ray_batch(64, 1, step=1)
    assert not np.array_equal(r1["rays"], r2["rays"]) and r1["rays"].shape == (64, 3, 2)
    u = synth.uniform01(1000, 3)
    assert 0 <= u.min() and u.max() < 1


def test_model_mirror_has_reference_state_dict_keys():
    import argparse
    from lush_nerf_amd import model as M
    args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                              N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                              rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma",
                              render_rmnearplane=80)
    net = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4))
    sd = net.state_dict()
    assert len(sd) == 108 and sum(p.numel() for p in net.parameters()) == 1301993
    for k in ("mlp_coarse.pts_linears.0.weight", "mlp_fine.rgb_linear.bias", "mlp_noise_coarse.alpha_linear.weight",
              "blur_kernel_net.RBK.r_linear.weight", "dbk_view_embedding.view_embed_layer.weight",
              "mlp_rbk.view_embed_linears.3.bias", "blur_kernel_net.view_embed_layer.view_embed_layer.weight"):
        assert k in sd, k
    M.load_reference_weights(net, synth.all_weights(30, 2))
    assert np.array_equal(net.mlp_fine.pts_linears[5].weight.detach().numpy(),
                          synth.all_weights(30, 2)["mlp_fine.pts_linears.5.weight"])
    with pytest.raises(NotImplementedError):
        args2 = argparse.Namespace(**{**vars(args), "multires": 6})
        M.NeRFAll(args2, None)


def test_unbuilt_branches_are_refused_not_ignored():
    """Branches of the cited functions that this build does not implement raise (models/lushnerf.py:709-713 c2w_staticcam,
    :222-260 / :760 / :817 use_awp); `kernelpixel` / `allkernel` are dead parameters of the reference's render trio (never read
    in :679-866) and stay accepted."""
    import argparse
    from lush_nerf_amd import model as M
    args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                              N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                              rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma",
                              render_rmnearplane=80)
    net = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4))
    rays = torch.zeros(4, 3, 2)
    K = [[10., 0, 4], [0, 10., 4], [0, 0, 1]]
    for fn in (net.render_infer, net.render_train_scene, net.render_train_noise):
        with pytest.raises(NotImplementedError, match="c2w_staticcam"):
            fn(8, 8, K, 1024, rays=rays, use_viewdirs=True, c2w_staticcam=torch.eye(4)[:3], N_samples=8)
        with pytest.raises(NotImplementedError, match="use_awp"):
            fn(8, 8, K, 1024, rays=rays, use_viewdirs=True, use_awp=True, N_samples=8)
        with pytest.raises(RuntimeError, match="no CPU path"):      # accepted keywords reach the ops, which refuse CPU tensors
            fn(8, 8, K, 1024, rays=rays, use_viewdirs=True, kernelpixel=torch.ones(4), allkernel=1, N_samples=8)
    with pytest.raises(NotImplementedError, match="use_awp"):
        net._render_train_scene_packed(torch.zeros(4, 11), 1024, use_awp=True, N_samples=8)
    with pytest.raises(NotImplementedError):
        M.NeRF(use_awp=True)
    with pytest.raises(NotImplementedError):
        M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4, use_awp=True)


def test_flat_params_views():
    from lush_nerf_amd.trainer import FlatParams
    lin1, lin2 = torch.nn.Linear(3, 4), torch.nn.Linear(4, 2)
    w0 = lin1.weight.detach().clone()
    fp = FlatParams([list(lin1.parameters()), list(lin2.parameters()) + [lin1.weight]])   # alias is de-duplicated
    assert fp.numel == 3 * 4 + 4 + 4 * 2 + 2 and fp.segments == [(0, 16), (16, 26)]
    assert torch.equal(lin1.weight.detach(), w0)
    fp.param[:12] += 1.0
    assert torch.equal(lin1.weight.detach(), w0 + 1.0)
    (lin2(lin1(torch.ones(5, 3))).sum()).backward()
    assert float(fp.grad.abs().sum()) > 0 and lin1.weight.grad.data_ptr() == fp.grad.data_ptr()


_DIST_SCRIPT = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from lush_nerf_amd.trainer import FlatParams
from lush_nerf_amd import synth
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU(), torch.nn.Linear(16, 3))
fp = FlatParams([list(net.parameters())])
# every rank draws its own rays (disjoint seeds), SURVEY 8e
b = synth.ray_batch(32, seed=1000 + rank)
x = torch.from_numpy(b["rays"]).reshape(32, 6)
loss = ((net(x) - torch.from_numpy(b["target"])) ** 2).mean()
loss.backward()
local = fp.grad.clone()
dist.all_reduce(fp.grad)                       # the one collective of the step
gathered = [torch.zeros_like(local) for _ in range(world)]
dist.all_gather(gathered, local)
assert torch.allclose(fp.grad, sum(gathered)), "all-reduce != sum of per-rank gradients"
fp.param -= 0.1 * fp.grad / world              # redundant update on every rank
chk = [torch.zeros_like(fp.param) for _ in range(world)]
dist.all_gather(chk, fp.param)
assert all(torch.equal(chk[0], c) for c in chk), "replicas diverged"
assert not torch.equal(gathered[0], gathered[1]), "ranks must see different rays"
dist.destroy_process_group()
open(os.path.join(sys.argv[2], f"rank{rank}.ok"), "w").write("ok")     # stdout of the two ranks interleaves
'''


def test_data_parallel_allreduce_two_ranks_gloo(tmp_path):
    import socket
    script = tmp_path / "dp.py"
    script.write_text(_DIST_SCRIPT)
    with socket.socket() as sk:                      # a free rendezvous port (a fixed one can sit in TIME_WAIT)
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", port, str(script), ROOT, str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists(), r.stdout[-1000:]


_TRAINER_DIST_SCRIPT = r'''
"""Two gloo ranks drive the REAL Trainer.step control flow (zero-grad, micro-batch loop, one all-reduce of the flat
gradient, three Adam segments with grad_scale = 1/world, lr schedule); the HIP forward+backward of a slice is replaced
by injected rank-dependent gradients and the Adam kernel by its torch restatement, nothing else."""
import argparse, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from lush_nerf_amd import model as M, synth
from lush_nerf_amd.trainer import Trainer
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                          N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                          rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma", render_rmnearplane=80)
net = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4))
M.load_reference_weights(net, synth.all_weights(30, 50 + rank))       # ranks start DIFFERENT on purpose
calls = []

def fake_fwd_bwd(batch, a, b, i, draws, frac, force_naive):
    g = torch.from_numpy(synth.normal((tr.flat.numel,), 7000 + 10 * i + rank, a)) * frac
    if force_naive:                       # the reference leaves RBK + noise MLP with grad=None in the naive phase
        s1 = tr.flat.segments[1]
        g[s1[0]:s1[1]] = 0
    s2 = tr.flat.segments[2]
    g[s2[0]:s2[1]] = 0                    # mlp_noise_coarse.alpha_linear never receives a gradient
    tr.flat.grad += g
    calls.append((a, b, i, frac))
    return torch.tensor(float(rank + 1) * frac)

def torch_adam(param, grad, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    g = grad * grad_scale
    m.lerp_(g, 1 - beta1); v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = v.sqrt() / (1 - beta2 ** step) ** 0.5 + eps
    param.sub_((lr / (1 - beta1 ** step)) * m / denom)

tr = Trainer(net, 640, 1120, 1000.0, kernel_start_iter=1, distributed=True, micro_batch=8, step_fn=fake_fwd_bwd)
tr._adam = torch_adam
assert tr.world == 2 and tr.distributed
# construction broadcast: both ranks now hold rank 0's weights
w0 = torch.from_numpy(synth.all_weights(30, 50)["mlp_fine.pts_linears.3.weight"])
assert torch.equal(net.mlp_fine.pts_linears[3].weight.detach(), w0), "parameters were not broadcast from rank 0"
assert tr.replica_checksum() == 0.0
ref_p = tr.flat.param.clone(); ref_m = torch.zeros_like(ref_p); ref_v = torch.zeros_like(ref_p)
steps = [0, 0, 0]
batch = {"target": torch.zeros(40, 3)}
for i in range(3):                         # i = 0 is the naive phase (kernel_start_iter = 1)
    before = tr.flat.param.clone()
    lr_used = tr.lr()
    loss = tr.step(batch, i)
    assert [c[:2] for c in calls[-5:]] == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 40)], calls[-5:]      # micro-batches of 8 input rays
    # what the reference's DataParallel computes: gradient of the mean loss over the global batch = mean of rank grads
    gsum = torch.zeros(tr.flat.numel)
    for r in range(world):
        for a, b in ((0, 8), (8, 16), (16, 24), (24, 32), (32, 40)):
            g = torch.from_numpy(synth.normal((tr.flat.numel,), 7000 + 10 * i + r, a)) * ((b - a) / 40)
            gsum += g
    if i < 1:
        s1 = tr.flat.segments[1]; gsum[s1[0]:s1[1]] = 0
    s2 = tr.flat.segments[2]; gsum[s2[0]:s2[1]] = 0
    assert torch.allclose(tr.flat.grad, gsum, rtol=1e-5, atol=2e-6), "flat gradient != sum over ranks"   # fp32 association differs
    active = [True, i >= 1, False]
    for s, (a, b) in enumerate(tr.flat.segments):
        if active[s]:
            steps[s] += 1
            torch_adam(ref_p[a:b], gsum[a:b], ref_m[a:b], ref_v[a:b], lr_used, steps[s], grad_scale=1.0 / world)
    # Adam's first steps move a parameter by ~lr * g / |g|: on the one-in-a-million element whose summed gradient is within
    # fp32 summation-order noise of zero that is ill-conditioned (the sum is taken in another order here than in the
    # trainer), so a handful of the 1.3 M elements may differ; every other one must match
    bad = ~torch.isclose(tr.flat.param, ref_p, rtol=1e-5, atol=1e-7)
    assert int(bad.sum()) <= 8 and float((tr.flat.param - ref_p).abs().max()) < 2e-3, f"step {i}: parameters != Adam on the mean gradient ({int(bad.sum())} elements)"
    s1, s2 = tr.flat.segments[1], tr.flat.segments[2]
    assert torch.equal(tr.flat.param[s2[0]:s2[1]], before[s2[0]:s2[1]]), "dead segment was stepped"
    if i < 1:
        assert torch.equal(tr.flat.param[s1[0]:s1[1]], before[s1[0]:s1[1]]), "RBK/noise segment stepped in the naive phase"
    else:
        assert not torch.equal(tr.flat.param[s1[0]:s1[1]], before[s1[0]:s1[1]])
    assert tr.replica_checksum() == 0.0, "replicas diverged"
    chk = [torch.zeros_like(tr.flat.param) for _ in range(world)]
    dist.all_gather(chk, tr.flat.param)
    assert torch.equal(chk[0], chk[1])
assert tr.steps == [3, 2, 0] and tr.global_step == 3
# The reference's DataParallel semantics, stated directly: two ranks of N rays == ONE rank stepping the concatenated 2N batch
# (run_lushnerf.py:348, 652-661: the loss is a mean over the gathered batch).  Global slice [a, b) of the 80-ray batch is
# rank a // 40's slice [a % 40, b % 40): the injected gradient of that slice, weighted by its share of 80 rays.
if rank == 0:
    net1 = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4))
    M.load_reference_weights(net1, synth.all_weights(30, 50))

    def fake_single(batch, a, b, i, draws, frac, force_naive):
        g = torch.from_numpy(synth.normal((tr1.flat.numel,), 7000 + 10 * i + a // 40, a % 40)) * frac
        if force_naive:
            s1 = tr1.flat.segments[1]
            g[s1[0]:s1[1]] = 0
        s2 = tr1.flat.segments[2]
        g[s2[0]:s2[1]] = 0
        tr1.flat.grad += g
        return torch.tensor(frac)
    tr1 = Trainer(net1, 640, 1120, 1000.0, kernel_start_iter=1, distributed=False, micro_batch=8, step_fn=fake_single)
    tr1._adam = torch_adam
    for i in range(3):
        tr1.step({"target": torch.zeros(80, 3)}, i)
        if i == 2:      # gradient of the last step: sum over ranks / world == the single rank's gradient
            assert torch.allclose(tr.flat.grad / world, tr1.flat.grad, rtol=2e-4, atol=2e-6), "2-rank gradient != 1-rank gradient on the concatenated batch"
    bad = ~torch.isclose(tr.flat.param, tr1.flat.param, rtol=1e-5, atol=1e-7)
    assert int(bad.sum()) <= 8 and float((tr.flat.param - tr1.flat.param).abs().max()) < 2e-3, "2 ranks x N rays != 1 rank x 2N rays"
dist.destroy_process_group()
open(os.path.join(sys.argv[2], f"trainer_rank{rank}.ok"), "w").write("ok")
'''


def test_trainer_step_two_ranks_gloo(tmp_path):
    """SURVEY 8e / BASELINE config 4 on CPU: the real Trainer.step over gloo, world size 2."""
    import socket
    script = tmp_path / "dp_trainer.py"
    script.write_text(_TRAINER_DIST_SCRIPT)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", port, str(script), ROOT, str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "trainer_rank0.ok").exists() and (tmp_path / "trainer_rank1.ok").exists()


def test_bench_refuses_wrong_world(tmp_path):
    """bench.py --gpus N must never print an N-GPU line from fewer ranks: it self-launches N ranks when no launcher set
    WORLD_SIZE (and fails when the devices are missing) and refuses a launcher whose world size differs."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=300)
    if torch.cuda.device_count() < 2:
        assert r.returncode != 0 and "only" in (r.stdout + r.stderr) and '"metric"' not in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stdout + r.stderr) and '"metric"' not in r.stdout


def test_bench_dump_outputs_writes_float_arrays(tmp_path, monkeypatch):
    """--dump-outputs DIR: one DIR/<name>.npy per array, float32 (float64 kept), a 0-d loss as one element; over the byte budget
    a fixed sample of rows, the same in every call."""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    d = tmp_path / "out"
    bench.dump_outputs(str(d), {"loss": torch.tensor(0.25), "params": torch.arange(6, dtype=torch.float16).reshape(2, 3),
                                "grad": torch.ones(4, dtype=torch.float64)})
    loss, params, grad = (np.load(d / f"{n}.npy") for n in ("loss", "params", "grad"))
    assert loss.dtype == np.float32 and loss.tolist() == [0.25]
    assert params.dtype == np.float32 and params.shape == (2, 3) and params[1, 2] == 5.0
    assert grad.dtype == np.float64 and grad.shape == (4,)
    big = {"rows": torch.arange(4000, dtype=torch.float32).reshape(1000, 4), "loss": torch.tensor(1.0)}
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    for sub in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / sub), big)
    r1, r2 = (np.load(tmp_path / sub / "rows.npy") for sub in ("big1", "big2"))
    assert 200 < r1.shape[0] <= 250 and r1.shape[1] == 4 and np.array_equal(r1, r2)      # <= the budget, the same rows each time
    assert np.all(np.diff(r1[:, 0]) > 0) and np.all(r1[:, 0] % 4 == 0)      # whole rows, in row order
    assert np.load(tmp_path / "big1" / "loss.npy").tolist() == [1.0]
    # the option parses (the run then stops at the --gpus check, before anything touches a device)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path / "x"), "--gpus", "0"],
                       capture_output=True, text=True, timeout=300)
    assert "--gpus must be >= 1" in (r.stderr + r.stdout), r.stderr[-400:]


def test_bench_plain_run_refuses_what_only_full_measures():
    """A plain bench.py run measures the headline alone: an option that asks for one of --full's passes is refused before anything
    touches a device, not silently dropped; with --full the same options parse (the run then stops at the --gpus check)."""
    bench = os.path.join(ROOT, "bench.py")
    for opt in (["--also", "2,2"], ["--extra", "C1"], ["--sustained", "3"]):
        r = subprocess.run([sys.executable, bench, *opt], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and opt[0] in r.stderr and "--full" in r.stderr and '"metric"' not in r.stdout, r.stderr[-400:]
    r = subprocess.run([sys.executable, bench, "--full", "--also", "2,2", "--extra", "C1", "--sustained", "3", "--gpus", "0"],
                       capture_output=True, text=True, timeout=300)
    assert "--gpus must be >= 1" in (r.stderr + r.stdout), r.stderr[-400:]
    # asking for none of them is a plain run (the traffic child's own tail: tests above)
    r = subprocess.run([sys.executable, bench, "--also=", "--extra=", "--sustained", "0", "--gpus", "0"], capture_output=True, text=True, timeout=300)
    assert "--gpus must be >= 1" in (r.stderr + r.stdout), r.stderr[-400:]


def test_trainer_lr_follows_reference_loop():
    """run_lushnerf.py:675-685, 788: step g runs with the rate computed from global_step g-1."""
    from oracle import lush_oracle as O
    _, tr = _small_trainer(1)
    used = []
    for g in range(6):
        used.append(tr.lr())
        tr.global_step += 1
    assert used == O.lr_schedule(6)
    tr.global_step = 250000
    assert abs(tr.lr() - O.lr_at(249999)) < 1e-18 and abs(tr.lr() / 5e-5 - 1) < 1e-4


def _small_trainer(seed=0):
    import argparse
    from lush_nerf_amd import model as M
    from lush_nerf_amd.trainer import Trainer
    args = argparse.Namespace(blur_model_type="dpnerf", multires=10, multires_views=4, i_embed=0, use_viewdirs=True,
                              N_importance=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256,
                              rgb_activate="sigmoid", sigma_activate="relu", tone_mapping_type="gamma",
                              render_rmnearplane=80)
    net = M.NeRFAll(args, M.RBK(30, 64, 4, 64, 1, 32, 1, 32, 1, 32, 3, 3, [4], True, 0.1, 4))
    M.load_reference_weights(net, synth.all_weights(30, seed))
    return net, Trainer(net, 640, 1120, 1000.0)


def test_checkpoint_interop_with_reference_layout(tmp_path):
    """the file we write has exactly the reference's keys/shapes, its optimizer state loads
    into a torch.optim.Adam built the way the reference builds it, and a round trip restores everything."""
    from lush_nerf_amd import checkpoint as CK
    g = util.golden("checkpoint_layout")
    net, tr = _small_trainer(3)
    tr.steps = [7, 5, 0]
    tr.global_step = 7
    tr.m.copy_(torch.from_numpy(synth.normal((tr.m.numel(),), 1)))
    tr.v.copy_(torch.from_numpy(synth.uniform((tr.v.numel(),), 0, 1, 2)))
    path = str(tmp_path / "000007.tar")
    tr.live.dense_now, tr.live.dense_steps, tr.live_share = True, 5, 0.73          # where the live-point policy stands (round 6: saved too)
    CK.save_checkpoint(path, net, 7, tr)
    ck = torch.load(path, weights_only=False)
    # the reference's three keys (all its loader reads, run_lushnerf.py:373-389) + one of ours it never looks at
    assert set(ck) == {"global_step", "network_state_dict", "optimizer_state_dict", "lush_live_policy"}
    assert list(ck["network_state_dict"].keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in ck["network_state_dict"].values()] == [str(s) for s in g["shapes"]]
    osd = ck["optimizer_state_dict"]
    assert [len(gr["params"]) for gr in osd["param_groups"]] == [int(x) for x in g["group_sizes"]]
    # loads into an optimizer constructed exactly as run_lushnerf.py:359-371 does
    noise = list(net.mlp_noise_coarse.parameters())
    ids = set(map(id, noise))
    base = [p for p in net.parameters() if id(p) not in ids]
    assert [p.numel() for p in base] == [int(x) for x in g["group0_numel"]]
    assert [p.numel() for p in noise] == [int(x) for x in g["group1_numel"]]
    opt = torch.optim.Adam([{"params": base}, {"params": noise, "lr": 5e-4}], lr=5e-4)
    opt.load_state_dict(osd)
    st = opt.state[net.mlp_fine.pts_linears[3].weight]
    off = (net.mlp_fine.pts_linears[3].weight.data_ptr() - tr.flat.param.data_ptr()) // 4
    assert torch.equal(st["exp_avg"].reshape(-1), tr.m[off:off + 65536]) and float(st["step"]) == 7
    assert net.mlp_noise_coarse.alpha_linear.weight not in opt.state            # never stepped -> no state
    # round trip into a fresh model / trainer
    net2, tr2 = _small_trainer(4)
    assert CK.load_checkpoint(path, net2, tr2) == 7
    for (k, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a, b), k
    assert tr2.steps == [7, 5, 0] and tr2.global_step == 7
    assert (tr2.live.dense_now, tr2.live.dense_steps, tr2.live_share, tr2.live.in_flight) == (True, 5, 0.73, [])      # a resumed run chooses as the uninterrupted one
    a, b = tr.flat.segments[1]
    assert torch.equal(tr2.m[:b], tr.m[:b]) and torch.equal(tr2.v[:b], tr.v[:b])
    # the reference resumes with the rate its optimizer was saved with (lr of global_step 7), for one step
    assert tr2._lr_next == pytest.approx(5e-4 * 0.1 ** (7 / 250000), rel=1e-12)
    # without a trainer the file still carries the reference's two parameter groups (its loader calls
    # optimizer.load_state_dict unconditionally, run_lushnerf.py:386) and global_step is restored
    path2 = str(tmp_path / "000009.tar")
    CK.save_checkpoint(path2, net, 9)
    ck2 = torch.load(path2, weights_only=False)
    assert set(ck2) == {"global_step", "network_state_dict", "optimizer_state_dict"}
    opt2 = torch.optim.Adam([{"params": base}, {"params": noise, "lr": 5e-4}], lr=5e-4)
    opt2.load_state_dict(ck2["optimizer_state_dict"])
    assert len(opt2.state) == 0
    net3, tr3 = _small_trainer(5)
    tr3.m.fill_(1.0); tr3.steps = [4, 4, 0]
    tr3.live.dense_now, tr3.live_share = True, 0.9
    assert CK.load_checkpoint(path2, net3, tr3) == 9
    assert (tr3.live.dense_now, tr3.live_share) == (False, None)                   # a file without the key: the policy starts over
    assert tr3.global_step == 9 and tr3.steps == [0, 0, 0] and float(tr3.m.abs().max()) == 0.0


def test_sample_merge_refuses_sizes_beyond_its_lds_arrays():
    """include/lush_march.h states the limits of lush_sample_merge (3 <= S <= 256, S + Ni <= 512: fixed LDS arrays of the
    one-wavefront-per-ray kernel); beyond them the entry point must refuse BEFORE launching anything (checked here
    without a GPU: the refusal happens on the host) and say why."""
    from lush_nerf_amd import lib
    l = lib.load()
    for S, Ni in ((257, 64), (2, 64), (256, 257), (300, 300), (64, 0)):
        rc = l.lush_sample_merge(None, None, 4, S, Ni, None, None, None, None, None, None)
        assert rc != 0, (S, Ni)
        assert b"lush_sample_merge" in l.lush_last_error(), l.lush_last_error()


def test_mlp_launch_refuses_more_points_than_its_32_bit_offsets_reach():
    """The 64-points-per-wave kernels address per-point rows by 32-bit byte offsets from a scalar base: R * S >= 2^27 points in
    one launch must be refused on the host, before anything is launched (include/lush_march.h, LIMIT at lush_mlp_fwd)."""
    from lush_nerf_amd import lib
    l = lib.load()
    st = lib.MlpParams()
    one = ctypes.c_void_p(8)        # any non-null pointer: the refusal comes before it is looked at
    rc = l.lush_mlp_fwd(0, 17, 1, one, one, 1 << 20, 128, one, ctypes.byref(st), one, one, 0, None)
    assert rc != 0 and b"2^27" in l.lush_last_error(), l.lush_last_error()
    rc = l.lush_mlp_bwd_chain(0, 17, 17, one, one, 1 << 20, 128, one, ctypes.byref(st), one, one, one, one, 0, None)
    assert rc != 0 and b"2^27" in l.lush_last_error(), l.lush_last_error()


def test_march_is_refused_when_it_is_sized_not_half_way_through_its_backward():
    """A march with R * (N_samples + N_importance) >= 2^27 points cannot run (no MLP launch, nor lush_live_compact, takes that many):
    lush_march_workspace_bytes says so (0) for every form of the backward, instead of sizing a workspace whose forward runs and
    whose backward then fails (advisor, round 5).  And the live-point march with a fine pass keeps ONE stash region for both passes:
    its workspace is smaller than the dense form's by the coarse pass's stash."""
    from lush_nerf_amd import lib
    l = lib.load()
    mk = lambda R, S, Ni, variant: lib.MarchCfgC(R, S, Ni, 1.0, 1.0, 0, 0, 0.0, 17, 17, variant, 0)
    for variant in (0, lib.VARIANT_DENSE_BWD):
        assert l.lush_march_workspace_bytes(ctypes.byref(mk(1 << 20, 64, 64, variant))) == 0, variant      # exactly 2^27 points
        assert l.lush_march_workspace_bytes(ctypes.byref(mk((1 << 20) - 1, 64, 64, variant))) > 0, variant
    live, dense = (l.lush_march_workspace_bytes(ctypes.byref(mk(20480, 64, 64, v))) for v in (0, lib.VARIANT_DENSE_BWD))
    stash_c = l.lush_mlp_stash_bytes(0, 17, 17, 20480 * 64)
    assert stash_c > 5e9 and 0 < dense - live and abs((dense - live) - (stash_c - 20 * 20480 * 128)) < 0.02 * stash_c, (live, dense, stash_c)
    off_c, off_f, n = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    cfg = mk(20480, 64, 64, 0)
    assert l.lush_march_view(ctypes.byref(cfg), lib.VIEW_STASH_COARSE, ctypes.byref(off_c), ctypes.byref(n)) == 0
    assert l.lush_march_view(ctypes.byref(cfg), lib.VIEW_STASH_FINE, ctypes.byref(off_f), ctypes.byref(n)) == 0
    assert off_c.value == off_f.value


def test_bench_self_launch_builds_the_documented_command(monkeypatch):
    """`python bench.py --gpus N` without a launcher starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` as a CHILD (never an exec) and exits with its code; the
    subprocess call is replaced here, nothing is launched."""
    import argparse
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench.self_launch(argparse.Namespace(gpus=4))
    assert e.value.code == 7                                  # the child's exit code
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "5", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # fewer devices than ranks: refused before anything is started
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    seen.clear()
    with pytest.raises(SystemExit) as e:
        bench.self_launch(argparse.Namespace(gpus=4))
    assert "only 1 GPU" in str(e.value.code) and not seen


def test_bench_traffic_child_profiles_the_same_workload():
    """Advisor (round 4): the child runs behind roofline.traffic (rocprofv3 --pmc passes of `this very command`) dropped the size
    arguments and profiled the default workload whatever the parent timed.  They are forwarded now, with mode, variant and library."""
    import argparse
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    a = argparse.Namespace(planes="h,h", config="C2", variant=64, n_rand=2048, n_samples=128, n_importance=128, micro_batch=1024, so="/x/y.so")
    t = bench.traffic_child_args(a)
    val = lambda k: t[t.index(k) + 1]
    assert (val("--n-rand"), val("--n-samples"), val("--n-importance"), val("--micro-batch")) == ("2048", "128", "128", "1024")
    assert val("--planes") == "h,h" and val("--variant") == "64" and val("--so") == "/x/y.so" and val("--steps") == "2"
    assert "--no-traffic" in t and "--no-kernel-pass" in t and "--no-cpu-baseline" in t and "--no-dense" in t and val("--sustained") == "0"      # no recursion, nothing else timed
    # and the parser accepts exactly that tail
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *[x for x in t if x != "/x/y.so" and x != "--so"], "--gpus", "0"],
                       capture_output=True, text=True, timeout=300)
    assert "--gpus must be >= 1" in (r.stderr + r.stdout), r.stderr[-400:]


def test_quoted_numbers_match_their_sources():
    """Every number in the marked blocks of DESIGN.md / README.md is what tools/quoted_numbers.py derives from the driver's BENCH_rNN.json
    (the file the status block names) and the committed profiles/ artefacts: no hand-edited figures."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quoted_numbers.py"), "--check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # ... and the driver file quoted is the one that was the newest when this round's profiles were made: round N's profiles
    # (profiles/rNN_bench_line.json) go with BENCH_r(N-1).json -- round 5 quoted BENCH_r04.json beside r05 profiles (verdict item 7); a
    # BENCH_rNN.json the driver adds AFTER the round does not make the committed text stale
    import glob, re
    tags = sorted(int(os.path.basename(f)[1:3]) for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_line.json")))
    for doc in ("README.md", "DESIGN.md"):
        m = re.search(r"the driver's own run, `BENCH_r(\d\d)\.json`", open(os.path.join(ROOT, doc)).read())
        assert m, doc
        if os.path.exists(os.path.join(ROOT, "BENCH_r%02d.json" % (tags[-1] - 1))):
            assert int(m.group(1)) == tags[-1] - 1, (doc, m.group(1), tags[-1])


def test_live_point_policy_state_machine():
    """LivePolicy.decide (no GPU: the decision logic alone): live until a share arrives; dense above MAX_SHARE with one
    live probe every PROBE_EVERY steps; back to live below MIN_SHARE (hysteresis); "live" / "dense" override."""
    from lush_nerf_amd.trainer import LivePolicy
    t = LivePolicy("cpu")
    assert (t.mode, t.share, t.dense_now, t.dense_steps) == ("auto", None, False, 0)
    t.PROBE_EVERY = 4
    assert t.decide() is False                                    # nothing known yet
    t.share = 0.5
    assert t.decide() is False
    t.share = 0.9
    seq = [t.decide() for _ in range(9)]
    assert seq == [True, True, True, True, False, True, True, True, False], seq      # every fourth dense step is a live probe
    assert (t.MIN_SHARE, t.MAX_SHARE) == (0.65, 0.70)             # inside the measured break-even band 0.69 .. 0.76 (profiles/r05_live_points.md)
    t.share = 0.67                                                # between MIN and MAX: stays dense
    assert t.decide() is True
    t.share = 0.5
    assert t.decide() is False and t.dense_now is False
    t.share = 0.67                                                # ... and stays live until it exceeds MAX again
    assert t.decide() is False
    t.mode, t.share = "dense", 0.1
    assert t.decide() is True
    t.mode, t.share = "live", 0.99
    assert t.decide() is False


class _Event:
    """Stands in for torch.cuda.Event in a LivePolicy on CPU tensors."""
    made = []

    def __init__(self):
        self.recorded = self.waited = False
        _Event.made.append(self)

    def record(self):
        self.recorded = True

    def synchronize(self):
        assert self.recorded
        self.waited = True


def test_live_point_policy_reads_a_fixed_lag():
    """The choice for step n is taken from the counts of step n - LAG, whatever has or has not arrived: choose() WAITS for that
    snapshot (event.synchronize) and leaves younger ones alone, so a seeded run makes the same choices every time (advisor, round 5:
    event.query() made them depend on host / device timing).  Counts a caller accumulated in a buffer of its own start a new series
    instead of being subtracted from the policy's -- and the policy's own series goes on where it was when its accumulator returns
    (the parent started it over from zero: 160 / 600 instead of 40 / 200)."""
    from lush_nerf_amd.trainer import LivePolicy
    t = LivePolicy("cpu", event=_Event)
    t.mode = "live"                                                # (the readings are the subject: every step is a live one)
    evs = _Event.made = []
    other = torch.zeros(4, dtype=torch.int64)                      # a caller's accumulator

    def snap(counts, acc=None):
        (t.acc if acc is None else acc).copy_(torch.tensor(counts))
        assert t.snapshot(acc) is True and t.in_flight[-1][2] == t.step

    assert t.choose() is False and t.step == 1
    snap([40, 100, 10, 100])
    t.choose()
    assert t.step == 2 and t.share is None and not evs[0].waited   # step 1's counts are not step 2's business yet
    snap([100, 200, 20, 200])
    t.choose()
    assert t.step == 3 and evs[0].waited and not evs[1].waited and t.share == 0.25      # step 3 decides on step 1: (40 + 10) / 200
    t.choose()
    assert t.step == 4 and evs[1].waited and t.share == (60 + 10) / 200
    snap([5, 10, 5, 10], acc=other)                                # a caller's accumulator: a new series from zero, no negative delta
    t.choose()
    snap([15, 20, 15, 20], acc=other)
    t.choose()
    assert t.step == 6 and t.share == 0.5 and other.data_ptr() in t._prev and not evs[3].waited
    t.choose()
    assert t.step == 7 and t.share == 1.0 and not t.in_flight
    t.choose()
    snap([130, 300, 30, 300])                                      # the policy's own accumulator again: on from [100, 200, 20, 200]
    t.choose()
    t.choose()
    assert t.step == 10 and t.share == (30 + 10) / (100 + 100) and not t.in_flight
    assert set(t._prev) == {t.acc.data_ptr()}                      # (one caller's reading is kept at the most: a fresh tensor per step is fine)


def test_live_point_policy_keeps_at_most_lag_plus_one_snapshot_in_flight():
    """A snapshot is enqueued for exactly the steps whose choice the policy took and answered "live", once: 100 rounds of "take the
    choice, snapshot if live" at a share above MAX_SHARE (dense steps and probes) never leave more than LAG + 1 in flight and never
    have a snapshot refused; a request on behalf of a step the policy was not asked about (a small launch: the parent filled the
    ring with those and then dropped the first counted step's) leaves nothing behind."""
    from lush_nerf_amd.trainer import LivePolicy
    t = LivePolicy("cpu", event=_Event)
    t.PROBE_EVERY = 4
    assert t.snapshot() is False and not t.in_flight               # before any choice
    chosen = []
    for n in range(100):
        if n % 7 == 3:                                             # a step that does not consult the policy
            before = list(t.in_flight)
            assert t.snapshot() is False and t.in_flight == before
            continue
        chosen.append(t.choose())
        if not chosen[-1]:
            t.acc += torch.tensor([90, 100, 95, 100])              # a live march: 185 of 200 points live
            assert t.snapshot() is True                            # never refused ...
            assert t.snapshot() is False                           # ... and one per step
        assert len(t.in_flight) <= t.LAG + 1
    # live until step 1's share arrives at step 3, then dense with every fourth dense step a live probe
    assert chosen == [False, False, True] + [k % 4 != 0 for k in range(1, len(chosen) - 2)], chosen
    assert t.share == 0.925 and t.step == len(chosen) == 86


def test_live_point_policy_restore_starts_over_from_the_present_counts():
    """LivePolicy.load_state (checkpoint load): the snapshots in flight are dropped, the step counter restarts and the accumulator's
    present value is the previous reading, so the first share after a restore covers the steps after it only."""
    from lush_nerf_amd.trainer import LivePolicy
    t = LivePolicy("cpu", event=_Event)
    for counts in ([40, 100, 10, 100], [100, 200, 20, 200]):
        t.choose()
        t.acc.copy_(torch.tensor(counts))
        assert t.snapshot()
    assert len(t.in_flight) == 2 and t.step == 2
    t.load_state({"policy": "dense", "dense_now": False, "dense_steps": 3, "live_share": 0.5})
    assert t.in_flight == [] and t.step == 0 and t.counts() == [100, 200, 20, 200]
    assert t.state() == {"policy": "auto", "dense_now": False, "dense_steps": 3, "live_share": 0.5}      # (the caller's own mode stays)
    t.choose()
    t.acc += torch.tensor([30, 100, 30, 100])
    assert t.snapshot()
    t.choose()
    assert t.share == 0.5
    t.choose()
    assert t.step == 3 and t.share == 60 / 200
    t.load_state(None)                                             # a file without the key: the policy starts over
    assert (t.dense_now, t.dense_steps, t.share, t.step, t.in_flight) == (False, 0, None, 0, [])


def test_kernel_sources_have_one_compile_time_form():
    """Every preprocessor conditional in the kernel sources and the public header is an include guard, `__cplusplus`, `LUSH_CLOCK`
    (lush_common.h: three macros, empty in the product) or an `#ifndef X` / `#define X value` default that selects no code.  Timing
    ablations and profiling counters do not live inside the product kernels (tools/micro/ prototypes)."""
    import glob
    csrc = os.path.join(ROOT, "lush_nerf_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))) + [os.path.join(ROOT, "include", "lush_march.h")]
    assert len(files) > 10, files
    bad, seen = [], 0
    for f in files:
        lines = open(f).read().split("\n")
        for k, line in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            seen += 1
            kind, cond = m.group(1), re.sub(r"//.*|/\*.*", "", m.group(2)).strip()
            if kind == "ifdef" and cond in ("__cplusplus", "LUSH_CLOCK"):
                continue
            if kind == "ifndef" and re.fullmatch(r"\w+", cond) and k + 1 < len(lines) and re.match(r"\s*#\s*define\s+%s\b" % cond, lines[k + 1]):
                continue      # an include guard or a tuning default
            bad.append(f"{os.path.relpath(f, ROOT)}:{k + 1}: {line.strip()}")
    assert seen >= 10, seen      # (the scan found the conditionals that are allowed: it is reading the right files)
    assert not bad, "\n".join(bad)


def test_weight_gradient_launch_plan_is_pinned():
    """How a backward cuts up its grouped weight-gradient launch (plan_dw_group in lush_abi.hip, a third of the headline step) decided
    on the host from the job table, the padded point count, live or dense, the variant word and the CU count: lush_debug_dw_plan
    returns it without a device.  Every word equals tests/dw_plan_expected.json, recorded from the dispatch code as it stood before
    it was taken apart (a scratch hook in front of its launch_dw_group call); null there = the call is refused (a live launch of the
    noise net or with an older-kernel variant bit).  Plus what holds without a table."""
    import itertools
    import json
    l = lib.load()
    want = json.load(open(os.path.join(ROOT, "tests", "dw_plan_expected.json")))
    MAX_PTS = 262144                                      # LUSH_DW_PERJOB_MAX_PTS
    variants = (0, lib.VARIANT_HEAD_KERNEL, lib.VARIANT_PE_ROWS, lib.VARIANT_DW_SPLIT, lib.VARIANT_DW_WALK)
    cases = list(itertools.product((0, 1), ((17, 17), (2, 17), (2, 2), (1, 1)), (96, 4096, 32768, 262144, 262400, 526336, 2621440), variants, (0, 1), (256, 40)))
    assert len(want) == len(cases) == 1120
    forms = set()
    for net, (pf, pb), P, var, live, cus in cases:
        key = f"{net},{pf},{pb},{P},{var},{live},{cus}"
        o = (ctypes.c_longlong * 80)()
        rc = l.lush_debug_dw_plan(net, pf, pb, P, var, live, cus, o)
        if want[key] is None:
            assert rc != 0 and live and (net == 1 or var), key
            continue
        assert rc == 0, (key, l.lush_last_error())
        n, per_job, Ppad, pps, gx, gy, cursors = o[:7]
        got = list(o)[:7 + 6 * n] + [o[79]]
        assert got == want[key], (key, got, want[key])
        assert all(w == -1 for w in list(o)[7 + 6 * n:79]), key
        jobs = [list(o)[7 + 6 * i:13 + 6 * i] for i in range(n)]      # n_out, k_in, k2_in, pe_mode, pps, first
        first = [j[5] for j in jobs] + [o[79]]
        assert Ppad == (P + 255) // 256 * 256 and pps % 32 == 0 and all(j[4] % 32 == 0 for j in jobs), key
        assert gy == (n if per_job == 1 else 1) and cursors == (per_job == 3), key
        if per_job in (2, 3):
            assert first[0] == 0 and first[n] == gx and all(b > a for a, b in zip(first, first[1:])), (key, first)      # every job has a workgroup
        assert (per_job == 1) == (Ppad <= MAX_PTS and not live), key
        if per_job == 3:
            assert Ppad > MAX_PTS and not var & lib.VARIANT_DW_WALK and Ppad % 256 == 0, key
        forms.add(per_job)
    assert forms == {0, 1, 2, 3}      # the cases reach every form
    o = (ctypes.c_longlong * 80)()
    assert l.lush_debug_dw_plan(0, 3, 3, 4096, 0, 0, 256, o) != 0 and b"three planes" in l.lush_last_error()      # one launch per layer: no plan
    assert l.lush_debug_dw_plan(0, 17, 17, 1 << 27, 0, 0, 256, o) != 0 and l.lush_debug_dw_plan(0, 17, 17, 4096, 0, 0, 0, o) != 0


MARCH_VIEWS = ("VIEW_Z", "VIEW_RAW", "VIEW_WEIGHTS", "VIEW_Z_COARSE", "VIEW_STASH_COARSE", "VIEW_STASH_FINE", "VIEW_LIVE_COUNTS")


def march_layout_rows():
    """{case key: [workspace bytes, trunk form, coarse trunk form, then (return code, offset, bytes) of each of MARCH_VIEWS]} over
    the grid of test_march_layout_is_pinned, from the loaded library (a view that is refused reads (code, 0, 0))."""
    import itertools
    l, h = lib.load(), lib.PLANES_F16
    shapes = ((7, 64, 64), (523, 44, 44), (20480, 64, 64), (4096, 64, 0), (1 << 20, 64, 64))
    planes = ((h, h), (2, h), (2, 2), (3, 3), (h, 0))
    variants = (0, lib.VARIANT_DENSE_BWD, lib.VARIANT_FWD_HALF, lib.VARIANT_PE_ROWS)
    extras = (0, lib.MARCH_FWD_LIST_KEPT, lib.MARCH_COARSE_TRUNK, lib.MARCH_FWD_LIST_KEPT | lib.MARCH_COARSE_TRUNK)
    rows = {}
    for (R, S, ni), (pf, pb), var, extra, same in itertools.product(shapes, planes, variants, extras, (0, 1)):
        c = lib.MarchCfgC(R, S, ni, 1.0, 1.0, 0, 0, -1.0, pf, pb, var | extra, same)      # (the other fields: tests/test_coarse_trunk._cfg)
        row = [int(l.lush_march_workspace_bytes(ctypes.byref(c))), int(l.lush_march_trunk_form(ctypes.byref(c))),
               int(l.lush_march_coarse_trunk_form(ctypes.byref(c)))]
        for which in MARCH_VIEWS:
            off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
            rc = int(l.lush_march_view(ctypes.byref(c), getattr(lib, which), ctypes.byref(off), ctypes.byref(nb)))
            row += [rc, off.value, nb.value] if rc == 0 else [rc, 0, 0]
        rows[f"{R},{S},{ni},{pf},{pb},{var},{extra},{same}"] = row
    return rows


def test_march_layout_is_pinned():
    """Where every region of the march's workspace lies (layout() in lush_march_abi.hip), as far as the library tells without a
    device: lush_march_workspace_bytes, the two form predicates and all seven lush_march_view answers, over shapes x plane codes x
    kernel variants x the two bits of the word that are no kernel bits x one net or two.  Every row equals
    tests/march_layout_expected.json, recorded with march_layout_rows() above from a library built from the sources as they stood
    before layout() was rewritten around one record per pass -- not from the code under test.  The file holds each distinct row once
    ("rows") and, per case, its number ("cases")."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "march_layout_expected.json")))
    got = march_layout_rows()
    assert len(got) == len(want["cases"]) == 800 and list(got) == list(want["cases"])
    for key, row in got.items():
        assert row == want["rows"][want["cases"][key]], (key, row, want["rows"][want["cases"][key]])
    # the grid reaches every form: the 2^27-point shape is refused everywhere (no bytes, no form, no view), the trunk form, the
    # coarse trunk form, the live-point marches (the ones with a LIVE_COUNTS view)
    rows = list(got.values())
    refused = [r for r in rows if r[0] == 0]
    assert len(refused) == 160 and all(r[1] == r[2] == 0 and all(r[3 + 3 * k] != 0 for k in range(7)) for r in refused)
    assert sum(r[1] for r in rows) == 32 and sum(r[2] for r in rows) == 12
    assert sum(1 for r in rows if r[0] and r[3 + 3 * MARCH_VIEWS.index("VIEW_LIVE_COUNTS")] == 0) == 96
    assert len({tuple(r) for r in rows}) == len(want["rows"]) == 63
