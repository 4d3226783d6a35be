"""Loader / builder for liblush_march.so (the hand-written HIP kernels + C ABI).

The shared object is built IN-TREE by ``build()`` (hipcc --offload-arch=gfx950)
and loaded with ctypes.  There is no fallback: if the library is missing or a
call fails the product raises.  Signatures, structs and constants are read from include/lush_march.h (abi.py), the one
later entry point from the second contract header include/lush_subframe.h, the trunk form's from the third, include/lush_live_fwd.h,
the coarse pass's trunk form from the fourth, include/lush_live_coarse.h.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Sequence

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO_PATH = os.path.join(HERE, "liblush_march.so")      # (developer tools load another build with use_library(path) BEFORE load())
SOURCES = ["lush_march.hip", "lush_mlp.hip", "lush_mlp_chain.hip", "lush_mlp_wide.hip", "lush_mlp_wide_bwd.hip", "lush_abi.hip", "lush_march_abi.hip", "lush_field.hip",
           "lush_rays.hip", "lush_rbk.hip", "lush_image.hip", "lush_step.hip"]
HEADERS = ["lush_common.h", "lush_composite.h", "lush_rays.h", "lush_mlp.h", "lush_mlp_dev.h", "lush_mlp_wide.h", "lush_host.h", os.path.join("..", "..", "include", "lush_live_coarse.h"),
           os.path.join("..", "..", "include", "lush_live_fwd.h"),
           os.path.join("..", "..", "include", "lush_subframe.h"),
           os.path.join("..", "..", "include", "lush_march.h")]      # (the last one is the contract _abi is read from)

_lib = None


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def needs_build() -> bool:
    if not os.path.exists(SO_PATH):
        return True
    t = os.path.getmtime(SO_PATH)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def use_library(path: str):
    """Developer tools only (tools/*.py: a build made by tools/build_variant.py, e.g. a parent commit's for a same-box A/B): load() will open `path` instead of the in-tree product."""
    global SO_PATH, _lib
    if _lib is not None:
        raise RuntimeError("lib.use_library: a library is already loaded")
    SO_PATH = os.path.abspath(path)


def build(force: bool = False, verbose: bool = False, extra_flags: Sequence[str] = (), out: str = None, audit: bool = True) -> str:
    """Compile the HIP sources for gfx950 into lush_nerf_amd/liblush_march.so and audit the result (isa_check).

    The product build takes nothing from the environment.  `extra_flags` / `out` are for developer builds (tools/build_variant.py:
    -DLUSH_CLOCK, a tuning default such as -DLUSH_DW_PE_COST=700) and refuse to write the product's path."""
    product = out is None
    if extra_flags and product:
        raise ValueError("lib.build: extra compiler flags need an explicit `out` path (the in-tree product is built without any)")
    target = SO_PATH if product else os.path.abspath(out)
    if product and not force and not needs_build():
        return SO_PATH
    # -ffp-contract=off: fp32 VALU expressions round op by op like the reference's torch ops
    # (o + d*z must not become one FMA: a 1-ulp point error is amplified x512 by the encoding).
    # one hipcc -c per source, in parallel (the chain kernels alone take ~1 min), then one link
    import re
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", *extra_flags]
    # per file: the 64-points-per-wave kernels keep their accumulators in VGPRs (the VALU converts them; AGPR-resident
    # accumulators cost one v_accvgpr_read per value) and let the B-operand buffers, which only MFMAs read, go to AGPRs
    per_file = {"lush_mlp_wide.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"], "lush_mlp_wide_bwd.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}
    usage = {}
    with tempfile.TemporaryDirectory(prefix="lush_build_") as tmp:
        def compile_one(f):
            obj = os.path.join(tmp, os.path.splitext(f)[0] + ".o")
            cmd = [_hipcc(), *flags, *per_file.get(f, []), "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, f), "-o", obj]
            if verbose:
                print(" ".join(cmd))
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
            # resource usage per kernel (informational; build_report() prints it).  Scalar spills are legal compiler behaviour;
            # what made round 3's spilled builds fault is checked on the emitted code below (isa_check rule R1).
            names = re.findall(r"Function Name: (\S+)", r.stderr)
            sg = [int(m) for m in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
            vg = [int(m) for m in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
            sc = [int(m) for m in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
            if f in per_file and not (names and len(names) == len(sg) == len(vg) == len(sc)):
                raise RuntimeError(f"{f}: no kernel-resource-usage remarks parsed (hipcc output format changed?)")
            for n, a_, b_, c_ in zip(names, sg, vg, sc):
                usage[n] = {"file": f, "sgpr_spills": a_, "vgpr_spills": b_, "scratch_bytes_per_lane": c_}
            return obj
        with ThreadPoolExecutor(max_workers=min(6, len(SOURCES))) as ex:
            objs = list(ex.map(compile_one, SOURCES))
        cmd = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", *objs, "-o", target + ".tmp"]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc link failed:\n" + r.stdout + r.stderr)
    if audit:
        # The hazards hipcc does not pad for `asm volatile` statements, checked on what was actually emitted (DESIGN.md
        # section 4, "Hazards"): a build in which register allocation or scheduling happened to create one never reaches a GPU.
        from . import isa_check
        n, found = isa_check.check_shared_object(target + ".tmp")
        if found:
            os.replace(target + ".tmp", target + ".rejected")
            raise RuntimeError(f"isa_check: {len(found)} hazard(s) in the built code objects ({n} kernels; the library was left at "
                               f"{target}.rejected, NOT installed):\n  " + "\n  ".join(found[:20]))
    os.replace(target + ".tmp", target)
    global LAST_BUILD_USAGE
    LAST_BUILD_USAGE = usage
    return target


LAST_BUILD_USAGE = {}


# The binding is READ from the header (abi.py): signatures, structs and constants are stated there, once.
_abi = abi.parse(open(os.path.join(CSRC, HEADERS[-1])).read())
_SIGS = _abi.protos                     # name -> (argtypes, restype), every prototype of the header
EXPORTS = list(_SIGS)
MlpParams, RbkParams = _abi.structs["lush_mlp_params"], _abi.structs["lush_rbk_params"]      # ... and lush_mlp_grads / lush_rbk_grads
MarchCfgC, PackJobC = _abi.structs["lush_march_cfg"], _abi.structs["lush_pack_job"]
MarchDraws, MarchOut, MarchGout = (_abi.structs["lush_march_" + n] for n in ("draws", "out", "gout"))
# every LUSH_X of the header as lib.X: ABI_VERSION, PLANES_F16 (plane code of ONE fp16 plane; 1..3 = bf16 planes), VARIANT_* (kernel-variant
# bits of the MLP entry points; 0 = the product's choice), VIEW_*, FAULT_*, RBK_*
globals().update({k[len("LUSH_"):]: v for k, v in _abi.consts.items()})
# bits of the numerical-fault word -> keys of the render result dict (final pass, coarse pass)
_FAULT_KEYS = {"RGB": ("rgb_map", "rgb0"), "DEPTH": ("depth_map", "depth0"), "ACC": ("acc_map", "acc0"),
               "DENSITY": ("density_map", "density0"), "RAW": ("raw", "raw0")}
FAULT_NAMES = {_abi.consts["LUSH_FAULT_" + c] << shift: keys[k]
               for k, shift in enumerate((0, _abi.consts["LUSH_FAULT_COARSE_SHIFT"])) for c, keys in _FAULT_KEYS.items()}
FAULT_NAMES[_abi.consts["LUSH_FAULT_ZSTD"]] = "z_std"
FAULT_BITS = {n: b for b, n in FAULT_NAMES.items()}
# The second contract header, include/lush_subframe.h (one entry point of the same library; lush_march.h and its tables above stay as they are)
_abi_subframe = abi.parse(open(os.path.join(CSRC, HEADERS[-2])).read(), "lush_subframe.h")
_SIGS_SUBFRAME = _abi_subframe.protos
EXPORTS_SUBFRAME = list(_SIGS_SUBFRAME)
# The third one, include/lush_live_fwd.h: the training march whose final pass computes colour on live points only -- its pieces,
# the predicate lush_march_trunk_form and the permission bit MARCH_FWD_LIST_KEPT of lush_march_bwd
_abi_live_fwd = abi.parse(open(os.path.join(CSRC, HEADERS[-3])).read(), "lush_live_fwd.h")
_SIGS_LIVE_FWD = _abi_live_fwd.protos
EXPORTS_LIVE_FWD = list(_SIGS_LIVE_FWD)
MARCH_FWD_LIST_KEPT = _abi_live_fwd.consts["LUSH_MARCH_FWD_LIST_KEPT"]
LIVE_LIST_COUNT_WORD = _abi_live_fwd.consts["LUSH_LIVE_LIST_COUNT_WORD"]
# The fourth, include/lush_live_coarse.h: the configuration bit that gives the coarse pass the same form (a stash and list regions of
# its own in the workspace), the word of its list's length and the predicate lush_march_coarse_trunk_form
_abi_live_coarse = abi.parse(open(os.path.join(CSRC, HEADERS[-4])).read(), "lush_live_coarse.h")
_SIGS_LIVE_COARSE = _abi_live_coarse.protos
EXPORTS_LIVE_COARSE = list(_SIGS_LIVE_COARSE)
MARCH_COARSE_TRUNK = _abi_live_coarse.consts["LUSH_MARCH_COARSE_TRUNK"]
LIVE_COARSE_LIST_COUNT_WORD = _abi_live_coarse.consts["LUSH_LIVE_COARSE_LIST_COUNT_WORD"]


def fault_names(word: int):
    return [n for b, n in FAULT_NAMES.items() if word & b]


def load():
    """Load the library (building is NOT implicit: call build() first)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64; it must be in the process before our library is
    # dlopen'ed, or the library binds a second HIP runtime that sees no device.
    import torch  # noqa: F401
    if not os.path.exists(SO_PATH):
        raise RuntimeError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is required; there is no fallback path)")
    lib = C.CDLL(SO_PATH)
    for name, (args, res) in (*_SIGS.items(), *_SIGS_SUBFRAME.items(), *_SIGS_LIVE_FWD.items(), *_SIGS_LIVE_COARSE.items()):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def call(name: str, *args):
    """Call an int-returning entry point; raise with lush_last_error() on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.lush_last_error().decode()}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def mlp_struct(tensors: Sequence, n_layers: int) -> MlpParams:
    """tensors = [w0,b0,...,w{n-1},b{n-1}, views_w, views_b, feat_w, feat_b, alpha_w, alpha_b, rgb_w, rgb_b]."""
    s = MlpParams()
    for l in range(n_layers):
        s.w[l] = tensors[2 * l].data_ptr()
        s.b[l] = tensors[2 * l + 1].data_ptr()
    o = 2 * n_layers
    s.w_views, s.b_views = tensors[o].data_ptr(), tensors[o + 1].data_ptr()
    s.w_feat, s.b_feat = tensors[o + 2].data_ptr(), tensors[o + 3].data_ptr()
    s.w_alpha, s.b_alpha = tensors[o + 4].data_ptr(), tensors[o + 5].data_ptr()
    s.w_rgb, s.b_rgb = tensors[o + 6].data_ptr(), tensors[o + 7].data_ptr()
    return s


def rbk_struct(tensors: Sequence) -> RbkParams:
    """tensors = [embed, (w,b)x4 trunk, r_branch w,b, v_branch w,b, w_branch w,b, r_linear w,b,
    v_linear w,b, w_linear w,b]."""
    s = RbkParams()
    s.embed = tensors[0].data_ptr()
    for l in range(4):
        s.w_trunk[l] = tensors[1 + 2 * l].data_ptr()
        s.b_trunk[l] = tensors[2 + 2 * l].data_ptr()
    names = ("w_rb", "b_rb", "w_vb", "b_vb", "w_wb", "b_wb", "w_r", "b_r", "w_v", "b_v", "w_w", "b_w")
    for k, n in enumerate(names):
        setattr(s, n, tensors[9 + k].data_ptr())
    return s
