"""CPU tests of isa_check rule R6: the VGPR that the chunk queue's claim owns in dw_group_kernel<.., 1> (v255) is named only by the
returning atomic and by the LDS store behind a counted wait."""
import re

from lush_nerf_amd import isa_check as C, lib


def _text(body: str) -> str:
    lines = [l.strip() for l in body.strip().split("\n") if l.strip()]
    out = ["0000000000001000 <k>:"]
    for n, l in enumerate(lines):
        out.append(f"\t{l}    // {0x1000 + 4 * n:012X}: 00000000")
    return "\n".join(out)


def _check(body: str, name="_ZN4lush15dw_group_kernelILb1ELb1ELi1ELi1EEEvNS_7DwGroupE"):
    return [f for f in C.check_kernel(name, C.parse_kernels(_text(body))["k"]) if f.startswith("R6")]


GOOD = """
    s_nop 4
    global_atomic_add v255, v2, v3, s[18:19] sc0
    v_add_u32_e32 v4, v5, v6
    s_waitcnt vmcnt(8)
    ds_write_b32 v3, v255
    s_endpgm
"""


def test_the_claim_statements_pass():
    assert _check(GOOD) == []


def test_a_copy_of_the_pending_register_is_refused():
    assert len(_check(GOOD.replace("v_add_u32_e32 v4, v5, v6", "v_mov_b32_e32 v4, v255"))) == 1
    assert len(_check(GOOD.replace("v_add_u32_e32 v4, v5, v6", "v_mfma_f32_32x32x16_bf16 v[0:15], v[200:203], v[252:255], v[0:15]"))) == 1
    assert len(_check(GOOD.replace("v_add_u32_e32 v4, v5, v6", "v_add_u32_e32 v255, v5, v6"))) == 1


def test_the_store_needs_its_counted_wait():
    assert len(_check(GOOD.replace("s_waitcnt vmcnt(8)", "s_waitcnt lgkmcnt(0)"))) == 1
    assert len(_check(GOOD.replace("s_waitcnt vmcnt(8)", "s_waitcnt vmcnt(12)"))) == 1


def test_other_kernels_keep_their_v255():
    assert _check(GOOD.replace("v_add_u32_e32 v4, v5, v6", "v_mov_b32_e32 v4, v255"), name="_ZN4lush15dw_group_kernelILb1ELb1ELi1EEEvNS_7DwGroupE") == []


def test_the_kernel_is_compiled_without_v255():
    src = open(lib.CSRC + "/lush_mlp.hip").read()
    assert re.search(r"amdgpu_num_vgpr\(255\)\)\) void dw_group_kernel", src)
    assert list(C.R6_KERNELS.values()) == [255]
