"""The cases of tests/test_ray_kernels_gpu.py without a GPU (tests/ray_cases.py builds them for both files): the fp32 oracle against
the float64 oracle on every case -- the yardsticks -- must sit at or below 1/8 of the project's gate of its quantity, so the GPU
file's gates max(project gate, 8 x yardstick) ARE the project's figures and the cases are well conditioned; the index and
straddle conditions of the warp cases; and the loss-scale rule's expected-value table in numpy."""
import numpy as np
import pytest
import torch

from tests import ray_cases as RC

F32, F64 = torch.float32, torch.float64


def _check(tag, errs, quantity_of):
    bad = []
    for k, e in errs.items():
        q = quantity_of(k)
        print(f"RAYK yardstick {tag} {k}: {e:.3e} (gate {RC.GATES[q]:.0e} / 8)")
        if not e <= RC.GATES[q] / 8:
            bad.append((k, e, RC.GATES[q] / 8))
    assert not bad, bad


@pytest.mark.parametrize("run", RC.WARP_RUNS, ids=RC.warp_id)
def test_warp_yardsticks(run):
    _check("warp " + RC.warp_id(run), RC.warp_errors(RC.warp_oracle(run, F32), RC.warp_oracle(run, F64), run[1]), RC.warp_quantity)


def test_warp_cases_straddle_what_they_claim():
    assert RC.warp_rpb(4, 51) == 51 and RC.warp_rpb(4, 52) == 51          # one workgroup / a second one with a single ray
    assert -(-255 // RC.warp_rpb(4, 255)) == 5 and -(-300 // RC.warp_rpb(2, 300)) == 4 and 257 % RC.warp_rpb(1, 257) == 1
    seen = {}
    for run in RC.WARP_RUNS:
        n_img, M, N, ndc, variant = run
        x = RC.warp_inputs(run)
        assert x["rays"].shape == (N, 3, 2) and x["idx"].shape == (N,) and 0 <= x["idx"].min() and x["idx"].max() < n_img
        assert x["params"]["mlp_rbk.r_linear.weight"].shape == (3 * M, 32) and x["params"]["mlp_rbk.w_linear.weight"].shape == (M + 1, 32)
        seen[n_img] = max(seen.get(n_img, 0), int(x["idx"].max()))
        if variant == "partial_mask":
            assert 0 < int(x["mask"].sum()) < N
        if variant == "zero_mask":
            assert int(x["mask"].sum()) == 0
    assert seen[65] >= RC.WN_IMGS and seen[80] >= RC.WN_IMGS and seen[64] < RC.WN_IMGS      # the global-atomics fallback is exercised past the table
    # the all-zero mask: no gradient reaches the rays or the r / v heads, the weight head keeps its own
    ref = RC.warp_oracle((30, 4, 255, True, "zero_mask"), F64)
    assert not bool(ref["d_rays"].any()) and all(not bool(ref["params"][i].any()) for i in RC.RV_HEADS)
    assert all(bool(ref["params"][i].any()) for i in RC.W_HEAD)


@pytest.mark.parametrize("run", RC.COMP_RUNS, ids=RC.comp_id)
def test_compositing_backward_yardsticks(run):
    R = run[0]
    _check("composite " + RC.comp_id(run), RC.comp_errors(RC.comp_oracle(run, F32), RC.comp_oracle(run, F64)), lambda k: "comp_bwd")
    blocks = min(-(-R // 4), 2048)
    walked = np.concatenate([RC.comp_block_rays(R, blocks, b) for b in range(blocks)])
    assert np.array_equal(np.sort(walked), np.arange(R))
    if R == 8262:
        assert blocks == 2048 and len(RC.comp_block_rays(R, blocks, 0)) == 8 and len(RC.comp_block_rays(R, blocks, 2047)) == 4


@pytest.mark.parametrize("N,M1,gamma", RC.TAIL_RUNS)
def test_image_tail_yardsticks(N, M1, gamma):
    _check(f"tail N={N} M1={M1} gamma={int(gamma)}", RC.tail_errors(RC.tail_oracle(N, M1, gamma, F32), RC.tail_oracle(N, M1, gamma, F64), M1),
           lambda k: RC.tail_columns(k, M1)[0])
    ref = RC.tail_oracle(N, M1, gamma, F64)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())


@pytest.mark.parametrize("N,same,scale", RC.LOSS_RUNS)
def test_train_loss_yardsticks(N, same, scale):
    a, b, tg, hits = RC.loss_inputs(N)
    assert hits == int((a == tg).sum()) and (hits >= 1 if N >= 85 else True) and hits <= max(1, 0.03 * a.size)
    o32, o64 = RC.loss_oracle(N, same, scale, F32), RC.loss_oracle(N, same, scale, F64)
    errs = {"loss": RC.colerr(o32["loss"], o64["loss"]), "ga": RC.colerr(o32["ga"], o64["ga"], 3)}
    if not same:
        errs["gb"] = RC.colerr(o32["gb"], o64["gb"], 3)
    _check(f"loss N={N} same={int(same)} scale={scale}", errs, lambda k: "tail_fwd" if k == "loss" else "tail_bwd")
    if hits:      # the sign term is 0 where a equals the target: the gradient there is the (zero) squared term's alone
        assert float(o64["ga"][torch.from_numpy(a == tg)].abs().max()) == 0.0


@pytest.mark.parametrize("V,ns", RC.CONSIST_RUNS)
def test_consistency_loss_yardsticks(V, ns):
    rgb, cert = RC.consist_inputs(V, ns)
    above = (cert >= np.float32(RC.CONSIST_THR)).sum(0)
    assert above[RC.CONSIST_NONE] == 0 and above[RC.CONSIST_ONE] == 1 and above.max() >= min(V, 2) and 0 < above.sum() < V * ns
    o32, o64 = RC.consist_oracle(V, ns, F32), RC.consist_oracle(V, ns, F64)
    _check(f"consist V={V} ns={ns}", {"loss": RC.colerr(o32["loss"], o64["loss"]), "grad": RC.colerr(o32["grad"], o64["grad"], 3)},
           lambda k: "tail_fwd" if k == "loss" else "tail_bwd")
    assert not bool(o64["grad"][:, RC.CONSIST_NONE].any()) and not bool(o64["grad"][:, RC.CONSIST_ONE].any())


def test_loss_scale_table():
    """The rule in numpy: below a maximum of 2^-124 the unclamped 2^(4 - e) is not a float (+Inf, reciprocal 0), and already at
    2^-124 its reciprocal is subnormal; the clamp at 2^126 leaves every maximum of 2^-122 and above as it was."""
    f = np.float32
    table = {tag: RC.scale_exponent(mx) for tag, mx in RC.SCALE_MAXIMA}
    assert table == {"1.0": 3, "8.0": 0, "15.999": 0, "16.0": -1, "3e-5": 19, "1e30": -96, "2.9e38": -124, "2^-123": 126, "1.5e-38": 129,
                     "1e-42": 143, "zero": None, "inf": None, "nan": None}
    for tag, mx in RC.SCALE_MAXIMA:
        k, want = table[tag], RC.scale_expected(mx)
        if k is None:
            assert want == (f(1), f(1))
            continue
        with np.errstate(over="ignore", divide="ignore"):
            unclamped = np.ldexp(f(1), k)
            inv_unclamped = f(1) / unclamped
        if k <= RC.SCALE_K_MAX:
            assert want == (unclamped, inv_unclamped) and 8 <= float(f(mx)) * float(want[0]) < 16
            assert float(want[0]) * float(want[1]) == 1.0 and want[1] >= np.finfo(f).tiny
        else:
            assert want is None and np.isinf(unclamped) and inv_unclamped == 0      # the defect: d_raw x Inf x 0
            clamped = (np.ldexp(f(1), RC.SCALE_K_MAX), np.ldexp(f(1), -RC.SCALE_K_MAX))
            assert RC.scale_small_ok(mx, *clamped)
            assert not RC.scale_small_ok(mx, unclamped, inv_unclamped)
    # the boundary: 2^-122 is the smallest maximum the clamp leaves alone; k = 127 (2^-124) is finite but its reciprocal subnormal
    assert RC.scale_exponent(2.0 ** -122) == 125 and RC.scale_exponent(np.nextafter(f(2.0 ** -122), f(0))) == 126
    assert RC.scale_exponent(2.0 ** -124) == 127 and not RC.scale_small_ok(2.0 ** -124, np.ldexp(f(1), 127), np.ldexp(f(1), -127))
    cases = RC.scale_cases()
    assert len(cases) == (1 + 2 + 2 + 2 + 3) * len(RC.SCALE_MAXIMA)      # first, last, index 256 (the last of n = 257)
    for tag, n, a, mx in cases:
        assert a.shape == (n,) and a.dtype == np.float32
        if np.isfinite(mx):
            assert float(np.max(a)) == float(mx)
