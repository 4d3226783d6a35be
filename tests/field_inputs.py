"""Inputs of the free-point / free-z fixture (tests/golden/field_query.npz), regenerated from (seed, shape) by both the
generator (tests/golden/make_golden_field.py) and the tests: pure lush_nerf_amd.synth, no reference, no GPU."""
import numpy as np

from lush_nerf_amd import synth

SEED = 61
R, S, S_NOISE = 16, 12, 20
NUM_IMG = 30
WEIGHT_SETS = {"default": dict(), "trained": dict(trained_like=(6000, 40))}
# raw2outputs cases: (name, training, raw_noise_std, white_bkgd); eval has the near mask 80/128 = 0.625 inside the z range
R2O_CASES = (("train", True, 1.0, False), ("train_white", True, 1.0, True), ("eval", False, 0.0, False))
RMNEAR = 80


def _st(name):
    return synth._stream("field." + name)


def weights(which):
    return synth.all_weights(NUM_IMG, SEED, **WEIGHT_SETS[which])


def points():
    """[R,S,3] uniform in [-1.2,1.2]^3: not collinear, some outside the NDC cube."""
    return synth.uniform((R, S, 3), -1.2, 1.2, SEED, _st("pts"))


def points_noise():
    return synth.uniform((R, S_NOISE, 3), -1.2, 1.2, SEED, _st("pts_noise"))


def dirs():
    """[R,3] with norms 0.5 .. 2 on purpose: an implementation that normalises them fails."""
    d = synth.normal((R, 3), SEED, _st("dirs")).astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (d * synth.uniform((R, 1), 0.5, 2.0, SEED, _st("dirnorm")).astype(np.float64)).astype(np.float32)


def g_raw():
    return synth.normal((R, S, 4), SEED, _st("g_raw"))


def g_noise():
    return synth.normal((R, 3), SEED, _st("g_noise"))


def r2o_inputs():
    """raw [R,S,4] (sigma raw x 30), z_vals [R,S] increasing in 0.3 .. 1 (straddling 0.625), the served noise [R,S-1]."""
    raw = synth.normal((R, S, 4), SEED, _st("r2o.raw"))
    raw[..., 3] *= 30.0
    z = np.sort(synth.uniform((R, S), 0.3, 1.0, SEED, _st("r2o.z")), axis=-1)
    noise = synth.normal((R, S - 1), SEED, _st("r2o.noise"))
    return raw, z, noise


def r2o_upstream():
    """Upstream gradients of (rgb_map, density, acc_map, weights, depth_map)."""
    shapes = dict(rgb_map=(R, 3), density=(R, S - 1), acc_map=(R,), weights=(R, S), depth_map=(R,))
    return {k: synth.normal(sh, SEED, _st("r2o.g." + k)) for k, sh in shapes.items()}
