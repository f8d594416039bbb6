"""The array form of the search model (tests/ref_models_me.py) against the per-sample statement of
tests/test_gpu_me_golden.py, on the CPU: the GPU tests of the scalarised search rest on the former."""
import numpy as np
import pytest

import ref_models_me as mm
from test_gpu_me_golden import _me_ref


def _pictures(seed, wmb, hmb):
    rng = np.random.default_rng(seed)
    W, H = wmb * 16, hmb * 16
    base = rng.integers(0, 256, size=(H + 40, W + 40)).astype(np.float64)
    k = np.ones(5) / 5
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, base)
    ref = np.ascontiguousarray(np.clip(base[10:10 + H, 12:12 + W], 0, 255).astype(np.uint8))
    src = np.ascontiguousarray(np.clip(base[13:13 + H, 10:10 + W] + rng.normal(0, 2, size=(H, W)), 0, 255).astype(np.uint8))
    return rng, src, ref


@pytest.mark.parametrize("R,seed", [(4, 3), (2, 4)])
def test_array_model_equals_per_sample_model(host, R, seed):
    wmb, hmb = 3, 2
    rng, src, ref = _pictures(seed, wmb, hmb)
    pred = rng.integers(-24, 24, size=(wmb * hmb, 2)).astype(np.int16)
    lam = host.table("lambda")[0]
    rmv, rcost, rpred, rintra = _me_ref(src, ref, pred, 27, R, lam, wmb, hmb)
    m = mm.me_search(src, ref, pred, 27, R, lam, wmb, hmb)
    assert np.array_equal(m["mv"], rmv) and np.array_equal(m["cost"], rcost)
    assert np.array_equal(m["pred"], rpred) and np.array_equal(m["intra"], rintra)


def test_se_bits_is_exp_golomb():
    for v in range(-600, 600):
        u = -2 * v if v <= 0 else 2 * v - 1
        assert mm.se_bits(v) == 2 * int(np.floor(np.log2(u + 1))) + 1
