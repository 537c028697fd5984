"""The one statistical check of include/chiara_mx4_sr.h's rule, on tests/mx4_sr_ref.py (no GPU: the kernels are held
to that reference bit for bit by tests/test_gpu_mx4_sr.py)."""
import numpy as np

import mx4_ref
import mx4_sr_ref as sr


def test_rounding_is_unbiased():
    """2^16 blocks of one 6.0, which fixes the scale at 127, and 31 values of 1.2: between 1.0 and 1.5, f = 0.4, so a
    dequantized value is 1 + 0.5 * Bernoulli(floor(0.4 * 2^16) / 2^16) and the mean of N = 31 * 2^16 of them has
    sigma = 0.5 * sqrt(f (1 - f) / N) = 1.7e-4; the floor's bias, 0.5 * 2^-16 at most, is 0.04 sigma.  Within 5 sigma
    of 1.2 -- deterministic under the fixed seed; round-to-nearest gives exactly 1.0, 1 100 sigma away."""
    src = np.full((1 << 16, 32), 1.2, dtype=np.float32)
    src[:, 0] = 6.0
    tiles = sr.quantize_ref(src.reshape(-1), 7)
    v = mx4_ref.dequantize_ref(tiles, src.size).view(np.float32).reshape(src.shape)[:, 1:].astype(np.float64)
    sigma = 0.5 * np.sqrt(0.4 * 0.6 / v.size)
    assert set(np.unique(v)) == {1.0, 1.5}
    assert abs(v.mean() - 1.2) < 5 * sigma, (v.mean(), sigma)
