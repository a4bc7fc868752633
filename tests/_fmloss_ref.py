"""Float64 restatement of one flow-matching training pair for the tests, with the magnitudes its error bounds are taken
over, and the deterministic inputs the fmloss tests share.

Restated from the reference (nothing is imported from it):
    sigma(t) = (1 - t) sigma_min + t sigma_max                flowmse/odes.py:86-88
    x_t      = (1 - t) x0 + t y + sigma(t) z                  flowmse/odes.py:83-84, flowmse/model.py:134-137
    u        = (sigma_max - sigma_min) z + (y - x0)           flowmse/odes.py:102-107, flowmse/model.py:138-140
sigma_min / sigma_max are the float32 values the C ABI receives, t the float32 times.
"""
import numpy as np

SIGMA_MIN = float(np.float32(0.05))          # non-zero, so that every term of sigma(t) is exercised
SIGMA_MAX = float(np.float32(0.487))
T_EPS, T_REV = 0.03, 1.0


def times(B):
    """Per-row t cycling through t_eps, 0.5 and T_rev = 1 (float32)."""
    return np.asarray([(T_EPS, 0.5, T_REV)[b % 3] for b in range(B)], dtype=np.float32)


def inputs(shape, seed=0):
    """x0, y, z, v: complex64 [B,1,F,T] standard-normal-like arrays, fixed by (shape, seed)."""
    g = np.random.default_rng(1000 + seed)
    B, F, T = shape

    def c():
        return (g.standard_normal((B, 1, F, T)) + 1j * g.standard_normal((B, 1, F, T))).astype(np.complex64)
    return c(), c(), c(), c()


def pair_float64(x0, y, z, t, sigma_min, sigma_max):
    """(x_t, mag_xt, u, mag_u) in float64: the exact values for the given float32 inputs and, per real part, the sums of
    absolute terms |(1-t) x0| + |t y| + |sigma z| and |ds z| + |y - x0| the rounding bounds scale with.  Real and imaginary
    parts are independent, so every array is returned as float64 [..., 2]."""
    def parts(a):
        a = np.asarray(a)
        return np.stack([a.real, a.imag], axis=-1).astype(np.float64)
    x0, y, z = parts(x0), parts(y), parts(z)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1, 1, 1, 1)
    sig = (1.0 - t) * sigma_min + t * sigma_max
    ds = sigma_max - sigma_min
    xt = (1.0 - t) * x0 + t * y + sig * z
    mag_xt = np.abs((1.0 - t) * x0) + np.abs(t * y) + np.abs(sig * z)
    u = ds * z + (y - x0)
    mag_u = np.abs(ds * z) + np.abs(y - x0)
    return xt, mag_xt, u, mag_u


def parts32(t):
    """complex64 torch tensor -> float64 numpy [..., 2] (re, im) without changing a bit of the float32 values."""
    a = t.detach().cpu().numpy()
    return np.stack([a.real, a.imag], axis=-1).astype(np.float64)
