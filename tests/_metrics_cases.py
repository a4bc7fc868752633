"""The signals of the metrics tests (test_gpu_metrics.py, test_metrics_host.py): one generator, ten cases."""
import numpy as np

SR = 16000


def sig(L, seed, gaps=()):
    """(clean x, noisy y) float32 of L samples at 16 kHz: six warbling partials under a 4 Hz envelope, the samples
    [a L, b L) of every gap (a, b, g) scaled by g, plus white noise of standard deviation 0.1 drawn from ``seed``."""
    n = np.arange(L) / SR
    s = sum(np.sin(2 * np.pi * f * n * (1 + 0.05 * np.sin(2 * np.pi * 3 * n))) / (i + 1)
            for i, f in enumerate((180, 360, 540, 1250, 2400, 3100)))
    s = s * (0.55 + 0.45 * np.sin(2 * np.pi * 4 * n)) ** 2
    for a, b, g in gaps:
        s[int(a * L):int(b * L)] *= g
    x = (0.3 * s).astype(np.float32)
    y = (x + 0.1 * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)
    return x, y


# case -> (L, seed, gaps)
CASES = {
    1: (16000, 7, ()),                                             # plain 1 s signal
    2: (20000, 7, ((0.4, 0.6, 1e-4),)),                            # gap in the middle
    3: (20003, 7, ((0, 0.15, 1e-4), (0.9, 1, 1e-4))),              # gaps at both ends, L not a multiple of 8
    4: (4800, 7, ()),                                              # too short: 1e-5
    5: (6554, 1, ()),                                              # exactly 30 spectrum frames, one segment
    6: (8601, 7, ()),                                              # L10 = 5376: the exclusive range drops the last full frame
    7: (24000, 7, ((0.25, 1, 1e-4),)),                             # mostly silent: 1e-5 by way of the kept count
    8: (336000, 7, ((0.1, 0.2, 1e-4), (0.35, 0.45, 1e-4), (0.6, 0.7, 1e-4), (0.85, 0.95, 1e-4))),   # > 1024 first-pass frames
    9: (8000, 7, ()),                                              # all-zero clean signal: every norm zero, d = 0
    10: (16000, 7, ()),                                            # x_hat = x: d = 1
}
# case -> (first-pass frames, kept, spectrum frames) where the case was built for them
EXPECT = {1: (77, 74, 73), 2: (96, 75, 74), 3: (96, 70, 69), 4: (22, 22, 21), 5: (31, 31, 30), 6: (40, 40, 39),
          7: (116, 30, 29)}


def signals(case):
    """(clean, processed) of a case."""
    L, seed, gaps = CASES[case]
    x, y = sig(L, seed, gaps)
    if case == 9:
        return np.zeros(L, dtype=np.float32), y
    if case == 10:
        return x, x.copy()
    return x, y
