"""CPU: the float64 merge of GroupNorm partials (tests/_stats_ref.py) against numpy on the tensor itself.

The GPU tests of the fused statistics (tests/test_gpu_fused_stats.py) compare a kernel's partials, merged by
merge_partials, with tensor_stats of what the kernel stored.  Here the merge is fed exact float64 partials of a random
tensor, for every block geometry the producers use, and must reproduce the tensor's own statistics to 1e-12.
"""
import numpy as np
import pytest

import _stats_ref as S

TOL = 1e-12


def tensor(seed, B, HW, C, offset=0.0):
    rng = np.random.default_rng(seed)
    # per-channel means and spreads differ inside a group
    return rng.standard_normal((B, HW, C)) * (0.5 + rng.random(C)) + rng.standard_normal(C) + offset


def check(mu, var, o, G):
    mu_ref, var_ref = S.tensor_stats(o, G)
    e_mean, e_var, _ = S.errors(mu, var, mu_ref, var_ref)
    assert e_mean <= TOL and e_var <= TOL, (e_mean, e_var)


@pytest.mark.parametrize("HW,nblk", [(256, 1), (256, 8), (1024, 128), (64, 64),        # equal blocks (down to one pixel)
                                     (257, 2), (100, 3), (1000, 7), (4, 1)])           # a short last block
@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_merge_one_set(HW, nblk, offset):
    o = tensor(1, 2, HW, 48, offset)
    n = S.block_counts(HW, nblk)
    assert n.sum() == HW and (n[:-1] == n[0]).all() and n[-1] <= n[0]
    mu, var = S.merge_partials([S.partials_of(o, nblk)], HW, 12)
    check(mu, var, o, 12)


@pytest.mark.parametrize("HW,nblk1,nblk2", [(256, 16, 1), (1024, 16, 4), (257, 2, 5)])
def test_merge_two_sets_straddling_group(HW, nblk1, nblk2):
    """C = 256 + 128 over 32 groups of 12 channels: group 21 (channels 252 .. 263) takes four channels from set 1 and eight
    from set 2, whose blocks have another size"""
    o = tensor(2, 2, HW, 384, 3.0)
    sets = [S.partials_of(o[..., :256], nblk1), S.partials_of(o[..., 256:], nblk2)]
    mu, var = S.merge_partials(sets, HW, S.groups(384))
    assert S.groups(384) == 32 and 21 * 12 < 256 < 22 * 12
    check(mu, var, o, 32)


def test_merge_sees_a_wrong_count():
    """the merge weights every block by its own pixel count: one pixel more per block moves the result"""
    o = tensor(3, 1, 257, 16, 5.0)
    p = S.partials_of(o, 2)
    mu_ref, var_ref = S.tensor_stats(o, 4)
    mu, var = S.merge_partials([p], 257, 4)
    assert S.errors(mu, var, mu_ref, var_ref)[0] <= TOL
    p_wrong = S.partials_of(np.concatenate([o, o[:, :1]], axis=1), 2)       # blocks of 129 + 129 pixels
    mu, var = S.merge_partials([p_wrong], 257, 4)
    assert S.errors(mu, var, mu_ref, var_ref)[0] > 1e-6


def test_errors_allowance():
    """c_mean is what e_mean needs beyond 2^-22 |mu| / sigma, group by group"""
    mu_ref, var_ref = np.array([[1024.0, 0.0]]), np.array([[1.0, 4.0]])
    e_mean, e_var, c_mean = S.errors(mu_ref + np.array([[2.0 ** -12, 2e-6]]), var_ref * (1 + 1e-6), mu_ref, var_ref)
    assert abs(e_mean - 2.0 ** -12) < 1e-15 and abs(e_var - 1e-6) < 1e-12
    assert abs(c_mean - 1e-6) < 1e-15          # group 0: 2^-12 - 1024 * 2^-22 = 0; group 1: 2e-6 / 2 - 0
