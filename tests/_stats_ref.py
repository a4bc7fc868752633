"""float64 reference for the GroupNorm statistics the conv kernels fuse into their output stage.

A producer leaves one (mean, M2) partial per sample, pixel block and channel: partial [B, nblk, C, 2], block blk covering
n_blk = min(ppb, HW - blk * ppb) pixels with ppb = ceil(HW / nblk) (gn_pixels_per_block).  gn_finalize merges the partials
of a group's channels -- possibly from two sets with different nblk, for a concat input -- with Chan's formula.  Here the
same merge and the statistics of the stored tensor itself, both in float64 (numpy), and the two error measures the tests
bound.  Only GROUP statistics are specified: a kernel may spread a group's sums over the channels of the group as it likes
(conv3x3_pc16_kernel gives both channels of a pair the pair's joint mean and half its M2).
"""
import numpy as np


def groups(C):
    """the network's rule: nn.GroupNorm(min(C // 4, 32), C)"""
    return min(C // 4, 32)


def block_counts(HW, nblk):
    """pixels per block: nblk blocks of ceil(HW / nblk), the last one short"""
    ppb = -(-HW // nblk)
    n = np.array([min(ppb, HW - blk * ppb) for blk in range(nblk)], dtype=np.float64)
    assert (n > 0).all(), (HW, nblk)
    return n


def tensor_stats(o, G=None):
    """o: the stored tensor, NHWC ([B, H, W, C] or [B, HW, C]) -> mean, biased variance per (sample, group), [B, G] float64"""
    o = np.asarray(o, dtype=np.float64)
    B, C = o.shape[0], o.shape[-1]
    G = G or groups(C)
    x = o.reshape(B, -1, G, C // G)
    mu = x.mean(axis=(1, 3))
    var = ((x - mu[:, None, :, None]) ** 2).mean(axis=(1, 3))
    return mu, var


def partials_of(o, nblk):
    """the exact partials of a tensor: o NHWC -> [B, nblk, C, 2] float64 (mean, M2) per block and channel"""
    o = np.asarray(o, dtype=np.float64)
    B, C = o.shape[0], o.shape[-1]
    x = o.reshape(B, -1, C)
    HW = x.shape[1]
    ppb = -(-HW // nblk)
    p = np.empty((B, nblk, C, 2))
    for blk in range(nblk):
        seg = x[:, blk * ppb:min(HW, (blk + 1) * ppb)]
        p[:, blk, :, 0] = seg.mean(axis=1)
        p[:, blk, :, 1] = ((seg - p[:, blk, None, :, 0]) ** 2).sum(axis=1)
    return p


def merge_partials(sets, HW, G):
    """N-weighted Chan merge per group: sets = [partial [B, nblk_s, C_s, 2], ...] covering consecutive channel ranges (a
    group may straddle two sets) -> mean, biased variance [B, G] float64.
        mu = sum n_i m_i / N,   var = sum (M2_i + n_i (m_i - mu)^2) / N,   N = HW * C / G"""
    sets = [np.asarray(p, dtype=np.float64) for p in sets]
    B, C = sets[0].shape[0], sum(p.shape[2] for p in sets)
    cpg = C // G
    N = float(HW) * cpg
    counts = [block_counts(HW, p.shape[1])[None, :, None] for p in sets]
    s1 = np.concatenate([(n * p[..., 0]).sum(axis=1) for n, p in zip(counts, sets)], axis=1)          # [B, C]
    mu = s1.reshape(B, G, cpg).sum(axis=2) / N
    mu_c = np.repeat(mu, cpg, axis=1)                                                                 # [B, C]
    c0, q = 0, []
    for n, p in zip(counts, sets):
        m = mu_c[:, None, c0:c0 + p.shape[2]]
        q.append((p[..., 1] + n * (p[..., 0] - m) ** 2).sum(axis=1))
        c0 += p.shape[2]
    var = np.concatenate(q, axis=1).reshape(B, G, cpg).sum(axis=2) / N
    return mu, var


MEAN_ULPS = 2.0 ** -22       # the partial means are fp32 numbers: four roundings of a value of size |mu| are always allowed


def errors(mu, var, mu_ref, var_ref):
    """Worst over samples and groups of
        e_mean = |mu - mu_ref| / sigma_ref,   e_var = |var / var_ref - 1|,
        c_mean = e_mean - 2^-22 |mu_ref| / sigma_ref   (what e_mean needs beyond the fp32 representation of the mean:
                 the c_m of the bound  e_mean <= 2^-22 |mu_ref| / sigma_ref + c_m; may be negative)"""
    sd = np.sqrt(var_ref)
    e_mean = np.abs(mu - mu_ref) / sd
    return (float(e_mean.max()), float(np.abs(var / var_ref - 1.0).max()),
            float((e_mean - MEAN_ULPS * np.abs(mu_ref) / sd).max()))
