"""Host: the output-stage exchange of conv3x3_w2d_kernel (flowmse_amd/csrc/conv_w2d.hip, w2d_out), restated in NumPy.

The products are transposed: source lane l holds unit l & 31 = (ur, uc) and register r holds channel
8 (r >> 2) + 4 (l >> 5) + (r & 3).  Per channel tile jd and register group q a source writes three float4 (partials c) to
destination wave (jd, ur), slot (h, c), position p = lambda ^ uc ^ 8 (ur & 1) with lambda = 8 uc + 2 q + kh; destination
lane lambda = (uc, cq) of wave (j, g) reads position lambda ^ uc ^ 8 (g & 1) of its twelve slots and stores its unit's
4 x 2 pixels as float4 over channels 4 cq .. 4 cq + 3.  Checked for every lane, register group, h, partial and NJ:
every (pixel, channel) of the tile is produced once, every slot position is written once per round, and the lane groups
of both LDS instructions touch distinct banks."""
import numpy as np
import pytest

XDEST = 4 * 3 * 256                      # floats per destination wave (W2_XDEST)
LANES = np.arange(64)

# lane groups that are served in one LDS cycle, and the bank modulus in dwords
READ_B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
READ_B128_GROUPS += [[l + 32 for l in g] for g in READ_B128_GROUPS]
CONTIG16 = [list(range(16 * k, 16 * k + 16)) for k in range(4)]
CONTIG8 = [list(range(8 * k, 8 * k + 8)) for k in range(8)]


def src_addr(lane, hq, jd, q, c):
    """float offset (inside the exchange region) of the float4 a source lane of wave h = hq writes"""
    li, kh = lane & 31, lane >> 5
    ur, uc = li >> 3, li & 7
    gpos = (uc * 8 + (kh ^ uc)) ^ ((ur & 1) << 3)
    return (jd * 4 + ur) * XDEST + (hq * 3 + c) * 256 + 4 * (gpos ^ (2 * q))


def dst_addr(lane, wave, s, c):
    """float offset of the float4 a destination lane of wave `wave` = (j, g) reads for h = s, partial c"""
    ucd, g = lane >> 3, wave & 3
    return wave * XDEST + (s * 3 + c) * 256 + 4 * ((lane ^ ucd) ^ ((g & 1) << 3))


def src_content(lane, jd, q):
    """(destination wave, unit column, channel quad) a source lane's register group q of channel tile jd holds"""
    li, kh = lane & 31, lane >> 5
    return jd * 4 + (li >> 3), li & 7, 2 * q + kh


def banks_distinct(addrs, groups, nbanks):
    """16-byte accesses at float offsets `addrs` (per lane): no two lanes of a group on one bank"""
    for g in groups:
        used = set()
        for l in g:
            b = {(int(addrs[l]) + d) % nbanks for d in range(4)}
            if used & b:
                return False
            used |= b
    return True


@pytest.mark.parametrize("NJ", [1, 2])
def test_exchange_map_is_a_bijection(NJ):
    """what a destination lane reads in slot (h, c) is what the source wave h wrote for that lane's (unit, channel quad)"""
    for hq in range(4):
        for c in range(3):
            written = {}
            for lane in LANES:
                for jd in range(NJ):
                    for q in range(4):
                        a = src_addr(lane, hq, jd, q, c)
                        assert a % 4 == 0 and 0 <= a < 8 * XDEST
                        assert a not in written, "slot position written twice in one round"
                        written[a] = src_content(lane, jd, q)
            assert len(written) == NJ * 4 * 64          # every position of slot (hq, c) of every destination, once
            for wave in range(4 * NJ):
                for lane in LANES:
                    a = dst_addr(lane, wave, hq, c)
                    assert written[a] == (wave, lane >> 3, lane & 7)


@pytest.mark.parametrize("NJ", [1, 2])
def test_every_pixel_and_channel_of_the_tile_once(NJ):
    """(lambda, row, x) -> pixel (4 g + row, 2 uc + x), channels 32 j + 4 cq .. + 3: the 16 x 16 x 32 NJ tile, once"""
    seen = np.zeros((16, 16, 32 * NJ), dtype=int)
    for wave in range(4 * NJ):
        j, g = wave >> 2, wave & 3
        for lane in LANES:
            ucd, cq = lane >> 3, lane & 7
            for i in range(8):
                row, x = i >> 1, i & 1
                seen[4 * g + row, 2 * ucd + x, 32 * j + 4 * cq: 32 * j + 4 * cq + 4] += 1
    assert (seen == 1).all()
    # one store instruction (fixed i) of a wave writes eight pixels x 128 bytes: whole lines
    for i in range(8):
        px = {(4 * 0 + (i >> 1), 2 * (l >> 3) + (i & 1)) for l in LANES}
        assert len(px) == 8
        for p in px:
            assert sorted(4 * (l & 7) for l in LANES if (4 * 0 + (i >> 1), 2 * (l >> 3) + (i & 1)) == p) == list(range(0, 32, 4))


def test_accumulator_layout_of_the_transposed_product():
    """register group q of lane half kh = channel quad 2 q + kh; the four registers of a group are consecutive channels"""
    for lane in LANES:
        for r in range(16):
            ch = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
            assert ch == 4 * (2 * (r >> 2) + (lane >> 5)) + (r & 3)


@pytest.mark.parametrize("NJ", [1, 2])
def test_lds_instructions_are_conflict_free(NJ):
    for hq in range(4):
        for c in range(3):
            for jd in range(NJ):
                for q in range(4):
                    a = np.array([src_addr(l, hq, jd, q, c) for l in LANES])
                    # ds_write_b128: eight groups of eight consecutive lanes over 32 banks ...
                    assert banks_distinct(a, CONTIG8, 32)
                    # ... and also when counted in four groups of sixteen consecutive lanes over 64 banks
                    assert banks_distinct(a, CONTIG16, 64)
            for wave in range(4 * NJ):
                a = np.array([dst_addr(l, wave, hq, c) for l in LANES])
                assert banks_distinct(a, READ_B128_GROUPS, 64)     # ds_read_b128's own four groups
                assert banks_distinct(a, CONTIG16, 64)


def test_the_unswizzled_layout_would_conflict():
    """the check has teeth: position = lambda, as a plain [lane 64][4] block, is an eight-way conflict for the writes"""
    a = np.array([(l & 7) * 8 * 4 for l in range(8)])           # eight unit columns, one channel quad
    assert not banks_distinct(np.concatenate([a, np.zeros(56, dtype=int)]), [list(range(8))], 32)
