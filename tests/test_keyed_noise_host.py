"""CPU: the keyed noise stream's host restatement, the utterance keys, the world-size-independent plan, the evaluate
command line and the C-ABI surface of the keyed calls (no GPU compute calls)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY_A, KEY_B = 0x0123456789ABCDEF, 0xFEDCBA9876543210
# 5 standard errors at n = 65536: sqrt(0.5 / n) = 2.76e-3 for the mean of a part (variance 1/2), the same for the variance
# estimate of a part (var of x^2 = 2 sigma^4 = 1/2) and less for the cross moments
BOUND = 1.4e-2


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    from flowmse_amd.util.noise import philox4x32_10
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    f = 0xFFFFFFFF
    assert philox4x32_10((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # the array form computes the same words
    w = philox4x32_10((np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]),
                       np.array([0, 0x03707344])), (np.array([0, 0xA4093822]), np.array([0, 0x299F31D0])))
    assert [int(v[0]) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v[1]) for v in w] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_reference_moments_and_independence():
    from flowmse_amd.util.noise import keyed_noise_reference
    z = keyed_noise_reference([KEY_A], 7, 256, 256)
    assert z.shape == (1, 1, 256, 256) and z.dtype == np.complex128 and np.isfinite(z.view(np.float64)).all()
    re, im = z.real.ravel(), z.imag.ravel()
    figures = {"mean re": re.mean(), "mean im": im.mean(), "var re - 1/2": re.var() - 0.5, "var im - 1/2": im.var() - 0.5,
               "E[re im]": (re * im).mean()}
    print(figures)
    for name, v in figures.items():
        assert abs(v) < BOUND, (name, v)
    other_key = keyed_noise_reference([KEY_B], 7, 256, 256).ravel()
    other_seed = keyed_noise_reference([KEY_A], 8, 256, 256).ravel()
    for name, o in (("key", other_key), ("seed", other_seed)):
        c = [np.corrcoef(a, b)[0, 1] for a in (re, im) for b in (o.real, o.imag)]
        print(name, c)
        assert max(abs(v) for v in c) < BOUND, (name, c)
        assert not np.array_equal(o, z.ravel())


def test_reference_addressing():
    from flowmse_amd.util.noise import keyed_noise_reference
    keys = [KEY_A, KEY_B, 3, 2 ** 64 - 1]
    z128 = keyed_noise_reference(keys, 11, 8, 128)
    z64 = keyed_noise_reference(keys, 11, 8, 64)
    assert np.array_equal(z128[..., :64], z64)                                    # the padded length does not matter
    assert np.array_equal(keyed_noise_reference(keys, 11, 4, 64), z64[:, :, :4])  # nor the number of bins
    for b, k in enumerate(keys):                                                  # nor the batch or the row
        assert np.array_equal(keyed_noise_reference([k], 11, 8, 64)[0], z64[b])
    perm = [2, 0, 3, 1]
    assert np.array_equal(keyed_noise_reference([keys[i] for i in perm], 11, 8, 64), z64[perm])
    assert not np.array_equal(z64[0], z64[1])


def test_utterance_key():
    import bench
    from flowmse_amd.util.noise import utterance_key
    assert utterance_key("p232_001.wav") == 0x912975D344AF26C6
    assert utterance_key("/data/test/noisy/p232_001.wav") == utterance_key("p232_001.wav") == \
        utterance_key(os.path.join("elsewhere", "p232_001.wav"))
    names = [f"vbdmd_{i:04d}.wav" for i in range(bench.VBDMD_UTTS)]
    assert len(names) == 824 and len({utterance_key(n) for n in names}) == 824
    assert all(0 <= utterance_key(n) < 2 ** 64 for n in names)


def _batches(plan):
    return sorted((T, tuple(ids)) for rank in plan for T, ids in rank)


def test_plan_shards_unlevelled_is_plan_batches_at_every_world():
    import bench
    from flowmse_amd.parallel import plan_batches, plan_shards
    config3 = [((t + 63) // 64) * 64 for t in bench.vbdmd_lengths(bench.VBDMD_UTTS)]
    g = np.random.default_rng(0)
    ragged = (64 * g.integers(2, 11, 200)).tolist()                               # padded lengths 128..640
    for lens in (config3, ragged):
        want = sorted((T, tuple(ids)) for T, ids in plan_batches(range(len(lens)), lens, 8))
        for world in (1, 2, 3, 8):
            plan = plan_shards(lens, world, 8, level=False)
            assert len(plan) == world and _batches(plan) == want, world
    # why the flag exists: the default's levelling step splits batches at world 8 (30 batches become 33)
    want = sorted((T, tuple(ids)) for T, ids in plan_batches(range(200), ragged, 8))
    levelled = _batches(plan_shards(ragged, 8, 8))
    assert levelled != want and len(levelled) > len(want)
    assert plan_shards(ragged, 8, 8) == plan_shards(ragged, 8, 8, level=True)


def test_gather_rows_without_process_group():
    from flowmse_amd.parallel import gather_rows
    rows = [(1, "a", 0.5), (0, "b", 2.0)]
    assert gather_rows(rows) == rows and gather_rows(iter(rows)) == rows
    assert gather_rows([]) == []


def test_evaluate_command_line(capsys):
    from flowmse_amd.evaluate import _synthetic_pairs, build_parser, parse_args
    base = ["--folder_destination", "o"]
    a = parse_args(base)
    assert (a.gpus, a.noise, a.seed, a.batch, a.streams, a.synthetic_seconds, a.N, a.precision) == \
        (1, "torch", None, 1, 1, [2.0], 5, "fp32")
    assert parse_args(base + ["--gpus", "2"]).noise == "keyed"
    assert parse_args(base + ["--gpus", "2", "--noise", "keyed"]).noise == "keyed"
    assert parse_args(base + ["--noise", "keyed"]).gpus == 1
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--gpus", "2", "--noise", "torch"])
    assert e.value.code == 2 and "keyed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(base + ["--gpus", "0"])
    assert parse_args(base + ["--synthetic_seconds", "1.0,2.0,3.0"]).synthetic_seconds == [1.0, 2.0, 3.0]
    assert "byte" in build_parser().format_help()                                 # --batch promises tolerance, not bytes
    # the default durations give the pairs evaluate always made; a list is cycled
    old, new = _synthetic_pairs(3), _synthetic_pairs(3, seconds=parse_args(base).synthetic_seconds)
    for (n0, c0, y0), (n1, c1, y1) in zip(old, new):
        assert n0 == n1 and c0.shape == (32000,) and np.array_equal(c0, c1) and np.array_equal(y0, y1)
    cyc = _synthetic_pairs(5, seconds=[1.0, 2.0, 3.0])
    assert [p[2].shape[0] for p in cyc] == [16000, 32000, 48000, 16000, 32000]
    assert [p[0] for p in cyc] == [f"synthetic_{i:02d}.wav" for i in range(5)]


def test_cabi_declares_and_exports_keyed_calls():
    from flowmse_amd import _lib
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("flowse_prior_sample_keyed", "flowse_op_keyed_noise"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.flowse_abi_version() == 3
    assert re.search(r"#define\s+FLOWSE_ABI_VERSION\s+3\b", header)


def test_prior_sampling_keys_on_cpu_tensors():
    from flowmse_amd.odes import FLOWMATCHING
    from flowmse_amd.util.noise import keyed_noise_reference
    ode = FLOWMATCHING()
    g = torch.Generator().manual_seed(0)
    y = torch.view_as_complex(torch.randn(3, 1, 16, 64, 2, generator=g))
    keys = [KEY_A, KEY_B, 5]
    x, z = ode.prior_sampling(y.shape, y, keys=keys, seed=9)
    ref = torch.from_numpy(keyed_noise_reference(keys, 9, 16, 64)).to(torch.complex64)
    assert torch.equal(z, ref) and z.dtype == torch.complex64
    assert torch.equal(x, y + ref * ode.prior_std())
    # the 64 key bits may also come as an int64 tensor
    kt = torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in keys], dtype=torch.int64)
    assert torch.equal(ode.prior_sampling(y.shape, y, keys=kt, seed=9)[0], x)
    with pytest.raises(ValueError):
        ode.prior_sampling(y.shape, y, ref, keys=keys)
    with pytest.raises(ValueError):
        ode.prior_sampling(y.shape, y, keys=keys[:2])
    # without keys nothing changes: z as given, or the process-wide generator
    assert torch.equal(ode.prior_sampling(y.shape, y, ref)[0], y + ref * ode.prior_std())
    torch.manual_seed(3)
    a = ode.prior_sampling(y.shape, y)[1]
    torch.manual_seed(3)
    assert torch.equal(a, torch.randn_like(y))
