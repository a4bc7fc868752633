"""CPU: the host side of the flow-matching objective -- keyed loss draws, the float64 definition, ``VFModel._loss`` and
the C-ABI surface (symbols, argument errors that are decided before any device call)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cases as Cs
import _fmloss_ref as R
from flowmse_amd.fmloss import fm_loss_reference
from flowmse_amd.util import noise as N

ERR_ARG = 1
KEYS = [0, 1, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000]


# ------------------------------------------------------------------------------------------------ loss_times / draw_key
def test_loss_times_range_dtype_and_known_answer():
    t = N.loss_times(KEYS, 7, 1.0, 0.03, draws=16)
    assert t.dtype == np.float32 and t.shape == (len(KEYS), 16)
    assert (t >= np.float32(0.03)).all() and (t <= np.float32(1.0)).all()
    assert len(np.unique(t)) > 70                                      # draws and keys give different times
    # known answer: the stated counter / key through the package's Philox (itself pinned to Random123's vectors)
    key, k, seed = KEYS[2], 5, 0xDEADBEEF12345678
    w0 = N.philox4x32_10((k, 0xFFFFFFFF, key & 0xFFFFFFFF, key >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
    u01 = np.float32((w0 >> 8) * 2.0 ** -24)
    want = np.minimum((np.float32(1.0) - u01) * np.float32(0.8 - 0.05) + np.float32(0.05), np.float32(0.8))
    got = N.loss_times([key], seed, 0.8, 0.05, draws=6)[0, 5]
    assert got.dtype == np.float32 and got == want


def test_loss_times_depend_on_key_seed_and_draw_only():
    a = N.loss_times(KEYS, 3, 1.0, 0.03, draws=4)
    b = N.loss_times(KEYS[::-1], 3, 1.0, 0.03, draws=4)
    assert np.array_equal(a, b[::-1])                                  # not on the order
    assert np.array_equal(N.loss_times([KEYS[2]], 3, 1.0, 0.03, draws=4)[0], a[2])          # not on the other keys
    assert np.array_equal(N.loss_times(KEYS, 3, 1.0, 0.03, draws=2), a[:, :2])              # not on the number of draws
    assert not np.array_equal(N.loss_times(KEYS, 4, 1.0, 0.03, draws=4), a)
    assert np.array_equal(N.loss_times(torch.tensor([-1], dtype=torch.int64).numpy().astype(np.uint64), 3, 1.0, 0.03, 4)[0], a[3])


def test_loss_times_refuse_t_eps_zero():
    for bad in (0.0, -0.01):
        with pytest.raises(ValueError, match="t_eps"):
            N.loss_times(KEYS, 0, 1.0, bad)


def test_draw_key():
    for k in KEYS:
        assert N.draw_key(k, 0) == k
        drawn = {N.draw_key(k, d) for d in range(1000)}
        assert len(drawn) == 1000 and all(0 <= v < 1 << 64 for v in drawn)
    assert N.draw_key(1, 1) == 1 ^ 0x9E3779B97F4A7C15
    assert N.loss_seed(7) == 7 ^ 0x6C6F7373 and N.loss_seed(N.loss_seed(7)) == 7


# ------------------------------------------------------------------------------------------------ fm_loss_reference
def test_reference_is_zero_when_the_field_is_the_target():
    x0, y, z, _ = R.inputs((3, 5, 6))
    ds = R.SIGMA_MAX - R.SIGMA_MIN
    u = ds * z.astype(np.complex128) + (y.astype(np.complex128) - x0)
    for kind in ("mse", "mae"):
        rows, mean = fm_loss_reference(u, x0, y, z, R.times(3), R.SIGMA_MIN, R.SIGMA_MAX, kind)
        assert rows.tolist() == [0.0, 0.0, 0.0] and mean == 0.0


def test_reference_hand_case_and_row_mean():
    # one row, two elements, sigma_max - sigma_min = 0.5: u = 0.5 z + (y - x0)
    x0 = np.array([[[[1 + 1j, 0j]]]])
    y = np.array([[[[2 + 1j, 1j]]]])
    z = np.array([[[[2j, 4 + 0j]]]])
    v = np.array([[[[4 + 5j, 2 - 2j]]]])
    # u = (1 + 1j, 2 + 1j); d = (3 + 4j, -3j); |d| = (5, 3)
    for kind, want in (("mse", 17.0), ("mae", 4.0)):
        rows, mean = fm_loss_reference(v, x0, y, z, [0.5], 0.25, 0.75, kind)
        assert rows.tolist() == [want] and mean == want
    # two rows: the mean is over rows, the sum over everything else
    two = [np.concatenate([a, 2 * a]) for a in (v, x0, y, z)]
    rows, mean = fm_loss_reference(*two, [0.5, 0.5], 0.25, 0.75, "mse")
    assert rows.tolist() == [17.0, 68.0] and mean == 42.5
    with pytest.raises(ValueError, match="loss_type"):
        fm_loss_reference(v, x0, y, z, [0.5], 0.25, 0.75, "huber")


# ------------------------------------------------------------------------------------------------ VFModel._loss
def test_model_loss_equals_the_reference_on_cpu_tensors():
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **Cs.TINY)
    x0, y, z, v = R.inputs((3, 5, 6), seed=1)
    zero = np.zeros_like(z)
    for kind in ("mse", "mae"):
        m.loss_type = kind
        got = m._loss(torch.from_numpy(v), torch.from_numpy(y))
        # with x0 = 0 and z = 0 the reference's target is y
        want = fm_loss_reference(v, zero, y, zero, R.times(3), R.SIGMA_MIN, R.SIGMA_MAX, kind)[1]
        assert got.dim() == 0 and abs(float(got) - want) <= 1e-5 * want          # fp32 tensor arithmetic against float64
    m.loss_type = "huber"
    with pytest.raises(ValueError, match="loss_type"):
        m._loss(torch.from_numpy(v), torch.from_numpy(y))
    with pytest.raises(ValueError, match="loss_type"):
        m._step((torch.from_numpy(x0), torch.from_numpy(y)), keys=[1, 2, 3])


def test_marginal_sample_on_cpu_tensors_is_the_tensor_formula():
    from flowmse_amd.odes import FLOWMATCHING
    ode = FLOWMATCHING(sigma_min=R.SIGMA_MIN, sigma_max=R.SIGMA_MAX)
    x0, y, z, _ = (torch.from_numpy(a) for a in R.inputs((3, 5, 6), seed=2))
    t = torch.from_numpy(R.times(3))
    x_t, z_out, u = ode.marginal_sample(x0, t, y, z, with_target=True)
    mean, std = ode.marginal_prob(x0, t, y)
    assert z_out is z and torch.equal(x_t, mean + std[:, None, None, None] * z)
    assert torch.equal(u, ode.der_std(t) * z + ode.der_mean(x0, t, y))
    xk, zk = ode.marginal_sample(x0, t, y, keys=[5, 6, 7], seed=9)
    want = torch.from_numpy(N.keyed_noise_reference([5, 6, 7], 9, 5, 6)).to(torch.complex64)
    assert torch.equal(zk, want) and torch.equal(xk, mean + std[:, None, None, None] * want)
    with pytest.raises(ValueError):
        ode.marginal_sample(x0, t, y, z, keys=[5, 6, 7])


# ------------------------------------------------------------------------------------------------ C-ABI surface
def test_surface_and_argument_errors_without_a_device():
    from flowmse_amd import _lib
    L = _lib.lib
    assert L.flowse_abi_version() == 3
    for name in ("flowse_fm_pair", "flowse_fm_loss_workspace_bytes", "flowse_fm_loss_rows", "flowse_fm_loss"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.flowse_fm_loss_workspace_bytes(8, 256, 256) >= 8 * 8
    assert L.flowse_fm_loss_workspace_bytes(1, 256, 256) * 8 >= L.flowse_fm_loss_workspace_bytes(8, 256, 256)
    for b, f, t in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, 3)):
        assert L.flowse_fm_loss_workspace_bytes(b, f, t) == -ERR_ARG
        assert b"flowse_fm_loss_workspace_bytes" in L.flowse_last_error()
    # host memory stands in for the tensors: every case below is refused before anything touches a device
    buf = (C.c_double * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 8)
    pair = [(None, p, p, p, None, p, 1, 4, 4), (p, p, p, p, p, p, 1, 4, 4), (p, p, p, None, None, p, 1, 4, 4),
            (p, p, p, p, None, p, 1, 4, 3), (p, p, p, p, None, p, 0, 4, 4), (odd, p, p, p, None, p, 1, 4, 4),
            (p, p, p, p, None, None, 1, 4, 4)]
    for x0, y, t, z, keys, xt, B, F, T in pair:
        assert L.flowse_fm_pair(x0, y, t, z, keys, 1, 0.0, 0.5, xt, None, B, F, T, None) == ERR_ARG
        assert b"flowse_fm_pair" in L.flowse_last_error()
    rows = [(p, p, 0, 4096, 1, 4, 4), (None, None, 0, 4096, 1, 4, 4), (p, None, 2, 4096, 1, 4, 4), (None, p, -1, 4096, 1, 4, 4),
            (p, None, 0, 4096, 1, 4, 5), (p, None, 0, 4096, 0, 4, 4), (odd, None, 0, 4096, 1, 4, 4)]
    for z, keys, kind, wsb, B, F, T in rows:
        assert L.flowse_fm_loss_rows(p, p, p, z, keys, 1, 0.0, 0.5, kind, p, p, wsb, B, F, T, None) == ERR_ARG
        assert b"flowse_fm_loss_rows" in L.flowse_last_error()
    assert L.flowse_fm_loss_rows(p, p, p, p, None, 1, 0.0, 0.5, 0, p, p, 7, 1, 4, 4, None) == ERR_ARG
    assert b"workspace" in L.flowse_last_error()
    assert L.flowse_fm_loss(None, p, p, p, p, None, 1, 0.0, 0.5, 0, p, 1, 4, 4, None) == ERR_ARG
    assert b"flowse_fm_loss:" in L.flowse_last_error()


def test_valid_loss_option_is_refused_with_torch_noise(capsys):
    from flowmse_amd.evaluate import parse_args
    assert parse_args(["--folder_destination", "o", "--synthetic", "1"]).valid_loss == 0
    assert parse_args(["--folder_destination", "o", "--synthetic", "1", "--noise", "keyed", "--valid_loss", "2"]).valid_loss == 2
    for extra in (["--valid_loss", "2"], ["--valid_loss", "2", "--noise", "torch"]):
        with pytest.raises(SystemExit):
            parse_args(["--folder_destination", "o", "--synthetic", "1"] + extra)
        assert "--valid_loss needs --noise keyed" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ validation item
@pytest.mark.parametrize("n_samples,left,start", [(16000, 8320, None), (16001, 8319, None), (48000, None, 7680),
                                                   (32640, None, 0)])
def test_validation_item_is_the_reference_crop_or_pad(n_samples, left, start):
    """flowmse/data_module.py:46-80 with shuffle_spec=False, normalize='noisy': centre crop from int((len - target) / 2), or
    zero pad pad // 2 left and pad // 2 + pad % 2 right, to (256 - 1) * 128 samples; both divided by the noisy crop's peak."""
    from flowmse_amd.model import VFModel
    from flowmse_amd.util.inference import validation_item
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **Cs.TINY)
    g = torch.Generator().manual_seed(n_samples)
    x, y = torch.randn(1, n_samples, generator=g), torch.randn(1, n_samples, generator=g)
    y[0, 3] = 9.0                                              # a peak outside the crop must not set the level
    target = 255 * 128
    if start is None:
        xs, ys = torch.zeros(1, target), torch.zeros(1, target)
        xs[:, left:left + n_samples], ys[:, left:left + n_samples] = x, y
    else:
        xs, ys = x[:, start:start + target], y[:, start:start + target]
    peak = ys.abs().max()
    X, Y = validation_item(m, x, y)
    assert X.shape == Y.shape == (1, 256, 256) and X.dtype == torch.complex64
    assert torch.equal(X, m._forward_transform(m._stft(xs / peak))) and torch.equal(Y, m._forward_transform(m._stft(ys / peak)))
    assert (peak == 9.0) == (start is None or start <= 3)
