"""GPU: the flow-matching objective (csrc/fmloss.hip) -- the pair kernel per element against float64, the loss kernels
against ``fm_loss_reference``, keyed against explicit noise bit for bit, row independence, ``flowse_fm_loss`` on the tiny
model against its three parts and against the CPU oracle's field, the facade, the argument checks and
``evaluate --valid_loss`` (child processes, one after the other, each under its own time limit).  No test asserts a time.

Rounding bounds of the pair kernel, counted from its operations (u = 2^-24; every fp32 operation rounds once, nothing is
fused; t, sigma_min, sigma_max >= 0, so sigma(t) is a sum of non-negative terms):
    a = fl(1 - t)                                            1 rounding
    sig = fl(fl(a sigma_min) + fl(t sigma_max))              a: 1, product: 1, sum: 1        -> 3 on sig
    x_t = fl(fl(fl(a x0) + fl(t y)) + fl(sig z))
      (1 - t) x0 : a 1, product 1, inner sum 1, outer sum 1                                  -> 4
      t y        : product 1, inner sum 1, outer sum 1                                       -> 3
      sigma z    : sig 3, product 1, outer sum 1                                             -> 5
    so |x_t - exact| <= gamma_5 (|(1-t) x0| + |t y| + |sigma z|), gamma_5 = 5u / (1 - 5u) < 6u:     K_XT = 6  (<= 8)
    u = fl(fl(ds z) + fl(y - x0)), ds = fl(sigma_max - sigma_min)
      ds z   : ds 1, product 1, sum 1                                                        -> 3
      y - x0 : difference 1, sum 1                                                           -> 2
    so |u - exact| <= gamma_3 (|ds z| + |y - x0|) < 4u (...):                                        K_U = 4   (<= 8)
The float64 reference's own rounding (2^-53 relative) is eight orders below either bound.
"""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _cases as C
import _fmloss_ref as R
from flowmse_amd import _lib
from flowmse_amd.fmloss import fm_loss_reference
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
U32 = 2.0 ** -24
K_XT, K_U = 6, 4
assert K_XT <= 8 and K_U <= 8
KEYS = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 3, 2 ** 64 - 1, 0x8000000000000000, 0x912975D344AF26C6, 1 << 32, 77]
SEED = 0x1F2E3D4C5B6A7988
SHAPES = [(1, 1, 2), (3, 5, 6), (2, 64, 64), (8, 256, 256)]
ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
TIGHT = 1e-4                     # the rel-L2 bound of test_gpu_model.py::test_tiny_forward_golden
MODE_CEILING = {"bf16": 1.7e-2, "fp16": 2.1e-3}      # test_gpu_model.py::test_precision_modes_vs_oracle


def _dev_keys(keys):
    return torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in keys], dtype=torch.int64, device="cuda")


def _noise(keys, seed, F, T):
    z = torch.empty(len(keys), 1, F, T, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_op_keyed_noise(_lib.ptr(_dev_keys(keys)), seed, _lib.ptr(z), len(keys), F, T, _lib.current_stream()))
    return z


def _pair(x0, y, t, z=None, keys=None, seed=SEED, smin=R.SIGMA_MIN, smax=R.SIGMA_MAX, target=True):
    B, _, F, T = x0.shape
    xt = torch.empty_like(x0)
    u = torch.empty_like(x0) if target else None
    kd = None if keys is None else _dev_keys(keys)
    _lib.check(L.flowse_fm_pair(_lib.ptr(x0), _lib.ptr(y), _lib.ptr(t), _lib.ptr(z), _lib.ptr(kd), seed, smin, smax,
                                _lib.ptr(xt), _lib.ptr(u), B, F, T, _lib.current_stream()))
    return xt, u


def _rows(v, x0, y, z=None, keys=None, seed=SEED, kind=0, smin=R.SIGMA_MIN, smax=R.SIGMA_MAX):
    B, _, F, T = x0.shape
    nbytes = L.flowse_fm_loss_workspace_bytes(B, F, T)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(B + 1, dtype=torch.float64, device="cuda")
    kd = None if keys is None else _dev_keys(keys)
    _lib.check(L.flowse_fm_loss_rows(_lib.ptr(v), _lib.ptr(x0), _lib.ptr(y), _lib.ptr(z), _lib.ptr(kd), seed, smin, smax, kind,
                                     _lib.ptr(out), _lib.ptr(ws), nbytes, B, F, T, _lib.current_stream()))
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The inputs of one shape on the host and on the device, made once and never written to."""
    host = R.inputs(shape)
    t = R.times(shape[0])
    dev = tuple(torch.from_numpy(a).cuda() for a in host)
    return host, t, dev, torch.from_numpy(t).cuda()


def _model(cfg):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    return _model(C.TINY)


# ---------------------------------------------------------------------------------------------------- pair, explicit z
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_pair_explicit_noise_per_element_against_float64(shape):
    """Measured on an MI355X, worst |kernel - float64| in units of u x magnitude, x_t / u: (1,1,2) 1.43 / 0.39, (3,5,6)
    1.88 / 1.44, (2,64,64) 2.73 / 1.98, (8,256,256) 3.11 / 2.29; asserted at the counted K_XT = 6 / K_U = 4 (header)."""
    (x0, y, z, _), t, (x0d, yd, zd, _), td = _case(shape)
    xt, u = _pair(x0d, yd, td, zd)
    torch.cuda.synchronize()
    ref_xt, mag_xt, ref_u, mag_u = R.pair_float64(x0, y, z, t, R.SIGMA_MIN, R.SIGMA_MAX)
    exc_xt = np.abs(R.parts32(xt) - ref_xt) / (U32 * mag_xt)
    exc_u = np.abs(R.parts32(u) - ref_u) / (U32 * mag_u)
    print(f"fm_pair {shape}: worst |x_t - ref| = {exc_xt.max():.3f} u * magnitude (bound {K_XT}), "
          f"worst |u - ref| = {exc_u.max():.3f} u * magnitude (bound {K_U})")
    assert np.isfinite(R.parts32(xt)).all() and exc_xt.max() <= K_XT
    assert exc_u.max() <= K_U
    # without the target the same x_t
    assert torch.equal(_pair(x0d, yd, td, zd, target=False)[0], xt)


def test_pair_at_t1_sigma_min0_is_the_prior_sample_bit_for_bit():
    """sigma_min = 0, t = 1: a = 0, so a x0 = +-0, t y = y, their sum y; sig = fl(0 + sigma_max) = sigma_max; x_t = y +
    fl(sigma_max z) -- the operation order of flowse_prior_sample (y + fl(z sigma); the product commutes), so the bits
    agree.  (A part of y that is -0 next to a +0 product of a x0 would give +0; the inputs hold no zero.)"""
    (_, y, _, _), _, (x0d, yd, zd, _), _ = _case((3, 5, 6))
    assert (y.real != 0).all() and (y.imag != 0).all()
    ones = torch.ones(3, device="cuda")
    xt, _ = _pair(x0d, yd, ones, zd, smin=0.0, smax=R.SIGMA_MAX, target=False)
    want = torch.empty_like(yd)
    _lib.check(L.flowse_prior_sample(_lib.ptr(yd), _lib.ptr(zd), R.SIGMA_MAX, _lib.ptr(want), yd.numel(), _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(xt, want) and not torch.equal(xt, yd)


# ---------------------------------------------------------------------------------------------------- pair, keyed
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_pair_keyed_equals_explicit_path_fed_the_generated_noise(shape):
    B, F, T = shape
    _, _, (x0d, yd, _, _), td = _case(shape)
    zk = _noise(KEYS[:B], SEED, F, T)
    want_xt, want_u = _pair(x0d, yd, td, zk)
    got_xt, got_u = _pair(x0d, yd, td, keys=KEYS[:B])
    torch.cuda.synchronize()
    assert torch.equal(got_xt, want_xt) and torch.equal(got_u, want_u)
    assert not torch.equal(_pair(x0d, yd, td, keys=KEYS[:B], seed=SEED + 1)[0], want_xt)


# ---------------------------------------------------------------------------------------------------- loss rows
@pytest.mark.parametrize("kind", ["mse", "mae"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_loss_rows_against_the_float64_definition(shape, kind):
    """Measured on an MI355X, worst relative error of a row in units of 2^-53, mse / mae: (1,1,2) 0 / 0, (3,5,6) 2.40 / 1.72,
    (2,64,64) 1.25 / 0, (8,256,256) 5.01 / 3.58; asserted at (F T + 8) 2^-53, the float64 sum of F T non-negative terms in
    any order."""
    B, F, T = shape
    (x0, y, z, v), t, (x0d, yd, zd, vd), _ = _case(shape)
    code = {"mse": 0, "mae": 1}[kind]
    out = _rows(vd, x0d, yd, zd, kind=code).cpu().numpy()
    want_rows, want_mean = fm_loss_reference(v, x0, y, z, t, R.SIGMA_MIN, R.SIGMA_MAX, kind)
    n = F * T
    rel = np.abs(out[:B] - want_rows) / want_rows
    print(f"fm_loss_rows {shape} {kind}: worst relative error {rel.max() / 2.0 ** -53:.2f} x 2^-53 (bound {n + 8})")
    assert np.isfinite(out).all() and (rel <= (n + 8) * 2.0 ** -53).all()
    s = 0.0
    for r in out[:B].tolist():                                      # out[B]: the rows summed in row order, divided by B
        s += r
    assert out[B] == s / B and abs(out[B] - want_mean) <= (n + 8) * 2.0 ** -53 * want_mean
    # keyed: the target is regenerated from the key, bit-identical to the explicit path fed the generated noise
    zk = _noise(KEYS[:B], SEED, F, T)
    assert torch.equal(_rows(vd, x0d, yd, keys=KEYS[:B], kind=code), _rows(vd, x0d, yd, zk, kind=code))


@pytest.mark.parametrize("shape", [(3, 5, 6), (2, 64, 64)], **ids)
def test_a_row_does_not_depend_on_its_batch_or_position(shape):
    B, F, T = shape
    _, _, (x0d, yd, zd, vd), _ = _case(shape)
    for kind in (0, 1):
        whole = _rows(vd, x0d, yd, zd, kind=kind)
        assert torch.equal(_rows(vd, x0d, yd, zd, kind=kind), whole)                          # a second identical call
        keyed = _rows(vd, x0d, yd, keys=KEYS[:B], kind=kind)
        for b in range(B):
            alone = _rows(*(a[b:b + 1].contiguous() for a in (vd, x0d, yd, zd)), kind=kind)
            assert alone[0] == whole[b] and alone[1] == whole[b]
            assert _rows(*(a[b:b + 1].contiguous() for a in (vd, x0d, yd)), keys=KEYS[b:b + 1], kind=kind)[0] == keyed[b]
        perm = list(range(1, B)) + [0]                                                        # every row at another position
        moved = _rows(*(a[perm].contiguous() for a in (vd, x0d, yd, zd)), kind=kind)
        assert torch.equal(moved[:B], whole[perm])


# ---------------------------------------------------------------------------------------------------- the whole call
def _tiny_case(times):
    x0, y, z = (a.cuda() for a in C.tiny_inputs())
    return x0, y, z, torch.tensor(times, dtype=torch.float32, device="cuda")


def _fm_loss(model, x0, y, t, z=None, keys=None, seed=SEED, kind=0):
    sm, sx = float(model.ode.sigma_min), float(model.ode.sigma_max)
    kd = None if keys is None else _dev_keys(keys)
    return model.dnn.fm_loss(x0, y, t, z, kd, seed, sm, sx, kind), sm, sx


@functools.lru_cache(maxsize=None)
def _oracle_field(times):
    """The CPU oracle's field at the x_t the pair kernel makes for the tiny inputs, with u and d = v_oracle - u in float64
    (computed once per time setting)."""
    from oracle import ncsnpp_oracle as O
    tb = C.param_tables()["tiny"]
    w = C.synth_weights(tb["names"], tb["shapes"])
    x0, y, z, t = _tiny_case(times)
    xt, _ = _pair(x0, y, t, z, smin=0.0, smax=float(np.float32(0.487)), target=False)
    v = O.vf_forward(w, O.make_cfg(**C.TINY), xt.cpu(), t.cpu(), y.cpu()).numpy().astype(np.complex128)
    ds = float(np.float32(0.487)) - 0.0
    u = ds * z.cpu().numpy().astype(np.complex128) + (y.cpu().numpy().astype(np.complex128) - x0.cpu().numpy())
    return v, v - u


def _oracle_gap_ok(out, times, eps, what):
    v, d = _oracle_field(times)
    B = v.shape[0]
    rows_o = 0.5 * (np.abs(d) ** 2).reshape(B, -1).sum(1)
    nd, nv = np.linalg.norm(d), np.linalg.norm(v)
    bound = 0.5 * (2 * nd * eps * nv + (eps * nv) ** 2)
    got = out.cpu().numpy()
    gap = abs(got[:B].sum() - rows_o.sum())
    print(f"flowse_fm_loss tiny t={times} {what}: rows {got[:B]}, oracle rows {rows_o}, |sum L - sum L_oracle| = {gap:.4e} "
          f"(bound {bound:.4e} at eps = {eps})")
    return np.isfinite(got).all() and gap <= bound


@pytest.mark.parametrize("times", [(0.03, 1.0), (0.5, 0.5)], **ids)
def test_fm_loss_equals_its_three_parts_and_the_oracle(tiny, times):
    """The rel-L2 bound eps of the tiny forward test is a bound over the whole [2,1,64,64] tensor, so the inequality
    |L - L_oracle| <= 0.5 (2 |d| eps |v_oracle| + (eps |v_oracle|)^2) is applied to the sum of the rows with whole-tensor
    norms (d = v_oracle - u)."""
    x0, y, z, t = _tiny_case(times)
    for kind in (0, 1):
        out, sm, sx = _fm_loss(tiny, x0, y, t, z, kind=kind)
        xt, _ = _pair(x0, y, t, z, smin=sm, smax=sx, target=False)
        v = tiny(xt, t, y)
        assert torch.equal(out, _rows(v, x0, y, z, kind=kind, smin=sm, smax=sx))
    keyed, _, _ = _fm_loss(tiny, x0, y, t, keys=KEYS[:2])
    assert torch.equal(keyed, _fm_loss(tiny, x0, y, t, _noise(KEYS[:2], SEED, 64, 64))[0])
    out, _, _ = _fm_loss(tiny, x0, y, t, z)
    assert _oracle_gap_ok(out, times, TIGHT, "fp32")


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_fm_loss_in_the_16_bit_modes(tiny, mode):
    """Finite, and within the mode's forward ceiling put through the inequality above.  The tiny network has no channel
    count the 16-bit kernels take, so on an MI355X these runs return the fp32 bits (measured gap 3.6e-3 in every mode):
    the test shows that the call works with the mode set, not what the mode costs."""
    times = (0.03, 1.0)
    x0, y, z, t = _tiny_case(times)
    tiny.dnn.set_precision(mode)
    try:
        out, _, _ = _fm_loss(tiny, x0, y, t, z)
        torch.cuda.synchronize()
    finally:
        tiny.dnn.set_precision("fp32")
    assert _oracle_gap_ok(out, times, MODE_CEILING[mode], mode)


def test_step_and_loss_rows_return_what_the_c_call_returns(tiny):
    x0, y, z, t = _tiny_case((0.03, 1.0))
    out, sm, sx = _fm_loss(tiny, x0, y, t, z)
    loss = tiny._step((x0, y), 0, t=t, z=z)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.is_cuda and loss == out[2]
    assert torch.equal(tiny.loss_rows(x0, y, t, z), out[:2])
    tiny.loss_type = "mae"
    try:
        assert tiny._step((x0, y), t=t, z=z) == _fm_loss(tiny, x0, y, t, z, kind=1)[0][2]
    finally:
        tiny.loss_type = "mse"
    # keyed: t from loss_times, z from the row keys, both under seed ^ 0x6C6F7373
    from flowmse_amd.util.noise import loss_seed, loss_times
    a = tiny._step((x0, y), keys=KEYS[:2], seed=11)
    tk = torch.from_numpy(loss_times(KEYS[:2], loss_seed(11), tiny.T_rev, tiny.t_eps)[:, 0].copy()).cuda()
    assert a == _fm_loss(tiny, x0, y, tk, keys=KEYS[:2], seed=loss_seed(11))[0][2]
    assert a == tiny._step((x0, y), keys=KEYS[:2], seed=11) and a != tiny._step((x0, y), keys=KEYS[:2], seed=12)
    # unkeyed: the reference's draws from torch's generator
    torch.manual_seed(3)
    b = tiny._step((x0, y))
    torch.manual_seed(3)
    assert torch.isfinite(b) and b == tiny._step((x0, y))
    # the path's own entry: one flowse_fm_pair launch
    xt, zz, u = tiny.ode.marginal_sample(x0, t, y, z, with_target=True)
    want_xt, want_u = _pair(x0, y, t, z, smin=sm, smax=sx)
    assert zz is z and torch.equal(xt, want_xt) and torch.equal(u, want_u)
    xk, none = tiny.ode.marginal_sample(x0, t, y, keys=KEYS[:2], seed=SEED)
    assert none is None and torch.equal(xk, _pair(x0, y, t, keys=KEYS[:2], smin=sm, smax=sx, target=False)[0])


# ---------------------------------------------------------------------------------------------------- validation set
def test_validation_loss_over_a_valid_set(tmp_path):
    """``validation_loss`` on the full network (the validation item has 256 bins) equals the keyed draws made by hand:
    same rows, same calls, so the same float64 values."""
    from test_host_logic import _valid_set
    from flowmse_amd.util.inference import validation_item, validation_loss
    from flowmse_amd.util.noise import draw_key, loss_seed, loss_times, utterance_key
    from flowmse_amd.util.other import read_wav
    full = _model(C.FULL)
    full.data_module.valid_set = vs = _valid_set(tmp_path, 3, seconds=[1.0, 3.0])          # a padded and a cropped item
    got = validation_loss(full, batch=1, seed=7, draws=2)
    rows = []
    for i in range(3):
        X, Y = validation_item(full, read_wav(vs.clean_files[i])[0].cuda(), read_wav(vs.noisy_files[i])[0].cuda())
        key = utterance_key(vs.noisy_files[i])
        ts = loss_times([key], loss_seed(7), full.T_rev, full.t_eps, draws=2)[0]
        for k in range(2):
            t = torch.tensor([float(ts[k])], dtype=torch.float32)
            rows.append(float(full.loss_rows(X[None], Y[None], t, keys=[draw_key(key, k)], seed=7)[0]))
    print("validation_loss over 3 files x 2 draws:", got, "rows", rows)
    assert np.isfinite(got) and got > 0 and abs(got - np.mean(rows)) <= 1e-12 * got
    first_last = validation_loss(full, num_files=2, batch=1, seed=7, draws=2)              # files 0 and 2, as evaluate_model picks
    assert abs(first_last - np.mean(rows[:2] + rows[4:])) <= 1e-12 * first_last
    assert validation_loss(full, batch=1, seed=8, draws=2) != got


# ---------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_return_a_status_and_leave_the_output_untouched(tiny):
    B, F, T = 2, 8, 16
    x = torch.zeros(B, 1, F, T, dtype=torch.complex64, device="cuda")
    t = torch.ones(B, device="cuda")
    kd = _dev_keys(KEYS[:B])
    out = torch.full((B + 1,), 7.0, dtype=torch.float64, device="cuda")
    xt = torch.full_like(x, 7.0)
    nbytes = L.flowse_fm_loss_workspace_bytes(B, F, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p, s = _lib.ptr, _lib.current_stream()
    # (z, keys, T, loss_type, workspace bytes)
    bad = [(p(x), p(kd), T, 0, nbytes), (None, None, T, 0, nbytes), (p(x), None, T - 1, 0, nbytes), (p(x), None, T, 2, nbytes),
           (p(x), None, T, 0, nbytes - 1)]
    for z, keys, tt, kind, wsb in bad:
        assert L.flowse_fm_loss_rows(p(x), p(x), p(x), z, keys, 1, 0.0, 0.5, kind, p(out), p(ws), wsb, B, F, tt, s) == ERR_ARG
        assert b"flowse_fm_loss_rows" in L.flowse_last_error()
    for z, keys, tt, kind, _ in bad[:4]:
        assert L.flowse_fm_loss(tiny.dnn._handle, p(x), p(x), p(t), z, keys, 1, 0.0, 0.5, kind, p(out), B, F, tt, s) == ERR_ARG
        assert b"flowse_fm_loss:" in L.flowse_last_error()
    for z, keys, tt, _, _ in bad[:3]:
        assert L.flowse_fm_pair(p(x), p(x), p(t), z, keys, 1, 0.0, 0.5, p(xt), None, B, F, tt, s) == ERR_ARG
        assert b"flowse_fm_pair" in L.flowse_last_error()
    with pytest.raises(_lib.FlowseError):
        _lib.check(L.flowse_fm_pair(p(x), p(x), p(t), None, None, 1, 0.0, 0.5, p(xt), None, B, F, T, s))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((xt == 7.0).all())                   # nothing was written
    with pytest.raises(ValueError):
        tiny.ode.marginal_sample(x[:, :, :, :15], t, x[:, :, :, :15])


# ---------------------------------------------------------------------------------------------------- CLI
def _evaluate(out, extra, limit=300):
    """One CLI child under its own time limit; returns (completed process, wall seconds)."""
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "flowmse_amd.evaluate",
                        "--folder_destination", str(out), "--synthetic_seconds", "0.5", "--N", "1", "--noise", "keyed",
                        "--seed", "7"] + extra, cwd=ROOT, capture_output=True, text=True)
    return r, time.time() - t0


def _column(path, name):
    lines = path.read_text().splitlines()
    header = lines[0].split(",")
    return header, {row.split(",")[0]: row.split(",")[header.index(name)] for row in lines[1:]} if name in header else None


@pytest.mark.timeout(1200)
def test_evaluate_valid_loss_column(tmp_path):
    """Children run one after the other; a failed one ends the test.  A file's valid_loss depends on (weights, file name,
    seed, draws) only: the 3-file set and the 5-file set print the same strings for the files they share."""
    arms = {"set3": ["--synthetic", "3", "--valid_loss", "2"], "set5": ["--synthetic", "5", "--valid_loss", "2"],
            "plain": ["--synthetic", "1"]}
    for tag, extra in arms.items():
        r, dt = _evaluate(tmp_path / tag, extra)
        print(f"arm ({tag}) {' '.join(extra)}: {dt:.1f} s wall (process start to exit)")
        assert r.returncode == 0, f"arm ({tag}) exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    header, vl3 = _column(tmp_path / "set3" / "_results.csv", "valid_loss")
    assert header == ["filename", "pesq", "estoi", "si_sdr", "si_sir", "si_sar", "valid_loss"]
    _, vl5 = _column(tmp_path / "set5" / "_results.csv", "valid_loss")
    assert len(vl3) == 3 and len(vl5) == 5 and all(vl5[n] == v for n, v in vl3.items())
    assert all(np.isfinite(float(v)) and float(v) > 0 for v in vl5.values()) and len(set(vl5.values())) == 5
    assert "valid_loss: " in (tmp_path / "set3" / "_avg_results.txt").read_text()
    assert "valid_loss draws: 2\n" in (tmp_path / "set3" / "_settings.txt").read_text()
    header, none = _column(tmp_path / "plain" / "_results.csv", "valid_loss")
    assert header == ["filename", "pesq", "estoi", "si_sdr", "si_sir", "si_sar"] and none is None
    assert "valid_loss" not in (tmp_path / "plain" / "_avg_results.txt").read_text()
    assert "valid_loss" not in (tmp_path / "plain" / "_settings.txt").read_text()
