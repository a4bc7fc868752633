"""GPU: the keyed prior noise (csrc/noise.hip) -- the kernel against its float64 restatement, the addressing invariances
on the device, the solvers' ``noise_keys=`` path, the C calls' argument checks, and ``evaluate --noise keyed`` across
``--gpus`` / ``--streams`` (child processes, one after the other, each under its own time limit).  No test asserts a time.
"""
import filecmp
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _cases as C
from flowmse_amd import _lib
from flowmse_amd.util import synth
from flowmse_amd.util.noise import keyed_noise_reference

pytestmark = pytest.mark.gpu
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
KEYS = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 3, 2 ** 64 - 1, 0x8000000000000000, 0x912975D344AF26C6, 1 << 32, 77]
SEED = 0x1F2E3D4C5B6A7988

# Largest |kernel - float64 restatement| over both parts, measured on an MI355X (gfx950) at seed SEED:
#   [1,256,64]: 3.553e-07    [3,64,128]: 3.506e-07    [8,256,256]: 3.755e-07        (max |z| there: 2.95 / 3.20 / 3.65)
# One fp32 ulp of values in [2, 4) is 2.4e-7, so this is one to two ulp of the largest values: the rounding of logf /
# sqrtf / cospif / sinpif and of the final product.  The bound is 4 x the largest figure (1.5e-6), the margin for other
# ROCm versions' math functions; a wrong word, pairing or address gives differences of order 1.
MEASURED_MAX = 3.755e-07
NOISE_BOUND = 4 * MEASURED_MAX
assert NOISE_BOUND < 1e-5


def _dev_keys(keys):
    return torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in keys], dtype=torch.int64, device="cuda")


def _noise(keys, seed, F, T):
    z = torch.empty(len(keys), 1, F, T, dtype=torch.complex64, device="cuda")
    _lib.check(L.flowse_op_keyed_noise(_lib.ptr(_dev_keys(keys)), seed, _lib.ptr(z), len(keys), F, T, _lib.current_stream()))
    return z


def _model(cfg):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    m.dnn.load_state_dict({n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    return _model(C.TINY)


# ---------------------------------------------------------------------------------------------------- 10
@pytest.mark.parametrize("shape", [(1, 256, 64), (3, 64, 128), (8, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_float64_restatement(shape):
    """Measured max |difference| per shape on an MI355X: [1,256,64] 3.553e-07, [3,64,128] 3.506e-07, [8,256,256]
    3.755e-07; asserted at 4 x the largest (MEASURED_MAX above)."""
    B, F, T = shape
    z = _noise(KEYS[:B], SEED, F, T)
    torch.cuda.synchronize()
    got = z.cpu().numpy()
    assert np.isfinite(got.view(np.float32)).all()
    ref = keyed_noise_reference(KEYS[:B], SEED, F, T)
    d = got.astype(np.complex128) - ref
    worst = max(np.abs(d.real).max(), np.abs(d.imag).max())
    print(f"keyed noise [{B},{F},{T}]: max |kernel - float64| = {worst:.3e}, max |z| = {np.abs(ref).max():.3f}, "
          f"E|z|^2 = {(np.abs(got) ** 2).mean():.4f}")
    assert worst <= NOISE_BOUND, worst


# ---------------------------------------------------------------------------------------------------- 11
def test_prior_sample_keyed_equals_prior_sample_of_the_noise():
    B, F, T = 3, 64, 128
    y = C.c64(synth.synth_spectrogram(5, B, F, T)).cuda()
    z = _noise(KEYS[:B], SEED, F, T)
    sigma = 0.487
    want, got = torch.empty_like(y), torch.empty_like(y)
    _lib.check(L.flowse_prior_sample(_lib.ptr(y), _lib.ptr(z), sigma, _lib.ptr(want), y.numel(), _lib.current_stream()))
    _lib.check(L.flowse_prior_sample_keyed(_lib.ptr(y), _lib.ptr(_dev_keys(KEYS[:B])), SEED, sigma, _lib.ptr(got), B, F, T,
                                           _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, y)
    # the facade: one launch, no noise tensor
    from flowmse_amd.odes import FLOWMATCHING
    ode = FLOWMATCHING()
    x, none = ode.prior_sampling(y.shape, y, keys=KEYS[:B], seed=SEED)
    assert none is None and torch.equal(x, ode.prior_sampling(y.shape, y, z)[0])
    assert torch.equal(ode.prior_sampling(y.shape, y, keys=_dev_keys(KEYS[:B]), seed=SEED)[0], x)
    with pytest.raises(ValueError):
        ode.prior_sampling(y.shape, y, z, keys=KEYS[:B])
    # CPU and GPU callers get the same noise: sigma x the kernel's distance from the restatement, plus the rounding of
    # the final add on either side (half an ulp of the largest part each)
    xc = ode.prior_sampling(y.shape, y.cpu(), keys=KEYS[:B], seed=SEED)[0]
    tol = NOISE_BOUND * ode.prior_std() + float(np.spacing(np.float32(torch.view_as_real(xc).abs().max().item())))
    assert (x.cpu() - xc).abs().max().item() <= tol


# ---------------------------------------------------------------------------------------------------- 12
def test_addressing_invariances_on_the_device():
    keys = KEYS[:4]
    z128, z64 = _noise(keys, SEED, 64, 128), _noise(keys, SEED, 64, 64)
    assert torch.equal(z128[..., :64], z64)                                       # padded length
    for b, k in enumerate(keys):                                                  # batch size and row
        assert torch.equal(_noise([k], SEED, 64, 64)[0], z64[b])
    perm = [2, 0, 3, 1]
    assert torch.equal(_noise([keys[i] for i in perm], SEED, 64, 64), z64[perm])  # order
    assert not torch.equal(z64[0], z64[1]) and not torch.equal(_noise(keys, SEED + 1, 64, 64), z64)


# ---------------------------------------------------------------------------------------------------- 13
@pytest.mark.parametrize("solver", ["euler", "rk4"])
def test_white_box_solver_keys_equal_explicit_noise(tiny, solver):
    from flowmse_amd.sampling import get_white_box_solver
    B, F, T = 2, 64, 64
    y = C.c64(synth.synth_spectrogram(1, B, F, T)).cuda()
    z = _noise(KEYS[:B], 11, F, T)
    want, n = get_white_box_solver(solver, tiny.ode, tiny, y, N=3, z=z)()
    got, m = get_white_box_solver(solver, tiny.ode, tiny, y, N=3, noise_keys=KEYS[:B], noise_seed=11)()
    torch.cuda.synchronize()
    assert n == m == 3 and torch.isfinite(torch.view_as_real(want)).all() and torch.equal(got, want)
    other, _ = get_white_box_solver(solver, tiny.ode, tiny, y, N=3, noise_keys=KEYS[:B], noise_seed=12)()
    assert not torch.equal(other, want)


def test_multi_solver_three_lanes_keys_equal_single_solvers(tiny):
    from flowmse_amd.sampling import get_white_box_solver, get_white_box_solver_multi
    shapes = [(1, 64), (2, 128), (1, 192)]
    Ys = [C.c64(synth.synth_spectrogram(20 + i, B, 64, T)).cuda() for i, (B, T) in enumerate(shapes)]
    keys = [[KEYS[0]], [KEYS[1], KEYS[2]], [KEYS[3]]]
    got, n = get_white_box_solver_multi("euler", tiny.ode, tiny, Ys, N=4, lanes=3, noise_keys=keys, noise_seed=5)()
    torch.cuda.synchronize()
    assert n == 4 and len(got) == 3
    for g, Y, k in zip(got, Ys, keys):
        assert torch.equal(g, get_white_box_solver("euler", tiny.ode, tiny, Y, N=4, noise_keys=k, noise_seed=5)()[0])
        assert torch.equal(g, get_white_box_solver("euler", tiny.ode, tiny, Y, N=4, z=_noise(k, 5, 64, Y.shape[-1]))()[0])
    with pytest.raises(ValueError):
        get_white_box_solver_multi("euler", tiny.ode, tiny, Ys, N=4, noise_keys=keys[:2])


def test_black_box_rk45_accepts_keys(tiny, monkeypatch):
    from scipy import integrate
    from flowmse_amd.sampling import get_black_box_solver
    B, F, T = 2, 64, 64
    y = C.c64(synth.synth_spectrogram(3, B, F, T)).cuda()
    want, nw = get_black_box_solver(tiny.ode, tiny, y, rtol=1e-3, atol=1e-3, z=_noise(KEYS[:B], 9, F, T))()

    def _no_scipy(*a, **k):
        raise AssertionError("solve_ivp called on the fused path")

    monkeypatch.setattr(integrate, "solve_ivp", _no_scipy)
    got, ng = get_black_box_solver(tiny.ode, tiny, y, rtol=1e-3, atol=1e-3, noise_keys=KEYS[:B], noise_seed=9)()
    assert ng == nw and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------- 14
def test_bad_arguments_return_a_status_and_launch_nothing():
    B, F, T = 2, 8, 16
    y = torch.zeros(B, 1, F, T, dtype=torch.complex64, device="cuda")
    out = torch.full_like(y, 7.0)
    kd = _dev_keys(KEYS[:B])
    s = _lib.current_stream()
    p = _lib.ptr
    bad_prior = [(None, p(kd), p(out), B, F, T), (p(y), None, p(out), B, F, T), (p(y), p(kd), None, B, F, T),
                 (p(y), p(kd), p(out), 0, F, T), (p(y), p(kd), p(out), B, -1, T), (p(y), p(kd), p(out), B, F, 0),
                 (p(y), p(kd), p(out), B, F, T - 1)]
    for yy, kk, oo, b, f, t in bad_prior:
        assert L.flowse_prior_sample_keyed(yy, kk, 1, 0.5, oo, b, f, t, s) == ERR_ARG
        assert b"flowse_prior_sample_keyed" in L.flowse_last_error()
    bad_noise = [(None, p(out), B, F, T), (p(kd), None, B, F, T), (p(kd), p(out), 0, F, T), (p(kd), p(out), B, 0, T),
                 (p(kd), p(out), B, F, -2), (p(kd), p(out), B, F, 15)]
    for kk, oo, b, f, t in bad_noise:
        assert L.flowse_op_keyed_noise(kk, 1, oo, b, f, t, s) == ERR_ARG
        assert b"flowse_op_keyed_noise" in L.flowse_last_error()
    with pytest.raises(_lib.FlowseError):
        _lib.check(L.flowse_op_keyed_noise(p(kd), 1, p(out), B, F, 15, s))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                               # nothing was written
    from flowmse_amd.odes import FLOWMATCHING
    with pytest.raises(ValueError):
        FLOWMATCHING().prior_sampling((1, 1, 8, 15), torch.zeros(1, 1, 8, 15, dtype=torch.complex64, device="cuda"), keys=[1])


# ---------------------------------------------------------------------------------------------------- 15
def _evaluate(out, extra, limit=400, env=None):
    """One CLI child under its own time limit; returns (completed process, wall seconds)."""
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "flowmse_amd.evaluate",
                        "--folder_destination", str(out)] + extra, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, **(env or {})))
    return r, time.time() - t0


def _same_tree(a, b, what):
    names = sorted(os.listdir(a / "files"))
    assert names == sorted(os.listdir(b / "files")), what
    for n in names:
        assert filecmp.cmp(a / "files" / n, b / "files" / n, shallow=False), f"{n} differs: {what}"
    assert (a / "_results.csv").read_bytes() == (b / "_results.csv").read_bytes(), f"_results.csv differs: {what}"
    return names


@pytest.mark.timeout(2400)
def test_evaluate_keyed_same_files_across_gpus_streams_and_sets(tmp_path):
    """(a) --gpus 1, (b) --gpus 2 (two ranks sharing device 0 over gloo), (c) --gpus 1 --streams 2 write the same wav bytes
    and the same _results.csv; a 3-file set and a 5-file set give their three common files the same bytes.  Children run
    one after the other; a failed one ends the test."""
    common = ["--synthetic", "5", "--synthetic_seconds", "1.0,2.0,3.0", "--batch", "2", "--noise", "keyed", "--seed", "7"]
    share = {"FLOWSE_EVAL_SHARE_GPU": "1", "FLOWSE_EVAL_BACKEND": "gloo"}
    arms = {"a": (["--gpus", "1"], None), "b": (["--gpus", "2"], share), "c": (["--gpus", "1", "--streams", "2"], None)}
    for tag, (extra, env) in arms.items():
        r, dt = _evaluate(tmp_path / tag, common + extra, env=env)
        print(f"arm ({tag}) {' '.join(extra)}: {dt:.1f} s wall (process start to exit)")
        assert r.returncode == 0, f"arm ({tag}) exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    assert len(_same_tree(tmp_path / "a", tmp_path / "b", "--gpus 1 against --gpus 2")) == 5
    _same_tree(tmp_path / "a", tmp_path / "c", "--streams 1 against --streams 2")
    settings = (tmp_path / "b" / "_settings.txt").read_text()
    assert settings.endswith("noise: keyed\nnoise seed: 7\ngpus: 2\n")
    for n, tag in ((3, "set3"), (5, "set5")):
        r, dt = _evaluate(tmp_path / tag, ["--synthetic", str(n), "--synthetic_seconds", "1.0,2.0,3.0", "--batch", "1",
                                           "--noise", "keyed", "--seed", "7"])
        assert r.returncode == 0, f"{tag} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    names = sorted(os.listdir(tmp_path / "set3" / "files"))
    assert len(names) == 3 and len(os.listdir(tmp_path / "set5" / "files")) == 5
    for n in names:
        assert filecmp.cmp(tmp_path / "set3" / "files" / n, tmp_path / "set5" / "files" / n, shallow=False), n


# ---------------------------------------------------------------------------------------------------- 16
@pytest.mark.timeout(600)
def test_evaluate_two_gpus_refused_without_two_devices(tmp_path):
    """``--gpus 2`` with one visible device (the child sees only the first one, whatever the box has) must not run."""
    env = {k: v for k, v in os.environ.items() if k not in ("FLOWSE_EVAL_SHARE_GPU", "FLOWSE_EVAL_BACKEND")}
    env["HIP_VISIBLE_DEVICES"] = (os.environ.get("HIP_VISIBLE_DEVICES") or "0").split(",")[0]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "flowmse_amd.evaluate", "--folder_destination",
                        str(tmp_path / "o"), "--synthetic", "2", "--gpus", "2"], cwd=ROOT, capture_output=True, text=True,
                       env=env)
    assert r.returncode != 0
    assert "needs 2 visible devices" in r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "o" / "files") or not os.listdir(tmp_path / "o" / "files")
