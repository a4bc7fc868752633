"""GPU: the fused RK45 black-box sampler (flowse_rk45_sample) against scipy's solve_ivp over the same HIP field.

The host path is the same HIP model behind a plain lambda, which sends get_black_box_solver to scipy: both paths see
the bitwise-same vector field, so the fused controller must take scipy's steps -- equal nfev, equal accepted times --
and reach scipy's end point.  The step-for-step checks hold for the scipy the controller ports (1.15.x); with another
minor version they are skipped and the end-point / nfev-band checks still run.
"""
import math

import pytest
import scipy
import torch

import _cases as C
from flowmse_amd.util import synth

pytestmark = pytest.mark.gpu

SCIPY_PORTED = tuple(int(v) for v in scipy.__version__.split(".")[:2]) == (1, 15)
T_REV, T_EPS = 1.0, 0.03


def _model(cfg):
    from flowmse_amd.model import VFModel
    m = VFModel(backbone="ncsnpp", ode="flowmatching", **cfg)
    sd = {n: torch.from_numpy(synth.synth_param(n, tuple(p.shape))) for n, p in m.dnn.named_parameters()}
    m.dnn.load_state_dict(sd)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    return _model(C.TINY)


@pytest.fixture(scope="module")
def full():
    assert torch.cuda.is_available()
    return _model(C.FULL)


def _inputs(seed, B, F, T):
    y = C.c64(synth.synth_spectrogram(seed, B, F, T)).cuda()
    z = C.c64(synth.synth_noise(seed, B, F, T)).cuda()
    return y, z


def _host(model, y, z, rtol, atol, **kw):
    """get_black_box_solver's scipy path, spelled out so that solution.t is visible: (x, nfev, accepted times)."""
    from scipy import integrate
    from flowmse_amd.sampling import from_flattened_numpy, to_flattened_numpy
    with torch.no_grad():
        x = model.ode.prior_sampling(y.shape, y, z)[0]

        def ode_func(t, xf):
            xt = from_flattened_numpy(xf, y.shape).to(y.device).type(torch.complex64)
            vec_t = torch.ones(y.shape[0], device=xt.device) * t
            return to_flattened_numpy(model(xt, vec_t, y))

        sol = integrate.solve_ivp(ode_func, (T_REV, T_EPS), to_flattened_numpy(x), rtol=rtol, atol=atol,
                                  method="RK45", **kw)
    x = torch.tensor(sol.y[:, -1]).reshape(y.shape).type(torch.complex64)
    return x, sol.nfev, list(sol.t[1:])


def _fused(model, y, z, rtol, atol, **kw):
    with torch.no_grad():
        x = model.ode.prior_sampling(y.shape, y, z)[0].contiguous()
        x, nfev, status, times = model.rk45_sample_(x, y, T_REV, T_EPS, rtol, atol, **kw)
    assert status == 0
    return x.cpu(), nfev, times


def _compare(model, y, z, rtol, atol, tag, **kw):
    print("scipy", scipy.__version__)
    xh, nh, th = _host(model, y, z, rtol, atol, **kw)
    xf, nf, tf = _fused(model, y, z, rtol, atol, **kw)
    err = C.rel_l2(xf, xh)
    dt = max(abs(a - b) / abs(b) for a, b in zip(tf, th)) if len(tf) == len(th) else math.inf
    print(f"{tag}: nfev fused {nf} host {nh}; accepted {len(tf)} / {len(th)}; max rel dt {dt:.3e}; "
          f"endpoint rel-L2 {err:.3e}")
    assert torch.isfinite(torch.view_as_real(xf)).all()
    if SCIPY_PORTED:
        assert nf == nh
        assert len(tf) == len(th) and dt <= 1e-12
    else:
        assert abs(nf - nh) <= 12, f"scipy {scipy.__version__} is not the ported 1.15"
    assert err <= 1e-5
    return nf


@pytest.mark.parametrize("tol", [1e-4, 1e-5])
def test_tiny_matches_scipy(tiny, tol):
    """Measured on MI355X (scipy 1.15.3): tol 1e-4: nfev 494 both, 74 accepted steps, times within 8.9e-16, end points
    bit-equal; tol 1e-5: nfev 1424 both, 205 steps, times within 3.2e-15, end points bit-equal."""
    y, z = _inputs(0, 2, 64, 64)
    _compare(tiny, y, z, tol, tol, f"tiny [2,1,64,64] tol {tol:g}")


@pytest.mark.parametrize("B,T", [(1, 64), (2, 128)])
def test_full_matches_scipy(full, B, T):
    """One error norm over the whole batch (the reference integrates the batch as one ODE system).  Measured on MI355X:
    [1,1,256,64] nfev 950 both, 152 steps; [2,1,256,128] nfev 962 both, 154 steps; times and end points bit-equal."""
    y, z = _inputs(7, B, 256, T)
    _compare(full, y, z, 1e-5, 1e-5, f"full [{B},1,256,{T}]")


@pytest.mark.parametrize("kw", [{"first_step": 0.05}, {"max_step": 0.1}, {"first_step": 0.01, "max_step": 0.2}])
def test_first_and_max_step(tiny, kw):
    """Measured on MI355X: nfev 487 / 482 / 481 on both paths, times within 3.6e-15, end points bit-equal."""
    y, z = _inputs(1, 2, 64, 64)
    _compare(tiny, y, z, 1e-4, 1e-4, f"tiny {kw}", **kw)


def test_deterministic(tiny):
    y, z = _inputs(2, 2, 64, 64)
    a, na, ta = _fused(tiny, y, z, 1e-5, 1e-5)
    b, nb, tb = _fused(tiny, y, z, 1e-5, 1e-5)
    assert torch.equal(a, b) and na == nb and ta == tb


def test_black_box_solver_takes_fused_path(tiny, monkeypatch):
    """get_black_box_solver on the HIP model never calls solve_ivp, and returns scipy's nfev and end point."""
    from scipy import integrate
    from flowmse_amd.sampling import get_black_box_solver
    y, z = _inputs(3, 2, 64, 64)
    host, nh = get_black_box_solver(tiny.ode, lambda x, t, yy: tiny(x, t, yy), y, rtol=1e-4, atol=1e-4, z=z)()

    def _no_scipy(*a, **k):
        raise AssertionError("solve_ivp called on the fused path")

    monkeypatch.setattr(integrate, "solve_ivp", _no_scipy)
    got, nf = get_black_box_solver(tiny.ode, tiny, y, rtol=1e-4, atol=1e-4, z=z)()
    print("get_black_box_solver fused nfev", nf, "host", nh, "rel-L2", C.rel_l2(got.cpu(), host.cpu()))
    assert got.dtype == torch.complex64 and got.shape == y.shape and got.is_cuda
    if SCIPY_PORTED:
        assert nf == nh
    assert C.rel_l2(got.cpu(), host.cpu()) <= 1e-5


@pytest.mark.parametrize("case", ["rk23", "t_eval", "host_override"])
def test_fallback_reaches_scipy(tiny, monkeypatch, case):
    """Calls outside the fused path run scipy exactly as before: bit-equal to the lambda-wrapped field."""
    from flowmse_amd.sampling import get_black_box_solver
    y, z = _inputs(4, 2, 64, 64)
    method = "RK23" if case == "rk23" else "RK45"
    kw = {"t_eval": [T_REV, 0.5, T_EPS]} if case == "t_eval" else {}
    if case == "host_override":
        monkeypatch.setenv("FLOWSE_RK45_HOST", "1")
    a, na = get_black_box_solver(tiny.ode, tiny, y, rtol=1e-3, atol=1e-3, method=method, z=z)(**kw)
    b, nb = get_black_box_solver(tiny.ode, lambda x, t, yy: tiny(x, t, yy), y, rtol=1e-3, atol=1e-3, method=method,
                                 z=z)(**kw)
    assert na == nb and torch.equal(a, b)


# measured on MI355X: see the docstring of test_16bit_modes
NFEV_BAND_16 = 1.2


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_16bit_modes(full, mode):
    """16-bit storage modes: the solve finishes with a finite end point and an nfev within NFEV_BAND_16 x of fp32.
    Measured on MI355X ([1,1,256,64], tol 1e-5): fp32 926; bf16 932 (end point 4.4e-3 rel-L2 from fp32); fp16 926
    (3.6e-4)."""
    y, z = _inputs(5, 1, 256, 64)
    x32, n32, _ = _fused(full, y, z, 1e-5, 1e-5)
    full.dnn.set_precision(mode)
    try:
        x16, n16, _ = _fused(full, y, z, 1e-5, 1e-5, max_nfev=20000)
    finally:
        full.dnn.set_precision("fp32")
    err = C.rel_l2(x16, x32)
    print(f"{mode}: nfev {n16} (fp32 {n32}), endpoint rel-L2 vs fp32 {err:.3e}")
    assert torch.isfinite(torch.view_as_real(x16)).all()
    assert n32 / NFEV_BAND_16 <= n16 <= n32 * NFEV_BAND_16


def test_graph_replay(tiny, monkeypatch):
    """Under FLOWSE_GRAPH=1 (read when the handle is created) every evaluation is a hipGraph launch; same solve."""
    monkeypatch.setenv("FLOWSE_GRAPH", "1")
    g = _model(C.TINY)
    monkeypatch.delenv("FLOWSE_GRAPH")
    y, z = _inputs(6, 2, 64, 64)
    a, na, ta = _fused(tiny, y, z, 1e-4, 1e-4)
    b, nb, tb = _fused(g, y, z, 1e-4, 1e-4)
    print("graph launches", g.dnn.graph_launches(), "nfev", nb)
    assert g.dnn.graph_launches() > 0
    assert na == nb and ta == tb and torch.equal(a, b)
