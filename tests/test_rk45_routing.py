"""CPU: which black-box calls take the fused RK45 path (flowse_rk45_sample) and which stay on scipy."""
import os
import re

import numpy as np
import pytest

from flowmse_amd.sampling import fused_rk45

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _HipField:
    """Stands in for a HIP-backed VFModel: only the attribute the predicate looks for."""

    def rk45_sample_(self, *a, **k):
        raise AssertionError("not called by the predicate")

    def __call__(self, x, t, y):
        raise AssertionError("not called by the predicate")


class _Dev:
    def __init__(self, cuda):
        self.is_cuda = cuda


CUDA, CPU = _Dev(True), _Dev(False)


@pytest.fixture(autouse=True)
def _no_host_override(monkeypatch):
    monkeypatch.delenv("FLOWSE_RK45_HOST", raising=False)


def test_fused_when_every_condition_holds():
    assert fused_rk45("RK45", _HipField(), CUDA, 1e-5, 1e-5, {})
    assert fused_rk45("RK45", _HipField(), CUDA, 1e-4, 0, {"first_step": 1e-3})
    assert fused_rk45("RK45", _HipField(), CUDA, np.float64(1e-5), 1e-5, {"first_step": None, "max_step": 0.1})


@pytest.mark.parametrize("method", ["RK23", "DOP853", "Radau", "rk45"])
def test_other_methods_use_scipy(method):
    assert not fused_rk45(method, _HipField(), CUDA, 1e-5, 1e-5, {})


def test_solver_class_uses_scipy():
    from scipy.integrate import RK45
    assert not fused_rk45(RK45, _HipField(), CUDA, 1e-5, 1e-5, {})


def test_plain_callable_field_uses_scipy():
    field = _HipField()
    assert not fused_rk45("RK45", lambda x, t, y: field(x, t, y), CUDA, 1e-5, 1e-5, {})


def test_host_state_uses_scipy():
    assert not fused_rk45("RK45", _HipField(), CPU, 1e-5, 1e-5, {})
    assert not fused_rk45("RK45", _HipField(), object(), 1e-5, 1e-5, {})


@pytest.mark.parametrize("rtol,atol", [(np.full(4, 1e-5), 1e-5), (1e-5, np.full(4, 1e-5)), ([1e-5], 1e-5),
                                       (1e-5, np.array([1e-5])), (1e-5 + 0j, 1e-5)])
def test_array_or_complex_tolerances_use_scipy(rtol, atol):
    assert not fused_rk45("RK45", _HipField(), CUDA, rtol, atol, {})


@pytest.mark.parametrize("kw", [{"t_eval": [0.5]}, {"dense_output": True}, {"events": lambda t, y: t},
                                {"vectorized": False}, {"args": ()}, {"first_step": 1e-3, "t_eval": [0.5]}])
def test_other_solver_options_use_scipy(kw):
    assert not fused_rk45("RK45", _HipField(), CUDA, 1e-5, 1e-5, kw)


def test_host_override(monkeypatch):
    monkeypatch.setenv("FLOWSE_RK45_HOST", "1")
    assert not fused_rk45("RK45", _HipField(), CUDA, 1e-5, 1e-5, {})
    monkeypatch.setenv("FLOWSE_RK45_HOST", "0")
    assert fused_rk45("RK45", _HipField(), CUDA, 1e-5, 1e-5, {})


def test_vfmodel_offers_the_fused_solver():
    from flowmse_amd.backbones.ncsnpp import NCSNpp
    from flowmse_amd.model import VFModel
    assert callable(getattr(VFModel, "rk45_sample_", None))
    assert callable(getattr(NCSNpp, "rk45_sample", None))


def test_cabi_declares_and_exports_rk45():
    from flowmse_amd import _lib
    header = open(os.path.join(ROOT, "include", "flowse_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+flowse_rk45_sample\s*\(", header)
    assert "flowse_rk45_sample" in _lib.SIGNATURES
    assert hasattr(_lib.lib, "flowse_rk45_sample")
