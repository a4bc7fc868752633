"""The flow-matching objective in float64: the definition ``csrc/fmloss.hip`` is held to.

Restated from the reference's ``VFModel._step`` / ``_loss`` (flowmse/model.py:118-143) and ``FLOWMATCHING``
(flowmse/odes.py:83-107); ``pytorch_lightning`` is not available where this package is built and tested, so equality with
the reference's Lightning module itself has not been run.  For a row with clean spectrogram x0, noisy y, time t, noise z:

    sigma(t) = (1 - t) sigma_min + t sigma_max                            odes.py:86-88
    x_t      = (1 - t) x0 + t y + sigma(t) z                              odes.py:83-84, model.py:134-137
    u        = (sigma_max - sigma_min) z + (y - x0)                       odes.py:102-107, model.py:138-140
    loss_b   = 0.5 * sum_{f,frame} |v - u|^2  ('mse')  |  0.5 * sum |v - u|  ('mae')       model.py:118-128
    loss     = mean_b loss_b
"""
import numpy as np

LOSS_TYPES = {"mse": 0, "mae": 1}           # FLOWSE_LOSS_MSE / FLOWSE_LOSS_MAE


def loss_type_code(loss_type):
    try:
        return LOSS_TYPES[loss_type]
    except (KeyError, TypeError):
        raise ValueError(f"unknown loss_type {loss_type!r}: expected 'mse' or 'mae'") from None


def _c128(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a.astype(np.complex128)


def fm_loss_reference(v, x0, y, z, t, sigma_min, sigma_max, loss_type="mse"):
    """``(rows, mean)``: the B row losses (float64 [B]) and their mean for a field ``v`` (complex [B,1,F,T]).  ``t`` is
    part of the signature because it is part of the training step; the conditional field of this path does not depend on
    it, so the value does not either.  Real and imaginary parts are formed separately, in the kernel's operation order:
    ``d = v - (ds * z + (y - x0))`` with ``ds = sigma_max - sigma_min``."""
    code = loss_type_code(loss_type)
    v, x0, y, z = _c128(v), _c128(x0), _c128(y), _c128(z)
    ds = float(sigma_max) - float(sigma_min)
    dre = v.real - (ds * z.real + (y.real - x0.real))
    dim = v.imag - (ds * z.imag + (y.imag - x0.imag))
    q = dre * dre + dim * dim
    terms = np.sqrt(q) if code == 1 else q
    rows = 0.5 * terms.reshape(terms.shape[0], -1).sum(axis=1)
    return rows, float(rows.sum() / rows.shape[0])
