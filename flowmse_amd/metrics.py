"""Evaluation metrics on the device: ESTOI and SI-SDR / SI-SIR / SI-SAR (``evaluate --metrics device``).

ESTOI is DEFINED here (and in ``include/flowse_hip.h``), step by step after ``pystoi.stoi(x, y, 16000,
extended=True)`` of pystoi 0.3 / 0.4, in float64, for float32 waveforms at 16 kHz of equal length (clean ``x``, processed
``y``), ``EPS = 2**-52``:

    1. 10 kHz: fc = 1/16, t = -290 .. 290, h = kaiser(581, 0.1102 (60 - 8.7)) * 2 * 5 * fc * sinc(2 fc t), h /= sum(h);
       x10 = scipy.signal.resample_poly(x, 5, 8, window=h), length ceil(5 L / 8)
    2. w = hanning(258)[1:-1]; frames start at range(0, L10 - 256, 128); e[i] = 20 log10(|w x10[s_i : s_i + 256]| + EPS) on
       the clean signal; frame i is kept iff max(e) - 40 - e[i] < 0; both signals are rebuilt by overlap-adding their K kept
       windowed frames at hop 128
    3. the rebuilt signals are framed the same way (K - 1 frames, w again), 512-point real DFT, 15 third-octave bands
       (``BANDS``): X_tob[b][j] = sqrt(sum over the band of |X[k][j]|^2)
    4. K - 1 < 30 or L10 <= 256: the result is 1e-5 (pystoi warns and returns it for too few frames; for none it would raise)
    5. segments m = 30 .. K - 1 take columns [m - 30, m) of both band matrices; each 15 x 30 segment is normalised -- row
       mean over time subtracted, rows divided by (|row| + EPS), column mean over bands subtracted, columns divided by
       (|col| + EPS) -- and d = sum(x_n y_n) / 30 / (number of segments)

EQUALITY WITH PYSTOI HAS NOT BEEN CHECKED: the package is not available where this project is built and tested.
``estoi_reference`` is the float64 numpy / scipy restatement of the five steps; the kernels (csrc/metrics.hip) are held
to it, and ``tests/test_metrics_host.py`` compares it with ``pystoi.stoi`` where a user has the package.

The energy ratios follow the reference's ``energy_ratios(s_hat, s, n)`` (utils.py:26-35) in float64 with ``n = y - x``,
in two passes, so that a small artefact term is not found by cancellation.
"""
import ctypes as C

import numpy as np
import torch

from flowmse_amd import _lib

SR = 16000
MAX_SAMPLES = 1 << 24
EPS = float(np.finfo(np.float64).eps)
# bin ranges [lo, hi) of the 15 third-octave bands: pystoi's thirdoct(10000, 512, 15, 150)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
         (87, 109), (109, 138), (138, 174), (174, 219))
_FRAME, _HOP, _NFFT, _SEG = 256, 128, 512, 30


def _check_rate(sr):
    if int(sr) != SR:
        raise ValueError(f"metrics: signals must be at {SR} Hz, got {sr} Hz")


def estoi_taps():
    """The 581 taps ``h`` of step 1 (sum 1) in float64, from ``flowse_estoi_taps`` (host only)."""
    n = int(_lib.lib.flowse_estoi_num_taps())
    taps = np.empty(n, dtype=np.float64)
    _lib.check(_lib.lib.flowse_estoi_taps(taps.ctypes.data_as(C.POINTER(C.c_double)), n))
    return taps


def taps_formula():
    """The same taps from numpy alone: the formula of step 1 as written."""
    fc = 1.0 / 16.0
    half = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2 * 5 * fc * np.sinc(2 * fc * t))
    return h / np.sum(h)


def _window():
    return np.hanning(_FRAME + 2)[1:-1]


def _frames(x):
    """Windowed frames [n, 256] of a 1-D float64 signal: starts range(0, len - 256, 128), the end exclusive."""
    w = _window()
    starts = range(0, x.shape[0] - _FRAME, _HOP)
    if len(starts) == 0:
        return np.zeros((0, _FRAME))
    return np.stack([w * x[s:s + _FRAME] for s in starts])


def reference_stages(x, x_hat, sr=SR):
    """The intermediate results of ``estoi_reference`` as a dict: ``L10``, ``energies`` (dB, first-pass frames of the clean
    signal), ``margins`` (max(e) - 40 - e[i]: a frame is kept iff negative), ``kept`` (K), ``frames`` (K - 1, -1 when no
    frame exists) and ``d``."""
    from scipy.signal import resample_poly
    _check_rate(sr)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(x_hat, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or x.shape[0] < 1:
        raise ValueError(f"estoi takes two 1-D signals of equal length, got shapes {x.shape} and {y.shape}")
    h = taps_formula()
    x10 = resample_poly(x, 5, 8, window=h)
    y10 = resample_poly(y, 5, 8, window=h)
    out = dict(L10=x10.shape[0], energies=np.zeros(0), margins=np.zeros(0), kept=0, frames=-1, d=1e-5)
    xf, yf = _frames(x10), _frames(y10)
    if xf.shape[0] == 0:
        return out
    e = 20.0 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    margins = np.max(e) - 40.0 - e
    mask = margins < 0
    xf, yf = xf[mask], yf[mask]
    K = xf.shape[0]
    out.update(energies=e, margins=margins, kept=K, frames=K - 1)
    if K - 1 < _SEG:
        return out
    xs, ys = np.zeros((K - 1) * _HOP + _FRAME), np.zeros((K - 1) * _HOP + _FRAME)
    for i in range(K):
        xs[i * _HOP:i * _HOP + _FRAME] += xf[i]
        ys[i * _HOP:i * _HOP + _FRAME] += yf[i]
    X = np.fft.rfft(_frames(xs), n=_NFFT, axis=1).T                # [257, K - 1]
    Y = np.fft.rfft(_frames(ys), n=_NFFT, axis=1).T
    x_tob = np.sqrt(np.stack([np.sum(np.abs(X[lo:hi]) ** 2, axis=0) for lo, hi in BANDS]))
    y_tob = np.sqrt(np.stack([np.sum(np.abs(Y[lo:hi]) ** 2, axis=0) for lo, hi in BANDS]))
    n_frames = x_tob.shape[1]
    assert n_frames == K - 1

    def normalise(tob):
        s = np.stack([tob[:, m - _SEG:m] for m in range(_SEG, n_frames + 1)])      # [segments, 15, 30]
        s = s - np.mean(s, axis=2, keepdims=True)
        s = s / (np.sqrt(np.sum(s * s, axis=2, keepdims=True)) + EPS)
        s = s - np.mean(s, axis=1, keepdims=True)
        return s / (np.sqrt(np.sum(s * s, axis=1, keepdims=True)) + EPS)

    xn, yn = normalise(x_tob), normalise(y_tob)
    out["d"] = float(np.sum(xn * yn) / _SEG / xn.shape[0])
    return out


def estoi_reference(x, x_hat, sr=SR):
    """ESTOI of clean ``x`` and processed ``x_hat`` by the float64 numpy / scipy restatement of the module docstring, on the
    CPU.  The oracle of the device path."""
    return reference_stages(x, x_hat, sr)["d"]


def energy_ratios_reference(x_hat, x, y):
    """(SI-SDR, SI-SIR, SI-SAR) in dB in float64: ``evaluate.energy_ratios`` on the widened signals with n = y - x."""
    from flowmse_amd.evaluate import energy_ratios as host
    x_hat, x, y = (np.asarray(a, dtype=np.float64) for a in (x_hat, x, y))
    return tuple(float(v) for v in host(x_hat, x, y - x))


# ---------------------------------------------------------------------------------------------------- the device path
_workspaces = {}                 # (device index, stream, size class) -> uint8 tensor


def workspace_bytes(L):
    n = int(_lib.lib.flowse_metrics_workspace_bytes(int(L)))
    if n < 0:
        _lib.check(-n)
    return n


def _workspace(device, L):
    """The cached workspace of a size class (the next power of two >= L, 2^14 at least) on ``device`` for the current
    stream: calls queued on one stream share it in order; another stream gets its own."""
    if not 1 <= L <= MAX_SAMPLES:
        raise ValueError(f"metrics: signals of 1 .. {MAX_SAMPLES} samples, got {L}")
    cls = max(1 << 14, 1 << (int(L) - 1).bit_length())
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, cls)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(workspace_bytes(cls), dtype=torch.uint8, device=device)
    return ws


def _device_signal(a, device, name):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else np.array(a))
    if not isinstance(a, torch.Tensor) or a.dim() != 1 or a.dtype != torch.float32:
        raise ValueError(f"metrics: {name} must be a 1-D float32 array or tensor, got "
                         f"{getattr(a, 'dtype', type(a))} {tuple(getattr(a, 'shape', ()))}")
    return a.to(device).contiguous()


def _pick_device(*arrays):
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _same_length(sigs):
    L = sigs[0].shape[0]
    if L < 1 or any(s.shape[0] != L for s in sigs):
        raise ValueError(f"metrics: signals of equal length >= 1, got {[int(s.shape[0]) for s in sigs]}")
    return L


def metrics_device(x, y, x_hat, out=None, sr=SR):
    """Queue ESTOI(x, x_hat) and the energy ratios of (x_hat, x, y) -- clean ``x``, noisy ``y``, enhanced ``x_hat``: 1-D
    float32 numpy arrays (uploaded) or tensors -- on the current stream and return the device ``float64[4]`` tensor
    ``(estoi, si_sdr, si_sir, si_sar)`` WITHOUT synchronising.  ``out``: a contiguous float64[4] device tensor to fill."""
    _check_rate(sr)
    device = out.device if out is not None else _pick_device(x, y, x_hat)
    xd, yd, hd = (_device_signal(a, device, n) for a, n in ((x, "x"), (y, "y"), (x_hat, "x_hat")))
    L = _same_length((xd, yd, hd))
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=device)
    elif out.dtype != torch.float64 or out.shape != (4,) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"metrics_device: out must be a contiguous float64[4] device tensor, got {out.dtype} {tuple(out.shape)}")
    with torch.cuda.device(device):
        ws = _workspace(device, L)
        stream = _lib.current_stream()
        _lib.check(_lib.lib.flowse_estoi(_lib.ptr(xd), _lib.ptr(hd), L, _lib.ptr(ws), ws.numel(), _lib.ptr(out), stream))
        _lib.check(_lib.lib.flowse_energy_ratios(_lib.ptr(hd), _lib.ptr(xd), _lib.ptr(yd), L, _lib.ptr(ws), ws.numel(),
                                                 C.c_void_p(out.data_ptr() + 8), stream))
    return out


def estoi(x, x_hat, sr=SR):
    """ESTOI of clean ``x`` and processed ``x_hat`` (1-D float32 numpy arrays or tensors) on the device, as a Python float
    (one read-back)."""
    _check_rate(sr)
    device = _pick_device(x, x_hat)
    xd, hd = _device_signal(x, device, "x"), _device_signal(x_hat, device, "x_hat")
    L = _same_length((xd, hd))
    out = torch.empty(1, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        ws = _workspace(device, L)
        _lib.check(_lib.lib.flowse_estoi(_lib.ptr(xd), _lib.ptr(hd), L, _lib.ptr(ws), ws.numel(), _lib.ptr(out),
                                         _lib.current_stream()))
    return float(out.item())


def energy_ratios(x_hat, x, y, sr=SR):
    """(SI-SDR, SI-SIR, SI-SAR) in dB of enhanced ``x_hat`` against clean ``x`` and noisy ``y`` on the device, as Python
    floats (one read-back)."""
    _check_rate(sr)
    device = _pick_device(x_hat, x, y)
    hd, xd, yd = (_device_signal(a, device, n) for a, n in ((x_hat, "x_hat"), (x, "x"), (y, "y")))
    L = _same_length((hd, xd, yd))
    out = torch.empty(3, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        ws = _workspace(device, L)
        _lib.check(_lib.lib.flowse_energy_ratios(_lib.ptr(hd), _lib.ptr(xd), _lib.ptr(yd), L, _lib.ptr(ws), ws.numel(),
                                                 _lib.ptr(out), _lib.current_stream()))
    return tuple(float(v) for v in out.tolist())
