"""Flow-matching probability path used by the sampler.

API mirror of the reference's ``ODERegistry`` / ``FLOWMATCHING`` (flowmse/odes.py:17-107) -- same registry name
``"flowmatching"``, constructor keywords and method names -- written for this package:

    mean(t)  = (1 - t) * x0 + t * y
    sigma(t) = (1 - t) * sigma_min + t * sigma_max          (defaults 0.0 / 0.487)
    prior    : x_T = y + sigma(1) * z,  z ~ CN(0, 1)         (odes.py:93-100)

Only ``prior_sampling`` is on the sampling hot path; on a GPU it is one ``flowse_prior_sample`` launch.
"""
import warnings

import torch

from flowmse_amd.util.registry import Registry

ODERegistry = Registry("ODE")


class ODE:
    """Minimal base: what the sampler needs from a probability path."""

    def marginal_prob(self, x0, t, y):
        raise NotImplementedError

    def prior_sampling(self, shape, y, z=None):
        raise NotImplementedError

    def copy(self):
        raise NotImplementedError


def _bcast(t):
    return t.reshape(-1, 1, 1, 1)


@ODERegistry.register("flowmatching")
class FLOWMATCHING(ODE):
    def __init__(self, sigma_min=0.0, sigma_max=0.487, **_unused):
        self.sigma_min, self.sigma_max = sigma_min, sigma_max

    @staticmethod
    def add_argparse_args(parser):
        for name, default in (("--sigma_min", 0.0), ("--sigma_max", 0.487)):
            parser.add_argument(name, type=float, default=default)
        return parser

    def copy(self):
        return type(self)(self.sigma_min, self.sigma_max)

    # the reference leaves the drift itself unimplemented as well (odes.py:81)
    def ode(self, x, t, *args):
        return None

    # ---- closed forms of the path -------------------------------------------------------------
    def _std(self, t):
        return self.sigma_min * (1 - t) + self.sigma_max * t

    def _mean(self, x0, t, y):
        return _bcast(1 - t) * x0 + _bcast(t) * y

    def marginal_prob(self, x0, t, y):
        return self._mean(x0, t, y), self._std(t)

    def der_mean(self, x0, t, y):
        return y - x0

    def der_std(self, t):
        return self.sigma_max - self.sigma_min

    # ---- prior --------------------------------------------------------------------------------
    def prior_std(self):
        """sigma(1) as the float32 number the reference evaluates for a batch of ones (odes.py:96)."""
        return float(self._std(torch.ones(1, dtype=torch.float32)))

    def prior_sampling(self, shape, y, z=None, *, keys=None, seed=0, frame0=None):
        """Returns ``(x_T, z)``.  ``z`` may be passed in for reproducible trajectories.

        ``keys`` (one 64-bit utterance key per row of ``y`` [B,1,F,T], a sequence of ints or an int64 tensor holding
        the same bits) with ``seed`` selects the keyed noise stream of ``flowmse_amd.util.noise`` instead of the
        process-wide generator: the noise of a row then depends on (seed, key, bin, frame) only.  On a HIP tensor this
        is one ``flowse_prior_sample_keyed`` launch that generates the noise in registers, and the returned ``z`` is
        ``None`` -- the noise never exists as a tensor there.  On a CPU tensor it is the float64 restatement rounded to
        complex64, and ``z`` is returned.  ``keys`` together with ``z`` raises ``ValueError``.

        ``frame0`` (with ``keys`` only: one even frame offset >= 0 per row) addresses the stream at absolute frames: row b
        gets the noise of frames ``frame0[b] ..`` of its key (``flowse_prior_sample_keyed_at``), so the chunks of one long
        recording share their utterance's key and start from the same ``x_T`` wherever they overlap."""
        if tuple(shape) != tuple(y.shape):
            warnings.warn(f"prior_sampling: requested shape {tuple(shape)} differs from y {tuple(y.shape)}; using y's")
        if keys is not None:
            if z is not None:
                raise ValueError("prior_sampling: pass either z or keys, not both")
            return self._prior_sampling_keyed(y, keys, seed, frame0)
        if frame0 is not None:
            raise ValueError("prior_sampling: frame0 addresses the keyed stream; pass keys")
        z = torch.randn_like(y) if z is None else z
        if not y.is_cuda:
            return y + z * _bcast(self._std(torch.ones(y.shape[0], device=y.device))), z
        from flowmse_amd import _lib
        y, zc = y.contiguous(), z.contiguous()
        x_T = torch.empty_like(y)
        with torch.cuda.device(y.device):
            _lib.check(_lib.lib.flowse_prior_sample(_lib.ptr(y), _lib.ptr(zc), self.prior_std(), _lib.ptr(x_T),
                                                    y.numel(), _lib.current_stream()))
        return x_T, z

    def _prior_sampling_keyed(self, y, keys, seed, frame0=None):
        if y.dim() != 4 or y.shape[1] != 1 or y.dtype != torch.complex64:
            raise ValueError(f"prior_sampling(keys=...): y must be complex64 [B,1,F,T], got {y.dtype} {tuple(y.shape)}")
        B, _, F, T = y.shape
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if torch.is_tensor(keys):
            if keys.dtype != torch.int64 or keys.numel() != B:
                raise ValueError(f"prior_sampling: keys must be {B} int64 words, got {keys.dtype} x {keys.numel()}")
            key_list = None if y.is_cuda else [int(k) for k in keys.reshape(-1).tolist()]
        else:
            key_list = [int(k) & 0xFFFFFFFFFFFFFFFF for k in keys]
            if len(key_list) != B:
                raise ValueError(f"prior_sampling: {len(key_list)} keys for a batch of {B}")
        if frame0 is not None:
            from flowmse_amd.util.noise import check_frame0
            frame0 = check_frame0(frame0, B)
        if not y.is_cuda:
            from flowmse_amd.util.noise import keyed_noise_reference
            z = torch.from_numpy(keyed_noise_reference([k & 0xFFFFFFFFFFFFFFFF for k in key_list], seed, F, T,
                                                       frame0=frame0)).to(torch.complex64)
            return y + z * self.prior_std(), z
        from flowmse_amd import _lib
        if T % 2:
            raise ValueError(f"prior_sampling(keys=...): the keyed kernel takes an even number of frames, got T={T}")
        if key_list is None:
            kd = keys.to(y.device).contiguous()
        else:                      # the 64 key bits as int64 (torch has no arithmetic-free uint64 on every build)
            kd = torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in key_list], dtype=torch.int64, device=y.device)
        y = y.contiguous()
        x_T = torch.empty_like(y)
        with torch.cuda.device(y.device):
            if frame0 is None:
                _lib.check(_lib.lib.flowse_prior_sample_keyed(_lib.ptr(y), _lib.ptr(kd), seed, self.prior_std(),
                                                              _lib.ptr(x_T), B, F, T, _lib.current_stream()))
            else:
                fd = torch.tensor(frame0, dtype=torch.int32, device=y.device)
                _lib.check(_lib.lib.flowse_prior_sample_keyed_at(_lib.ptr(y), _lib.ptr(kd), _lib.ptr(fd), seed,
                                                                 self.prior_std(), _lib.ptr(x_T), B, F, T,
                                                                 _lib.current_stream()))
        return x_T, None

    # ---- one training / validation pair of the path (reference VFModel._step, flowmse/model.py:134-140) ----------
    def marginal_sample(self, x0, t, y, z=None, *, keys=None, seed=0, with_target=False):
        """``x_t = mean(t) + sigma(t) z`` and, with ``with_target``, the conditional field
        ``u = der_std z + der_mean = (sigma_max - sigma_min) z + (y - x0)``.  Returns ``(x_t, z_or_None[, u])``.

        ``z=None`` without ``keys`` draws ``torch.randn_like(x0)`` as the reference does; ``keys`` (one 64-bit key per
        row, as in ``prior_sampling``) with ``seed`` takes z from the keyed stream instead.  On HIP tensors this is one
        ``flowse_fm_pair`` launch -- keyed noise is generated in registers and the returned ``z`` is ``None`` -- on CPU
        tensors the tensor formulas of ``marginal_prob`` / ``der_mean`` / ``der_std``."""
        if keys is not None and z is not None:
            raise ValueError("marginal_sample: pass either z or keys, not both")
        if x0.shape != y.shape or x0.dim() != 4 or x0.shape[1] != 1 or x0.dtype != torch.complex64 or y.dtype != x0.dtype:
            raise ValueError(f"marginal_sample: x0, y must be complex64 [B,1,F,T], got {x0.dtype} {tuple(x0.shape)} / "
                             f"{y.dtype} {tuple(y.shape)}")
        B, _, F, T = x0.shape
        if t.shape != (B,):
            raise ValueError(f"marginal_sample: t must have shape [{B}], got {tuple(t.shape)}")
        if keys is None and z is None:
            z = torch.randn_like(x0)
        if not x0.is_cuda:
            if keys is not None:
                from flowmse_amd.util.noise import keyed_noise_reference
                z = torch.from_numpy(keyed_noise_reference(key_words(keys, B), int(seed) & _MASK64, F, T)).to(torch.complex64)
            t = t.to(torch.float32)
            mean, std = self.marginal_prob(x0, t, y)
            x_t = mean + _bcast(std) * z
            return (x_t, z, self.der_std(t) * z + self.der_mean(x0, t, y)) if with_target else (x_t, z)
        from flowmse_amd import _lib
        if T % 2:
            raise ValueError(f"marginal_sample: the kernel takes an even number of frames, got T={T}")
        x0c, yc = x0.contiguous(), y.contiguous()
        zc = None if z is None else z.to(x0.device).contiguous()
        kd = None if keys is None else device_keys(keys, B, x0.device)
        td = t.to(device=x0.device, dtype=torch.float32).contiguous()
        x_t = torch.empty_like(x0c)
        u = torch.empty_like(x0c) if with_target else None
        with torch.cuda.device(x0.device):
            _lib.check(_lib.lib.flowse_fm_pair(_lib.ptr(x0c), _lib.ptr(yc), _lib.ptr(td), _lib.ptr(zc), _lib.ptr(kd),
                                               int(seed) & _MASK64, float(self.sigma_min), float(self.sigma_max),
                                               _lib.ptr(x_t), _lib.ptr(u), B, F, T, _lib.current_stream()))
        return (x_t, z, u) if with_target else (x_t, z)


_MASK64 = 0xFFFFFFFFFFFFFFFF


def key_words(keys, B):
    """The B row keys as Python ints in [0, 2**64): from a sequence of ints or an int64 tensor holding the same bits."""
    words = [int(k) & _MASK64 for k in (keys.reshape(-1).tolist() if torch.is_tensor(keys) else keys)]
    if len(words) != B:
        raise ValueError(f"{len(words)} keys for a batch of {B}")
    return words


def device_keys(keys, B, device):
    """The B row keys as an int64 device tensor holding the 64 key bits (torch has no arithmetic-free uint64 everywhere)."""
    if torch.is_tensor(keys) and keys.dtype == torch.int64 and keys.numel() == B:
        return keys.to(device).contiguous()
    return torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in key_words(keys, B)], dtype=torch.int64, device=device)
