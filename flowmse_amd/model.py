"""VFModel facade: the surface of ``flowmse.model.VFModel`` that ``evaluate.py`` touches, without Lightning.

Reference: flowmse/model.py:19-206.  What evaluate.py uses (evaluate.py:64-132): ``load_from_checkpoint``,
``eval(no_ema=False)`` (= swap the EMA shadow weights in, model.py:92-103), ``.cuda()``, ``.ode``, ``_stft``,
``_forward_transform``, ``to_audio`` and the model itself as ``VF_fn(x, t, y)`` (= ``-dnn(cat[x,y], t)``,
model.py:164-170).  The flow-matching objective is here forward-only (``_loss``, ``_step``, ``loss_rows``: model.py:118-143,
the number ``validation_step`` logs as ``valid_loss``); training itself (backward, optimizer, Lightning hooks, dataloaders)
is out of scope.
"""
import pickle
import types
import warnings

import torch
import torch.nn as nn

from flowmse_amd.backbones import BackboneRegistry
from flowmse_amd.data_module import SpecTransform
from flowmse_amd.odes import ODERegistry


# ---------------------------------------------------------------------------------------------- checkpoint reader
# A reference checkpoint pickles class references from packages that are absent on an inference box:
# hyper_parameters['data_module_cls'] = flowmse.data_module.SpecsDataModule (train.py:58,66 -> save_hyperparameters,
# model.py:66), and Lightning may wrap hyper_parameters in its AttributeDict.  None of them carries information the
# sampler needs, so unknown globals from those packages unpickle to inert placeholders instead of failing.
_FOREIGN_PREFIXES = ("flowmse", "sgmse", "pytorch_lightning", "lightning", "lightning_fabric", "torch_ema",
                     "torchmetrics", "wandb", "omegaconf")


class _ForeignDict(dict):
    """Placeholder for dict-like foreign containers (e.g. pytorch_lightning AttributeDict)."""

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)


def _foreign_placeholder(module, name):
    if name in ("AttributeDict", "DictConfig"):
        return _ForeignDict

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)

    return type(name, (), {"__module__": module, "__init__": __init__, "__setstate__": __setstate__,
                           "_flowse_foreign": True, "__reduce_ex__": object.__reduce_ex__})


class _CkptUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            if module.split(".")[0] in _FOREIGN_PREFIXES:
                return _foreign_placeholder(module, name)
            raise


_ckpt_pickle = types.SimpleNamespace(__name__="flowmse_amd_ckpt_pickle", Unpickler=_CkptUnpickler, load=pickle.load,
                                     loads=pickle.loads, dump=pickle.dump, dumps=pickle.dumps,
                                     UnpicklingError=pickle.UnpicklingError, PickleError=pickle.PickleError)


def read_checkpoint(path, map_location="cpu"):
    """torch.load for a reference (Lightning) checkpoint that works without flowmse / pytorch_lightning /
    torch_ema installed: class references into those packages become placeholders."""
    return torch.load(path, map_location=map_location, weights_only=False, pickle_module=_ckpt_pickle)


def _is_foreign(v):
    return getattr(v, "_flowse_foreign", False) or getattr(type(v), "_flowse_foreign", False)


# constructor keywords the facade understands (VFModel + NCSNpp + FLOWMATCHING + SpecTransform); every other
# hyper-parameter of a training run (dataset paths, loader settings, ...) is ignored with no effect
_KNOWN_HPARAMS = {
    "backbone", "ode", "lr", "ema_decay", "t_eps", "T_rev", "loss_abs_exponent", "num_eval_files", "loss_type",
    # NCSNpp (ncsnpp.py:45-67)
    "scale_by_sigma", "nonlinearity", "nf", "ch_mult", "num_res_blocks", "attn_resolutions", "resamp_with_conv",
    "conditional", "fir", "fir_kernel", "skip_rescale", "resblock_type", "progressive", "progressive_input",
    "progressive_combine", "init_scale", "fourier_scale", "image_size", "embedding_type", "dropout",
    # FLOWMATCHING (odes.py:66-68)
    "sigma_min", "sigma_max",
    # spectrogram transform half of SpecsDataModule (data_module.py:96-105)
    "n_fft", "hop_length", "window", "spec_factor", "spec_abs_exponent", "transform_type",
}


class VFModel(nn.Module):
    def __init__(self, backbone="ncsnpp", ode="flowmatching", lr=1e-4, ema_decay=0.999, t_eps=0.03, T_rev=1.0,
                 loss_abs_exponent=0.5, num_eval_files=10, loss_type="mse", data_module_cls=None, **kwargs):
        super().__init__()
        dnn_cls = BackboneRegistry.get_by_name(backbone)
        self.dnn = dnn_cls(**kwargs)
        ode_cls = ODERegistry.get_by_name(ode)
        self.ode = ode_cls(**kwargs)
        self.lr = lr
        self.ema_decay = ema_decay
        self.t_eps = t_eps
        self.T_rev = T_rev
        self.ode.T_rev = T_rev
        self.loss_type = loss_type
        self.num_eval_files = num_eval_files
        self.loss_abs_exponent = loss_abs_exponent
        self.data_module = SpecTransform(**kwargs) if data_module_cls is None else data_module_cls(**kwargs)
        # EMA state (torch_ema layout: list of tensors in self.parameters() order)
        self._ema_shadow = None
        self._ema_backup = None
        self._error_loading_ema = False

    # ------------------------------------------------------------------ checkpoint / EMA (model.py:81-106)
    def load_ema_shadow(self, shadow_params):
        params = [p for p in self.parameters()]
        trainable = [p for p in params if p.requires_grad]
        if len(shadow_params) == len(params):
            target = params
        elif len(shadow_params) == len(trainable):          # torch_ema keeps requires_grad params only
            target = trainable
        else:
            raise ValueError(f"EMA shadow has {len(shadow_params)} tensors, model has {len(params)} parameters "
                             f"({len(trainable)} trainable)")
        for s, p in zip(shadow_params, target):
            if tuple(s.shape) != tuple(p.shape):
                raise ValueError(f"EMA shadow shape {tuple(s.shape)} != parameter shape {tuple(p.shape)}")
        self._ema_shadow = [s.detach().clone().float() for s in shadow_params]
        self._ema_target = target

    @classmethod
    def load_from_checkpoint(cls, checkpoint_file, map_location="cpu", **overrides):
        """Parse a Lightning checkpoint of the reference without Lightning / torch_ema
        (layout: SURVEY.md section 5: hyper_parameters, state_dict['dnn.*'], ema['shadow_params'])."""
        ckpt = read_checkpoint(checkpoint_file, map_location)
        hp = dict(ckpt.get("hyper_parameters", {}))
        hp.update(overrides)                      # evaluate.py:64-67 passes base_dir / batch_size / num_workers / kwargs
        hp.pop("data_module_cls", None)           # class reference (placeholder here); SpecTransform stands in
        dropped = sorted(k for k in hp if k not in _KNOWN_HPARAMS)
        hp = {k: v for k, v in hp.items() if k in _KNOWN_HPARAMS and not _is_foreign(v)}
        model = cls(**hp)
        model.ignored_hparams = dropped
        sd = {k[len("dnn."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("dnn.")}
        if not sd:
            raise KeyError("checkpoint state_dict has no 'dnn.*' entries (not a flowmse VFModel checkpoint?)")
        model.dnn.load_state_dict(sd)
        ema = ckpt.get("ema")
        if ema is not None and "shadow_params" in ema:
            model.load_ema_shadow(ema["shadow_params"])
        else:
            model._error_loading_ema = True
            warnings.warn("EMA state_dict not found in checkpoint!")
        return model

    def train(self, mode=True, no_ema=False):
        res = super().train(mode)
        if not self._error_loading_ema and self._ema_shadow is not None:
            with torch.no_grad():
                if mode is False and not no_ema:
                    if self._ema_backup is None:
                        self._ema_backup = [p.detach().clone() for p in self._ema_target]
                        for p, s in zip(self._ema_target, self._ema_shadow):
                            p.copy_(s.to(p.device))
                        self.dnn.mark_dirty()
                elif self._ema_backup is not None:
                    for p, b in zip(self._ema_target, self._ema_backup):
                        p.copy_(b)
                    self._ema_backup = None
                    self.dnn.mark_dirty()
        return res

    def eval(self, no_ema=False):
        return self.train(False, no_ema=no_ema)

    # ------------------------------------------------------------------ vector field
    def forward(self, x, t, y):
        """-dnn(cat([x, y], 1), t) (model.py:164-170); x, y complex64 [B,1,F,T] on 'cuda', t float32 [B]."""
        return self.dnn.vf_call(x, t, y, 1)

    # ------------------------------------------------------------------ objective (model.py:118-143), forward only
    def _loss(self, vectorfield, condVF):
        """The reference's ``_loss`` (model.py:118-128): 0.5 * sum over (channel, bin, frame) of |err|^2 ('mse') or |err|
        ('mae'), mean over the batch.  An unknown ``loss_type`` raises (the reference falls through to an unbound name)."""
        from flowmse_amd.fmloss import loss_type_code
        err = vectorfield - condVF
        losses = err.abs() if loss_type_code(self.loss_type) else torch.square(err.abs())
        return torch.mean(0.5 * torch.sum(losses.reshape(losses.shape[0], -1), dim=-1))

    def _loss_draws(self, x0, t, z, keys, seed):
        """(t, z, keys, Philox seed) of one objective evaluation: what is not given is drawn -- from the keyed stream with
        ``keys`` (seed ^ 0x6C6F7373, apart from the sampler's prior noise), else from torch's generator as the reference
        does (model.py:132-135)."""
        from flowmse_amd.util.noise import loss_seed, loss_times
        if keys is not None and z is not None:
            raise ValueError("pass either z or keys, not both")
        B = x0.shape[0]
        if keys is not None:
            from flowmse_amd.odes import key_words
            keys = key_words(keys, B)
        if t is None:
            if keys is not None:
                t = torch.from_numpy(loss_times(keys, loss_seed(seed), self.T_rev, self.t_eps)[:, 0].copy())
            else:
                rdm = (1 - torch.rand(B, device=x0.device)) * (self.T_rev - self.t_eps) + self.t_eps
                t = torch.min(rdm, torch.tensor(self.T_rev, device=x0.device))
        if z is None and keys is None:
            z = torch.randn_like(x0)
        return t.to(x0.device), z, keys, loss_seed(seed)

    def _fm_loss(self, x0, y, t, z, keys, seed):
        """float64 [B + 1]: row losses and their mean.  HIP tensors: one ``flowse_fm_loss`` call."""
        from flowmse_amd.fmloss import loss_type_code
        code = loss_type_code(self.loss_type)
        t, z, keys, pseed = self._loss_draws(x0, t, z, keys, seed)
        if x0.is_cuda:
            from flowmse_amd.odes import device_keys
            kd = None if keys is None else device_keys(keys, x0.shape[0], x0.device)
            return self.dnn.fm_loss(x0, y, t, z, kd, pseed, float(self.ode.sigma_min), float(self.ode.sigma_max), code)
        x_t, _, u = self.ode.marginal_sample(x0, t, y, z, keys=keys, seed=pseed, with_target=True)
        err = (self(x_t, t, y) - u).abs().double()
        rows = 0.5 * (err if code else err * err).reshape(err.shape[0], -1).sum(-1)
        return torch.cat([rows, rows.mean().reshape(1)])

    def _step(self, batch, batch_idx=None, *, t=None, z=None, keys=None, seed=0):
        """The reference's ``_step`` (model.py:130-143), forward only: the flow-matching loss of ``batch = (x0, y)`` as a
        0-d float64 tensor on the inputs' device.  ``t`` / ``z`` may be given; ``keys`` (one 64-bit key per row) with
        ``seed`` draws both from the keyed stream (``util.noise.loss_times`` and the noise of row key ``keys[b]``), so the
        value depends on (weights, keys, seed) only."""
        x0, y = batch
        return self._fm_loss(x0, y, t, z, keys, seed)[-1]

    def loss_rows(self, x0, y, t=None, z=None, *, keys=None, seed=0):
        """The [B] per-row values whose mean ``_step`` returns (float64, on the inputs' device)."""
        return self._fm_loss(x0, y, t, z, keys, seed)[:-1]

    def weights_frozen(self):
        """Context manager of the backbone: no in-place parameter updates inside (see NCSNpp.weights_frozen)."""
        return self.dnn.weights_frozen()

    def euler_sample_(self, x, y, timesteps, stepsizes):
        """Fused N-step Euler loop, in place on x (used by sampling.get_white_box_solver)."""
        return self.dnn.euler_sample(x, y, timesteps, stepsizes)

    def rk_sample_(self, x, y, timesteps, stepsizes, tableau):
        """Fused N-step fixed-step loop ('euler' | 'heun' | 'rk4'), in place on x: one library call, no host sync."""
        return self.dnn.rk_sample(x, y, timesteps, stepsizes, tableau)

    def rk_sample_multi_(self, xs, ys, timesteps, stepsizes, tableau, lanes=2, lane_of=None):
        """The same loop on several items at once, on ``lanes`` streams that share one set of weights: one library call,
        every item bit-identical to ``rk_sample_`` on it (used by sampling.get_white_box_solver_multi)."""
        return self.dnn.rk_sample_multi(xs, ys, timesteps, stepsizes, tableau, lanes=lanes, lane_of=lane_of)

    def rk45_sample_(self, x, y, t0, t_bound, rtol, atol, first_step=None, max_step=float("inf"), max_nfev=100000):
        """Adaptive RK45 (scipy's step control) in place on x: one library call.  Returns ``(x, nfev, status,
        accepted_times)`` (used by sampling.get_black_box_solver)."""
        return self.dnn.rk45_sample(x, y, t0, t_bound, rtol, atol, first_step, max_step, max_nfev)

    # ------------------------------------------------------------------ spectrogram helpers (model.py:190-203)
    def to_audio(self, spec, length=None):
        return self._istft(self._backward_transform(spec), length)

    def _forward_transform(self, spec):
        return self.data_module.spec_fwd(spec)

    def _backward_transform(self, spec):
        return self.data_module.spec_back(spec)

    def _stft(self, sig):
        return self.data_module.stft(sig)

    def _istft(self, spec, length=None):
        return self.data_module.istft(spec, length)
