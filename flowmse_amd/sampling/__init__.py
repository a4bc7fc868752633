"""Samplers (reference: flowmse/sampling/__init__.py:27-62).

``get_white_box_solver`` keeps the reference signature and semantics: prior sample, ``torch.linspace(T_rev,
t_eps, N)`` time grid, step sizes ``t_i - t_{i+1}`` with the LAST step equal to ``t_{N-1}`` (so the trajectory
ends at t = 0), N solver updates, returns ``(x, N)``.

When ``VF_fn`` is a HIP-backed :class:`flowmse_amd.model.VFModel` and the solver is one the library implements
(``'euler'``, the reference's; ``'heun'`` / ``'rk4'``, the fixed-step plugins) the whole loop runs as one C-ABI call
(``flowse_rk_sample``): N x stages x (NCSN++ forward + solver update fused into the head kernel) enqueued on the
current stream with no host synchronisation.  Any other callable ``VF_fn`` / registered solver goes through the
generic plugin loop, exactly like the reference; that loop keeps its time grid on the host, so it never reads a
device tensor back either.
"""
import contextlib
import math
import numbers
import os
import warnings

import torch

from .odesolvers import ODEsolver, ODEsolverRegistry

__all__ = ["ODEsolverRegistry", "ODEsolver", "get_white_box_solver", "get_white_box_solver_multi", "get_black_box_solver",
           "fused_rk45", "time_grid"]


def time_grid(T_rev, t_eps, N, device="cpu"):
    """(timesteps, stepsizes) exactly as the reference loop builds them (sampling/__init__.py:45-53)."""
    timesteps = torch.linspace(T_rev, t_eps, N, device=device)
    steps = []
    for i in range(N):
        steps.append(timesteps[i] - timesteps[i + 1] if i != N - 1 else timesteps[-1])
    return timesteps, torch.stack(steps)


def _frozen(VF_fn):
    """``VF_fn.weights_frozen()`` when the field is a HIP-backed model (its per-call weight-version scan then runs once
    per sampler loop instead of once per network evaluation), else a no-op context."""
    f = getattr(VF_fn, "weights_frozen", None)
    return f() if callable(f) else contextlib.nullcontext()


def _fused_tableau(odesolver_cls):
    """Name of the library's fused implementation of this solver class, or None (plugin loop).

    Only a class that opts in ITSELF qualifies: ``fused_tableau`` must be set in the class's own ``__dict__`` and its
    ``update_fn`` must be the one defined next to it.  A plugin that subclasses a built-in solver
    (``class My(EulerODEsolver)``) and overrides ``update_fn`` inherits the attribute but not the claim -- it goes
    through the generic loop, where its ``update_fn`` is what runs."""
    name = odesolver_cls.__dict__.get("fused_tableau")
    if name is None or "update_fn" not in odesolver_cls.__dict__:
        return None
    return name


def _prior(ode, P, z, noise_keys, noise_seed, noise_frame0=None):
    """The prior sample of one solver call: explicit ``z``, the keyed stream (``noise_keys``: one 64-bit key per row of
    ``P``; ``noise_frame0``: the absolute frame each row starts at), or the process-wide generator -- each through the call
    ``prior_sampling`` had before keys (or offsets) existed."""
    if noise_frame0 is not None:
        if noise_keys is None:
            raise ValueError("noise_frame0 addresses the keyed noise stream; pass noise_keys")
        return ode.prior_sampling(P.shape, P, z, keys=noise_keys, seed=noise_seed, frame0=noise_frame0)[0]
    if noise_keys is not None:
        return ode.prior_sampling(P.shape, P, z, keys=noise_keys, seed=noise_seed)[0]
    return ode.prior_sampling(P.shape, P, z)[0] if z is not None else ode.prior_sampling(P.shape, P)[0]


def get_white_box_solver(odesolver_name, ode, VF_fn, Y, Y_prior=None, T_rev=1.0, t_eps=0.03, N=30, z=None,
                         noise_keys=None, noise_seed=0, noise_frame0=None, **kwargs):
    """Returns ``ode_solver() -> (x_result, N)``.  Extra keyword ``z``: explicit prior noise (reproducibility);
    ``noise_keys`` / ``noise_seed``: the keyed noise stream instead (``FLOWMATCHING.prior_sampling``), one key per row;
    ``noise_frame0``: with keys, the even absolute frame each row starts at in its utterance (chunks of a recording)."""
    odesolver_cls = ODEsolverRegistry.get_by_name(odesolver_name)
    odesolver = odesolver_cls(ode, VF_fn)
    fused = _fused_tableau(odesolver_cls) is not None and hasattr(VF_fn, "rk_sample_") and Y.is_cuda

    def ode_solver(Y_prior=Y_prior):
        with torch.no_grad():
            if Y_prior is None:
                Y_prior = Y
            xt = _prior(ode, Y_prior, z, noise_keys, noise_seed, noise_frame0).to(Y_prior.device)
            # host copy of the grid: the values equal torch.linspace(..., device=Y.device) of the reference
            timesteps, stepsizes = time_grid(T_rev, t_eps, N)
            if fused:
                xt = VF_fn.rk_sample_(xt.contiguous(), Y.contiguous(), timesteps.tolist(), stepsizes.tolist(),
                                      _fused_tableau(odesolver_cls))
                return xt, N
            try:
                with _frozen(VF_fn):
                    for i in range(N):
                        # t and the step size stay host values (0-d CPU tensors): `ones(B) * t` is a fill kernel with
                        # a scalar argument, and a solver may inspect the step ("does it land on t = 0?") with no
                        # readback
                        t = timesteps[i]
                        stepsize = stepsizes[i]
                        vec_t = torch.ones(Y.shape[0], device=Y.device) * float(t)
                        odesolver.step_start_time = float(t)
                        xt = odesolver.update_fn(xt, vec_t, Y, stepsize)
            finally:
                odesolver.step_start_time = None
            return xt, N

    return ode_solver


def get_white_box_solver_multi(odesolver_name, ode, VF_fn, Ys, Y_priors=None, T_rev=1.0, t_eps=0.03, N=30, zs=None,
                               lanes=2, noise_keys=None, noise_seed=0, **kwargs):
    """``get_white_box_solver`` for a list of independent items ``Ys[i]`` ([B_i,1,F,T_i]; batch sizes and lengths may
    differ): returns ``ode_solver() -> ([x_i], N)`` with every ``x_i`` equal, bit for bit, to what the single solver
    returns for item i.

    When the single solver would be fused for EVERY item (a solver the library implements on a HIP-backed field that
    offers ``rk_sample_multi_``, device tensors) the items run as ONE library call (``flowse_rk_sample_multi``) on
    ``lanes`` streams over shared weights, dealt to the lanes by ``flowmse_amd.parallel.plan_lanes``; the priors are drawn
    first, in list order, so the random stream is consumed as by the single solvers called in that order.  Otherwise the
    single solver runs per item, in order: same results, no concurrency.  ``noise_keys``: one key list per item (the
    keyed noise stream under ``noise_seed``, see ``get_white_box_solver``)."""
    odesolver_cls = ODEsolverRegistry.get_by_name(odesolver_name)
    n = len(Ys)
    Y_priors = list(Ys) if Y_priors is None else [Y if P is None else P for Y, P in zip(Ys, Y_priors)]
    zs = [None] * n if zs is None else list(zs)
    keys = [None] * n if noise_keys is None else list(noise_keys)
    if len(Y_priors) != n or len(zs) != n or len(keys) != n:
        raise ValueError("Ys, Y_priors, zs and noise_keys must have the same length")
    fused = _fused_tableau(odesolver_cls) is not None and hasattr(VF_fn, "rk_sample_") \
        and hasattr(VF_fn, "rk_sample_multi_") and n > 0 and all(Y.is_cuda for Y in Ys)

    def ode_solver():
        if not fused:
            return [get_white_box_solver(odesolver_name, ode, VF_fn, Y, Y_prior=P, T_rev=T_rev, t_eps=t_eps, N=N, z=z,
                                         noise_keys=k, noise_seed=noise_seed, **kwargs)()[0]
                    for Y, P, z, k in zip(Ys, Y_priors, zs, keys)], N
        from flowmse_amd.parallel import batch_cost, plan_lanes
        with torch.no_grad():
            xts = []
            for P, z, k in zip(Y_priors, zs, keys):
                xts.append(_prior(ode, P, z, k, noise_seed).to(P.device).contiguous())
            timesteps, stepsizes = time_grid(T_rev, t_eps, N)
            k = max(1, min(int(lanes), n))
            lane_of, _ = plan_lanes([batch_cost(Y.shape[-1], Y.shape[0]) for Y in Ys], k)
            VF_fn.rk_sample_multi_(xts, [Y.contiguous() for Y in Ys], timesteps.tolist(), stepsizes.tolist(),
                                   _fused_tableau(odesolver_cls), lanes=k, lane_of=lane_of)
            return xts, N

    return ode_solver


def to_flattened_numpy(x):
    """Flatten a torch tensor and convert it to numpy (sampling/__init__.py:17-19)."""
    return x.detach().cpu().numpy().reshape((-1,))


def from_flattened_numpy(x, shape):
    """Form a torch tensor with the given shape from a flattened numpy array (sampling/__init__.py:22-24)."""
    return torch.from_numpy(x.reshape(shape))


_RK45_FUSED_KWARGS = frozenset(("first_step", "max_step"))


def fused_rk45(method, VF_fn, y, rtol, atol, solver_kwargs):
    """True when ``get_black_box_solver`` runs the solve as one library call (``VF_fn.rk45_sample_``) instead of scipy:
    RK45, a HIP-backed field, a device state, scalar tolerances and no ``solve_ivp`` option beyond ``first_step`` /
    ``max_step``.  ``FLOWSE_RK45_HOST=1`` (read per call) forces scipy."""
    return (os.environ.get("FLOWSE_RK45_HOST", "0") != "1" and isinstance(method, str) and method == "RK45"
            and callable(getattr(VF_fn, "rk45_sample_", None)) and bool(getattr(y, "is_cuda", False))
            and _real_scalar(rtol) and _real_scalar(atol) and set(solver_kwargs) <= _RK45_FUSED_KWARGS)


def _real_scalar(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _rk45_fused(VF_fn, x, y, T_rev, t_eps, rtol, atol, first_step=None, max_step=math.inf):
    """The device solve with scipy's argument checks (validate_tol / validate_first_step / validate_max_step)."""
    from scipy.integrate._ivp.common import EPS
    if rtol < 100 * EPS:
        warnings.warn("At least one element of `rtol` is too small. "
                      f"Setting `rtol = np.maximum(rtol, {100 * EPS})`.", stacklevel=3)
        rtol = max(rtol, 100 * EPS)
    if atol < 0:
        raise ValueError("`atol` must be positive.")
    if max_step <= 0:
        raise ValueError("`max_step` must be positive.")
    if first_step is not None:
        if first_step <= 0:
            raise ValueError("`first_step` must be positive.")
        if first_step > abs(float(t_eps) - float(T_rev)):
            raise ValueError("`first_step` exceeds bounds.")
    x, nfev, status, _ = VF_fn.rk45_sample_(x, y, float(T_rev), float(t_eps), float(rtol), float(atol),
                                            first_step=first_step, max_step=float(max_step))
    if status == -2:
        raise RuntimeError(f"flowse_rk45_sample: stopped after {nfev} network evaluations (max_nfev)")
    return x, nfev


def get_black_box_solver(ode, VF_fn, y, rtol=1e-5, atol=1e-5, T_rev=1.0, t_eps=0.03, N=30, method="RK45",
                         device="cuda", z=None, noise_keys=None, noise_seed=0, **kwargs):
    """Adaptive black-box sampler (reference: flowmse/sampling/__init__.py:64-114): scipy ``solve_ivp`` on the
    flattened complex state from T_rev down to t_eps (NOT to 0), each right-hand side evaluation being one call
    of ``VF_fn`` (host <-> device round trip per evaluation, as in the reference).  Returns ``(x, nfe)``.
    ``evaluate.py`` imports but never calls it; provided for API completeness.

    When :func:`fused_rk45` holds (RK45 on a HIP-backed ``VFModel``) the solve is one C-ABI call
    (``flowse_rk45_sample``) that keeps the state on the device and takes the steps scipy takes -- same nfev, same
    accepted times, same end point up to the summation order of the error norm; the only host traffic is one 8-byte
    error norm per attempted step.  Everything else (other methods, array tolerances, ``t_eval``, ``dense_output``,
    ``events``, any other callable field) runs scipy exactly as before.  ``noise_keys`` / ``noise_seed``: the keyed
    noise stream for the prior (see ``get_white_box_solver``)."""
    from scipy import integrate

    def ode_solver(**solver_kwargs):
        with torch.no_grad():
            x = _prior(ode, y, z, noise_keys, noise_seed).to(device)
            if fused_rk45(method, VF_fn, y, rtol, atol, solver_kwargs):
                xd = x.to(device=y.device, dtype=torch.complex64).contiguous()
                xd, nfev = _rk45_fused(VF_fn, xd, y.contiguous(), T_rev, t_eps, rtol, atol, **solver_kwargs)
                return xd.to(device), nfev

            def ode_func(t, xf):
                xt = from_flattened_numpy(xf, y.shape).to(device).type(torch.complex64)
                vec_t = torch.ones(y.shape[0], device=xt.device) * t
                return to_flattened_numpy(VF_fn(xt, vec_t, y))

            with _frozen(VF_fn):
                solution = integrate.solve_ivp(ode_func, (T_rev, t_eps), to_flattened_numpy(x), rtol=rtol, atol=atol,
                                               method=method, **solver_kwargs)
            x = torch.tensor(solution.y[:, -1]).reshape(y.shape).to(device).type(torch.complex64)
            return x, solution.nfev

    return ode_solver
