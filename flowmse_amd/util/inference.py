"""Validation hook: enhance a few validation files with the fast sampler and score them.

Same call as the reference's ``evaluate_model(model, num_eval_files, inference_N)`` (flowmse/util/inference.py:15-71,
called from ``VFModel.validation_step``, model.py:139-150): files are picked uniformly over
``model.data_module.valid_set.{clean,noisy}_files``, each is normalised by its peak, transformed, padded, run through
the white-box Euler solver (one fused ``flowse_euler_sample`` call when ``model`` is the HIP-backed VFModel) and
resynthesised; returns the means ``(pesq, si_sdr, estoi)``.  PESQ / ESTOI need the optional ``pesq`` / ``pystoi``
packages and are NaN without them (the reference imports them unconditionally).
"""
import torch

from flowmse_amd.util.other import read_wav, si_sdr

sr = 16000
N = 5


def evaluate_model(model, num_eval_files, inference_N=N, odesolver="euler", VF_fn=None):
    from flowmse_amd.evaluate import enhance_waveform       # late: evaluate.py imports the sampling package
    try:
        from pesq import pesq
    except ImportError:
        pesq = None
    try:
        from pystoi import stoi
    except ImportError:
        stoi = None
    T_rev, t_eps = model.T_rev, model.t_eps
    model.ode.T_rev = T_rev
    valid = model.data_module.valid_set
    picks = torch.linspace(0, len(valid.clean_files) - 1, num_eval_files, dtype=torch.int).tolist()
    device = torch.device("cpu") if VF_fn is not None else next(model.parameters()).device
    tot_pesq = tot_sdr = tot_estoi = 0.0
    for i in picks:
        x, _ = read_wav(valid.clean_files[i])
        y, _ = read_wav(valid.noisy_files[i])
        x_hat = enhance_waveform(model, y.to(device), N=inference_N, T_rev=T_rev, t_eps=t_eps, odesolver=odesolver,
                                 VF_fn=VF_fn, device=device)
        x = x.squeeze().numpy()
        tot_sdr += si_sdr(x, x_hat)
        try:
            tot_pesq += pesq(sr, x, x_hat, "wb") if pesq else float("nan")
        except Exception:                                   # pesq raises on utterances without speech
            tot_pesq += float("nan")
        tot_estoi += stoi(x, x_hat, sr, extended=True) if stoi else float("nan")
    return tot_pesq / num_eval_files, tot_sdr / num_eval_files, tot_estoi / num_eval_files


# ------------------------------------------------------------------------------------------- valid_loss (model.py:151-153)
def validation_item(model, x, y, num_frames=256):
    """The reference's validation item of one file (flowmse/data_module.py:46-80 with ``shuffle_spec=False``,
    ``normalize="noisy"``): x, y float tensors [1, samples] (clean, noisy) -> ``(X, Y)`` complex64 [1, F, num_frames].
    Centre crop, or symmetric zero pad, to ``(num_frames - 1) * hop`` samples; both signals divided by the noisy crop's
    peak; ``_forward_transform(_stft(.))``."""
    target_len = (num_frames - 1) * model.data_module.hop_length
    current_len = x.size(-1)
    pad = max(target_len - current_len, 0)
    if pad == 0:
        start = int((current_len - target_len) / 2)
        x, y = x[..., start:start + target_len], y[..., start:start + target_len]
    else:
        x = torch.nn.functional.pad(x, (pad // 2, pad // 2 + (pad % 2)), mode="constant")
        y = torch.nn.functional.pad(y, (pad // 2, pad // 2 + (pad % 2)), mode="constant")
    normfac = y.abs().max()
    return model._forward_transform(model._stft(x / normfac)), model._forward_transform(model._stft(y / normfac))


def keyed_valid_losses(model, items, names, seed=0, draws=1, batch=8):
    """``valid_loss`` per file: for item i = ``(X, Y)`` of file ``names[i]`` the mean over ``draws`` keyed draws of the
    flow-matching loss (float64 numpy [len(items)]).  Draw k of a file takes its time from ``loss_times`` and its noise from
    row key ``draw_key(utterance_key(name), k)``; the (file, draw) rows are scored ``batch`` at a time, one
    ``flowse_fm_loss`` call each, and read back once."""
    import numpy as np

    from flowmse_amd.util.noise import draw_key, loss_seed, loss_times, utterance_key
    ukeys = [utterance_key(n) for n in names]
    times = loss_times(ukeys, loss_seed(seed), model.T_rev, model.t_eps, draws)
    rows = [(i, k) for i in range(len(items)) for k in range(draws)]
    parts = []
    for r0 in range(0, len(rows), batch):
        part = rows[r0:r0 + batch]
        x0 = torch.stack([items[i][0] for i, _ in part])
        y = torch.stack([items[i][1] for i, _ in part])
        t = torch.from_numpy(np.asarray([times[i, k] for i, k in part], dtype=np.float32))
        parts.append(model.loss_rows(x0, y, t, keys=[draw_key(ukeys[i], k) for i, k in part], seed=seed))
    vals = torch.cat(parts).cpu().numpy() if parts else np.zeros(0)
    return vals.reshape(len(items), draws).mean(axis=1)


def validation_loss(model, num_files=None, batch=8, seed=0, draws=1):
    """The ``valid_loss`` of the reference's ``validation_step`` (model.py:151-153) over ``model.data_module.valid_set``:
    the mean flow-matching loss of the files' validation items (all files, or ``num_files`` picked as ``evaluate_model``
    picks them), with keyed draws so that the number depends on (weights, file names, seed, draws) only."""
    valid = model.data_module.valid_set
    n = len(valid.clean_files)
    picks = list(range(n)) if num_files is None else torch.linspace(0, n - 1, num_files, dtype=torch.int).tolist()
    device = next(model.parameters()).device
    items = [validation_item(model, read_wav(valid.clean_files[i])[0].to(device), read_wav(valid.noisy_files[i])[0].to(device))
             for i in picks]
    vals = keyed_valid_losses(model, items, [valid.noisy_files[i] for i in picks], seed=seed, draws=draws, batch=batch)
    return float(vals.mean())
