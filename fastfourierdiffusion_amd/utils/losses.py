"""``fdiff.utils.losses`` mirror: the denoising score-matching loss, forward only.

``get_sde_loss_fn`` has the reference's signature (src/fdiff/utils/losses.py:12-17) and its evaluation behaviour
(losses.py:39-125): the perturbation, the score network and the weighted squared-error reduction are one stream-ordered
``ffd_sm_eval_batch`` call (csrc/ffd_loss.hip + the forward pass), and the batch mean is ``ffd_w2_summary``.  The only
torch arithmetic is the scheduler's ``marginal_coeffs`` on the (B,) timesteps.  ``train=True`` is refused: a closure
cannot own optimizer state, and the training surface is ``training.Trainer``.

``evaluate_loss`` runs a whole data set through the same entry point in batches without a host synchronisation.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from .. import _native as N
from ..schedulers.sde import SDE
from .dataclasses import DiffusableBatch

_MASK64 = (1 << 64) - 1
_DRAW_STRIDE = 0x9E3779B97F4A7C15  # Philox key of draw k = seed + k * this (mod 2^64)


def _eval_batch(model, X: torch.Tensor, timesteps: torch.Tensor, z: Optional[torch.Tensor], seed: int,
                sample_offset: int, likelihood_weighting: bool, reduce_mean: bool, out: torch.Tensor,
                scheduler: Optional[SDE] = None, labels=None) -> None:
    """Per-sample losses of X (B, L, C) at ``timesteps`` (B,) into ``out`` (B doubles, device); enqueue only.
    ``labels`` (a class-conditional model: (B,) integers, one int or None = null): the conditional branch, no dropout;
    their validation reads them on the host once."""
    if getattr(model, "n_classes", None) is not None:
        from ..models.score_models import class_labels

        with model.class_state(class_labels(labels, X.shape[0], model.n_classes, X.device)):
            _eval_batch_native(model, X, timesteps, z, seed, sample_offset, likelihood_weighting, reduce_mean, out, scheduler)
        return
    assert labels is None, f"{type(model).__name__} has no classes: labels must be None"
    _eval_batch_native(model, X, timesteps, z, seed, sample_offset, likelihood_weighting, reduce_mean, out, scheduler)


def _eval_batch_native(model, X, timesteps, z, seed, sample_offset, likelihood_weighting, reduce_mean, out, scheduler) -> None:
    ctx = model._ctx()
    scheduler = model.noise_scheduler if scheduler is None else scheduler
    mean_coeff, sigma = scheduler.marginal_coeffs(timesteps)
    mean_coeff, sigma = mean_coeff.contiguous(), sigma.contiguous()
    N.check(ctx.lib.ffd_sm_eval_batch(ctx.handle, X.data_ptr(), timesteps.data_ptr(), mean_coeff.data_ptr(),
                                      sigma.data_ptr(), z.data_ptr() if z is not None else None, seed & _MASK64,
                                      sample_offset, int(bool(likelihood_weighting)), int(bool(reduce_mean)),
                                      out.data_ptr(), X.shape[0], N.current_stream_ptr(X.device)),
            ctx.handle, "ffd_sm_eval_batch")


def _batch_mean(per_sample: torch.Tensor) -> torch.Tensor:
    """mean of a device vector of doubles (losses.py:124) as a 0-dim device tensor; no host synchronisation."""
    mm = torch.empty(2, device=per_sample.device, dtype=torch.float64)
    N.check(N.lib().ffd_w2_summary(per_sample.data_ptr(), per_sample.numel(), mm.data_ptr(),
                                   N.current_stream_ptr(per_sample.device)), None, "ffd_w2_summary")
    return mm[0]


def _draw_times(out: torch.Tensor, scheduler: SDE, seed: int, sample_offset: int) -> torch.Tensor:
    """losses.py:60-63 into ``out`` (n,) float32 on the device, by global sample index."""
    N.check(N.lib().ffd_sm_draw_times(out.data_ptr(), out.numel(), float(scheduler.eps), float(scheduler.T),
                                      seed & _MASK64, sample_offset, N.current_stream_ptr(out.device)),
            None, "ffd_sm_draw_times")
    return out


def get_sde_loss_fn(scheduler: SDE, train: bool, reduce_mean: bool = True, likelihood_weighting: bool = False, *,
                    rng: str = "torch", seed: int = 0,
                    sample_offset: int = 0) -> Callable[[torch.nn.Module, DiffusableBatch], torch.Tensor]:
    """losses.py:12-127.  ``rng`` (extension): ``"torch"`` draws the times (when ``batch.timesteps is None``) and z with
    ``torch.rand`` / ``torch.randn_like`` on the device, where the reference draws them; ``"philox"`` draws both inside
    the kernels from (``seed``, ``sample_offset`` + position in the batch), and no z tensor exists."""
    if train:
        raise NotImplementedError(
            "get_sde_loss_fn(train=True): a training loss closure is out of scope -- it could not own the optimizer "
            "state; train with fastfourierdiffusion_amd.training.Trainer, use train=False for the "
            "evaluation loss")
    if rng not in ("torch", "philox"):
        raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")

    def loss_fn(model: torch.nn.Module, batch: DiffusableBatch) -> torch.Tensor:
        model.eval()
        X = N.require_gpu_tensor(batch.X, "batch.X")
        assert X.dim() == 3 and X.size()[1:] == (model.max_len, model.n_channels), \
            f"X has wrong shape, should be {(X.size(0), model.max_len, model.n_channels)}, but is {X.size()}"
        B = X.shape[0]
        timesteps = batch.timesteps
        if timesteps is None:  # losses.py:59-63
            if rng == "torch":
                timesteps = torch.rand(B, device=X.device) * (scheduler.T - scheduler.eps) + scheduler.eps
            else:
                timesteps = _draw_times(torch.empty(B, device=X.device), scheduler, seed, sample_offset)
        assert timesteps.size(0) == B
        timesteps = timesteps.to(device=X.device, dtype=torch.float32).contiguous()
        z = torch.randn_like(X) if rng == "torch" else None  # losses.py:66
        per_sample = torch.empty(B, device=X.device, dtype=torch.float64)
        _eval_batch(model, X, timesteps, z, seed, sample_offset, likelihood_weighting, reduce_mean, per_sample,
                    scheduler, labels=batch.y if getattr(model, "n_classes", None) is not None else None)
        return _batch_mean(per_sample).to(torch.float32)

    return loss_fn


def evaluate_loss(model, X: torch.Tensor, batch_size: int, seed: int = 0, n_draws: int = 1, sample_offset: int = 0,
                  _return_noisy: bool = False, labels=None) -> dict:
    """The evaluation loss of ``model`` over a data set X (N, L, C) on the device, ``n_draws`` (time, noise) draws per
    sample, with the model's own scheduler and ``likelihood_weighting``.

    Times and noise come from the on-device Philox streams, keyed by (``seed``, draw) and counted by the global sample
    index ``sample_offset + i``: they do not depend on ``batch_size`` or on how X is cut into calls.  ``labels`` (N,)
    (a ``ClassConditionalScoreModule`` only; None: the null class) are sliced per batch.  Every batch is
    enqueued on the current stream; nothing is synchronised.  Returns device tensors: ``loss`` (0-dim float64, the mean
    of ``per_sample``), ``per_sample`` (n_draws, N) float64, ``timesteps`` (n_draws, N) float32.  ``_return_noisy``
    (tests) adds ``noisy`` (n_draws, N, L, C): the perturbed inputs, recomputed by ``ffd_sm_perturb``."""
    X = N.require_gpu_tensor(X, "X")
    assert X.dim() == 3 and X.size()[1:] == (model.max_len, model.n_channels), X.size()
    assert batch_size >= 1 and n_draws >= 1
    model.eval()
    sch = model.noise_scheduler
    n = X.shape[0]
    if getattr(model, "n_classes", None) is not None:
        from ..models.score_models import class_labels

        labels = class_labels(labels, n, model.n_classes, X.device)
    else:
        assert labels is None, f"{type(model).__name__} has no classes: labels must be None"
    per_sample = torch.empty((n_draws, n), device=X.device, dtype=torch.float64)
    times = torch.empty((n_draws, n), device=X.device, dtype=torch.float32)
    noisy = torch.empty((n_draws,) + tuple(X.shape), device=X.device, dtype=torch.float32) if _return_noisy else None
    for k in range(n_draws):
        key = (seed + k * _DRAW_STRIDE) & _MASK64
        _draw_times(times[k], sch, key, sample_offset)
        for i0 in range(0, n, batch_size):
            i1 = min(i0 + batch_size, n)
            _eval_batch(model, X[i0:i1], times[k, i0:i1], None, key, sample_offset + i0, model.likelihood_weighting,
                        True, per_sample[k, i0:i1], labels=labels[i0:i1] if labels is not None else None)
        if noisy is not None:
            mean_coeff, sigma = (c.contiguous() for c in sch.marginal_coeffs(times[k]))
            L, Cn = X.shape[1:]
            if sch.G is None:
                sch.set_noise_scaling(L)
            N.check(N.lib().ffd_sm_perturb(X.data_ptr(), noisy[k].data_ptr(), mean_coeff.data_ptr(), sigma.data_ptr(),
                                           sch._G_on(X.device).data_ptr(), None, key, sample_offset, n, L, Cn,
                                           N.current_stream_ptr(X.device)), None, "ffd_sm_perturb")
    out = {"loss": _batch_mean(per_sample.view(-1)), "per_sample": per_sample, "timesteps": times}
    if noisy is not None:
        out["noisy"] = noisy
    return out
