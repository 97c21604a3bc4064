"""Training on the device: the reference's recipe (src/fdiff/models/score_models.py:290-324 and
cmd/conf/trainer/default.yaml) without autograd -- denoising score-matching loss, AdamW (lr from the cosine schedule
with ``num_training_steps // 10`` warm-up steps, betas 0.9 / 0.999, eps 1e-8, weight decay 1e-2) and global-norm
gradient clipping at 1.0.  libffd's ``ffd_train_*`` entry points (csrc/ffd_train.hip) run the forward that keeps its
activations, the backward pass, the gradient norm and the update directly on the torch parameters' storage; torch only
holds memory.

What trains: ``ScoreModule`` (the transformer) and ``MLPScoreModule``.  ``LSTMScoreModule`` would need backpropagation
through time and ``MixtureScoreModule`` has nothing to train: both raise ``NotImplementedError``.  The transformer's
positional table is an ``nn.Embedding(max_norm)``: every forward of a training step first renormalises the parameter's
rows in place (as torch's lookup does, without gradient), and the gradient is taken with respect to the renormalised rows.
Dropout (p = 0.1 in the reference's blocks) is not implemented: ``dropout`` accepts only
0.0, so a model trained here is trained without it.  A model with the E2-CRF cache enabled is refused; FreSca is a property
of ``DiffusionSampler`` (it rescales the score inside the sampling loop), not of a model, and cannot reach training.

Classes.  A ``ClassConditionalScoreModule`` trains with labels (``step`` / ``loss_and_grad`` / ``fit(..., labels=)``,
indexed like X): each is dropped to the null class with probability ``p_uncond`` by an on-device draw keyed like the
times (classifier-free guidance's training recipe), and the table ``class_embedding.weight`` is one more tensor under
the same norm, clip, AdamW and decay.  Labels with a model without classes are an ``AssertionError``.

Draws.  Step k takes its times and noise from the Philox key ``seed + k * _DRAW_STRIDE`` -- the keying of
``evaluate_loss`` -- counted by the data-set row: with ``index`` a row's draw does not depend on the batch it lands in.
"""
from __future__ import annotations

import ctypes as C
import inspect
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .utils.losses import _DRAW_STRIDE, _MASK64, _batch_mean, _draw_times, evaluate_loss


def lr_at(step: int, lr_max: float, num_warmup_steps: int, num_training_steps: int) -> float:
    """The learning rate of optimizer step ``step`` (0-based): ``LambdaLR`` over
    ``transformers.get_cosine_schedule_with_warmup`` (score_models.py:318-324)."""
    return float(N.lib().ffd_host_lr_schedule(float(lr_max), int(step), int(num_warmup_steps), int(num_training_steps)))


def _refuse(model, dropout: float) -> None:
    """Everything that cannot train, refused before any native call."""
    kind = getattr(model, "_kind", None)
    if dropout != 0.0:
        raise NotImplementedError(f"dropout={dropout}: training runs without dropout only (the reference trains with "
                                  "p = 0.1); pass dropout=0.0")
    if kind == N.FFD_MODEL_LSTM:
        raise NotImplementedError("LSTMScoreModule cannot be trained here: there is no backpropagation through time")
    if kind == N.FFD_MODEL_MIXTURE:
        raise NotImplementedError("MixtureScoreModule has no trainable network")
    if kind not in (N.FFD_MODEL_MLP, N.FFD_MODEL_TRANSFORMER):
        raise NotImplementedError(f"{type(model).__name__} cannot be trained")
    if getattr(model, "use_cache", False):
        raise NotImplementedError("training with the E2-CRF cache enabled is refused: call disable_caching() first")


class Trainer:
    """Optimizer state and the native training object of one model.

    ``step`` / ``loss_and_grad`` enqueue on the current stream and return a 0-dim device tensor; nothing synchronises.
    The gradients live in the parameters' ``.grad`` (unclipped; the clip coefficient is applied inside the update),
    the Adam moments in ``exp_avg`` / ``exp_avg_sq`` by parameter name."""

    def __init__(self, model, seed: int = 0, grad_clip: float = 1.0, weight_decay: float = 1e-2,
                 betas=(0.9, 0.999), eps: float = 1e-8, dropout: float = 0.0, p_uncond: float = 0.1) -> None:
        _refuse(model, dropout)
        assert 0.0 <= float(p_uncond) <= 1.0, f"p_uncond must lie in [0, 1], got {p_uncond!r}"
        self.p_uncond = float(p_uncond)  # label dropout of a class-conditional model (classifier-free guidance)
        self.n_classes = getattr(model, "n_classes", None)
        self._labels = None  # the int32 device labels libffd reads during the native call in flight
        dev = model.device
        if dev.type != "cuda":
            raise N.FFDError(f"model parameters live on {dev}: training runs only on an MI355X (gfx950) device; "
                             "call .cuda() (there is no CPU fallback)")
        self.model = model
        self.seed = int(seed)
        self.grad_clip = float(grad_clip)
        self.weight_decay = float(weight_decay)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.global_step = 0
        self.last_per_sample: Optional[torch.Tensor] = None  # (B,) float64: the per-sample losses of the last batch
        self.lib = N.lib()
        self.exp_avg, self.exp_avg_sq = {}, {}
        for name, p in model.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise AssertionError(f"{name} must be contiguous float32")
            if p.requires_grad:
                self.exp_avg[name] = torch.zeros_like(p)
                self.exp_avg_sq[name] = torch.zeros_like(p)
        self.handle = C.c_void_p()
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        rc = self.lib.ffd_train_create(C.byref(self.handle), C.byref(model._desc()), float(dropout), idx)
        self._check(rc, "ffd_train_create")
        if self.n_classes is not None:
            self._check(self.lib.ffd_train_classes(self.handle, int(self.n_classes)), "ffd_train_classes")
        self._bound = None
        self._bind()

    # ------------------------------------------------------------------
    def _check(self, rc: int, what: str) -> None:
        if rc == 0:
            return
        raw = self.lib.ffd_train_last_error(self.handle) if self.handle else b""
        exc = {-1: AssertionError, -2: NotImplementedError}.get(rc, N.FFDError)
        raise exc(f"libffd {what} failed (status {rc}): {raw.decode() if raw else ''}")

    def _bind(self) -> None:
        """(Re)bind every parameter whose storage or gradient moved since the last call."""
        ptrs = []
        for name, p in self.model.named_parameters():
            if p.requires_grad and p.grad is None:
                p.grad = torch.zeros_like(p)
            ptrs.append((name, p.data_ptr(), p.grad.data_ptr() if p.requires_grad else 0))
        if ptrs == self._bound:
            return
        for name, p in self.model.named_parameters():
            if p.requires_grad:
                args = (p.data_ptr(), p.grad.data_ptr(), self.exp_avg[name].data_ptr(), self.exp_avg_sq[name].data_ptr())
            else:
                args = (p.data_ptr(), None, None, None)
            self._check(self.lib.ffd_train_bind(self.handle, name.encode(), *args, p.numel()), f"ffd_train_bind({name})")
        self._bound = ptrs

    def work_bytes(self, batch_size: int) -> int:
        """Bytes of the native workspace at this batch size."""
        return int(self.lib.ffd_train_work_bytes(C.byref(self.model._desc()), int(batch_size)))

    def _key(self, k: int) -> int:
        return (self.seed + k * _DRAW_STRIDE) & _MASK64

    def lr(self, step: Optional[int] = None) -> float:
        m = self.model
        return lr_at(self.global_step if step is None else step, m.lr_max, m.num_warmup_steps, m.num_training_steps)

    def _cfg(self, lr: Optional[float] = None) -> N.AdamWCfg:
        return N.AdamWCfg(self.lr() if lr is None else float(lr), self.betas[0], self.betas[1], self.eps,
                          self.weight_decay, self.grad_clip, self.global_step + 1)

    def _batch(self, X, sample_offset, index, timesteps, z, trusted_index=False):
        """Validated native arguments of one batch: (X, index, timesteps, mean_coeff, sigma, z, B)."""
        m = self.model
        X = N.require_gpu_tensor(X, "X")
        assert X.dim() == 3 and X.size()[1:] == (m.max_len, m.n_channels), \
            f"X has wrong shape, should be (*, {m.max_len}, {m.n_channels}), but is {tuple(X.size())}"
        rows = X.shape[0]
        if index is not None:
            assert index.dtype == torch.int64 and index.dim() == 1 and index.device == X.device and index.numel() >= 1
            index = index.contiguous()
            if not trusted_index:  # a caller's index is checked (one host synchronisation); fit's permutation is not
                assert bool(((index >= 0) & (index < rows)).all()), "index must lie within the rows of X"
        B = rows if index is None else index.numel()
        assert B >= 1
        if timesteps is None:  # losses.py:59-63, by global row: B draws, whatever the size of the data set
            timesteps = torch.empty(B, device=X.device)
            key = self._key(self.global_step)
            if index is None:
                _draw_times(timesteps, m.noise_scheduler, key, int(sample_offset))
            else:
                N.check(self.lib.ffd_sm_draw_times_at(timesteps.data_ptr(), index.data_ptr(), B, float(m.noise_scheduler.eps),
                                                      float(m.noise_scheduler.T), key, int(sample_offset),
                                                      N.current_stream_ptr(X.device)), None, "ffd_sm_draw_times_at")
        timesteps = timesteps.to(device=X.device, dtype=torch.float32).contiguous()
        assert timesteps.shape == (B,), "timesteps are per sample of the batch"
        mean_coeff, sigma = (c.contiguous() for c in m.noise_scheduler.marginal_coeffs(timesteps))
        if z is not None:
            z = N.require_gpu_tensor(z, "z")
            assert tuple(z.shape) == (B, m.max_len, m.n_channels), "z is (B, L, C) in batch order"
        return X, index, timesteps, mean_coeff, sigma, z, B

    def _set_labels(self, labels, X, trusted: bool = False) -> None:
        """Hand the labels of the coming native call to libffd: (rows of X,) integers indexed like X (by ``index`` where
        one is given), one int, or None (every sample null).  A model without classes takes None only.  ``trusted``:
        ``fit``'s labels, validated once and already int32 on the device."""
        if self.n_classes is None:
            assert labels is None, f"{type(self.model).__name__} has no classes: labels must be None"
            return
        from .models.score_models import class_labels

        y = labels if trusted else class_labels(labels, X.shape[0], self.n_classes, X.device)
        self._labels = y
        self._check(self.lib.ffd_train_labels(self.handle, y.data_ptr() if y is not None else None,
                                              y.numel() if y is not None else 0, self.p_uncond), "ffd_train_labels")

    def _native_args(self, X, index, timesteps, mean_coeff, sigma, z, sample_offset, per_sample, B):
        return (self.handle, X.data_ptr(), index.data_ptr() if index is not None else None, timesteps.data_ptr(),
                mean_coeff.data_ptr(), sigma.data_ptr(), z.data_ptr() if z is not None else None,
                self._key(self.global_step), int(sample_offset), int(bool(self.model.likelihood_weighting)),
                per_sample.data_ptr(), B)

    # ------------------------------------------------------------------
    def loss_and_grad(self, X: torch.Tensor, sample_offset: int = 0, index: Optional[torch.Tensor] = None,
                      timesteps: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None,
                      labels=None) -> torch.Tensor:
        """Fill every parameter's ``.grad`` with the gradient of the batch's loss and return the loss; no update.
        ``labels`` (a class-conditional model): indexed like X; each is dropped to the null class with probability
        ``p_uncond`` by the draw of its global row.

        ``index`` None: X (B, L, C) is the batch and sample b draws as global sample ``sample_offset + b``.  ``index``
        (B,) int64 on the device: X (N, L, C) is the data set, the batch is its rows ``index`` and row i draws as global
        sample ``sample_offset + i``.  ``timesteps`` (B,) and ``z`` (B, L, C), both in batch order, inject the draws."""
        self.model.train()
        self._bind()
        X, index, timesteps, mean_coeff, sigma, z, B = self._batch(X, sample_offset, index, timesteps, z)
        self._set_labels(labels, X)
        per_sample = torch.empty(B, device=X.device, dtype=torch.float64)
        args = self._native_args(X, index, timesteps, mean_coeff, sigma, z, sample_offset, per_sample, B)
        self._check(self.lib.ffd_train_loss_grad(*args, N.current_stream_ptr(X.device)), "ffd_train_loss_grad")
        self.last_per_sample = per_sample
        return _batch_mean(per_sample).to(torch.float32)

    def grad_sqnorm(self) -> torch.Tensor:
        """The squared global gradient norm as a 1-element float64 device tensor."""
        dev = self.model.device
        out = torch.empty(1, device=dev, dtype=torch.float64)
        self._check(self.lib.ffd_train_grad_sqnorm(self.handle, out.data_ptr(), N.current_stream_ptr(dev)),
                    "ffd_train_grad_sqnorm")
        return out

    def apply_update(self, sqnorm: Optional[torch.Tensor], lr: Optional[float] = None) -> None:
        """AdamW on every parameter from the gradients in place, at the schedule's rate (or ``lr``); advances the step
        count and invalidates the model's inference context."""
        self._bind()
        dev = self.model.device
        cfg = self._cfg(lr)
        self._check(self.lib.ffd_train_adamw(self.handle, sqnorm.data_ptr() if sqnorm is not None else None, C.byref(cfg),
                                             N.current_stream_ptr(dev)), "ffd_train_adamw")
        self._updated()

    def _updated(self) -> None:
        self.global_step += 1
        if self.model._native is not None:  # the next forward / sample uploads the trained weights
            self.model._native.weights_key = None

    def step(self, X: torch.Tensor, sample_offset: int = 0, index: Optional[torch.Tensor] = None,
             timesteps: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None,
             lr: Optional[float] = None, _trusted_index: bool = False, labels=None) -> torch.Tensor:
        """One training step (loss, gradients, norm, clipped AdamW update) in one native call; returns the loss of the
        batch before the update.  Arguments as ``loss_and_grad``.  Nothing synchronises, except that an ``index`` is
        checked against the rows of X on the host first."""
        self.model.train()
        self._bind()
        X, index, timesteps, mean_coeff, sigma, z, B = self._batch(X, sample_offset, index, timesteps, z, _trusted_index)
        self._set_labels(labels, X, _trusted_index)
        per_sample = torch.empty(B, device=X.device, dtype=torch.float64)
        args = self._native_args(X, index, timesteps, mean_coeff, sigma, z, sample_offset, per_sample, B)
        cfg = self._cfg(lr)
        self._check(self.lib.ffd_train_step(*args, C.byref(cfg), N.current_stream_ptr(X.device)), "ffd_train_step")
        self._updated()
        self.last_per_sample = per_sample
        return _batch_mean(per_sample).to(torch.float32)

    def epoch_order(self, n: int, epoch: int, shuffle: bool = True) -> np.ndarray:
        """The row order of an epoch: a host permutation from ``numpy.random.Generator`` seeded by (seed, epoch)."""
        if not shuffle:
            return np.arange(n, dtype=np.int64)
        return np.random.Generator(np.random.PCG64([self.seed, int(epoch)])).permutation(n).astype(np.int64)

    def fit(self, X: torch.Tensor, batch_size: int = 64, max_epochs: int = 1, X_val: Optional[torch.Tensor] = None,
            shuffle: bool = True, labels=None, labels_val=None) -> dict:
        """Train over the data set X (N, L, C), a device tensor already in the diffused domain.  Returns
        ``train_loss`` (steps,) on the device and, with ``X_val``, ``val_loss``: ``evaluate_loss`` after each epoch."""
        X = N.require_gpu_tensor(X, "X")
        assert batch_size >= 1 and max_epochs >= 1
        n = X.shape[0]
        if self.n_classes is not None:  # validated once (one host read), then handed over as they are every step
            from .models.score_models import class_labels

            labels = class_labels(labels, n, self.n_classes, X.device)
        else:
            assert labels is None and labels_val is None, f"{type(self.model).__name__} has no classes: labels must be None"
        first_epoch = self.global_step // max(1, -(-n // batch_size))
        history, val = [], []
        for epoch in range(first_epoch, first_epoch + max_epochs):
            order = torch.from_numpy(self.epoch_order(n, epoch, shuffle)).to(X.device)
            for i0 in range(0, n, batch_size):
                history.append(self.step(X, index=order[i0:i0 + batch_size], _trusted_index=True, labels=labels))
            if X_val is not None:
                val.append(evaluate_loss(self.model, X_val, batch_size, seed=self.seed, labels=labels_val)["loss"])
        out = {"train_loss": torch.stack(history)}
        if X_val is not None:
            out["val_loss"] = torch.stack(val)
        return out

    # ------------------------------------------------------------------
    def hyper_parameters(self) -> dict:
        """The constructor arguments of the model, as Lightning's ``save_hyperparameters`` records them."""
        m = self.model
        names = set(inspect.signature(type(m).__init__).parameters) - {"self"}
        alias = {"fourier_noise_scaling": "scale_noise"}
        return {k: getattr(m, alias.get(k, k)) for k in sorted(names)}

    def save_checkpoint(self, path) -> None:
        """A Lightning-format file: ``ScoreModule.load_from_checkpoint`` reads it unchanged; ``resume`` continues it."""
        cpu = lambda d: {k: v.detach().cpu().clone() for k, v in d.items()}  # noqa: E731
        torch.save({"state_dict": cpu(self.model.state_dict()), "hyper_parameters": self.hyper_parameters(),
                    "optimizer_states": [{"exp_avg": cpu(self.exp_avg), "exp_avg_sq": cpu(self.exp_avg_sq)}],
                    "global_step": self.global_step,
                    "trainer": {"seed": self.seed, "grad_clip": self.grad_clip, "weight_decay": self.weight_decay,
                                "betas": list(self.betas), "eps": self.eps, "p_uncond": self.p_uncond}}, path)

    def resume(self, path) -> None:
        """Load parameters, moments and the step count of ``save_checkpoint`` in place; training continues bit for bit."""
        from .schedulers import sde as _sde

        with torch.serialization.safe_globals([_sde.VPScheduler, _sde.VEScheduler]):
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for k, v in ckpt["state_dict"].items():
                params[k].copy_(v)
            opt = ckpt["optimizer_states"][0]
            for k in self.exp_avg:
                self.exp_avg[k].copy_(opt["exp_avg"][k])
                self.exp_avg_sq[k].copy_(opt["exp_avg_sq"][k])
        t = ckpt["trainer"]
        self.seed, self.grad_clip, self.weight_decay = int(t["seed"]), float(t["grad_clip"]), float(t["weight_decay"])
        self.betas, self.eps = (float(t["betas"][0]), float(t["betas"][1])), float(t["eps"])
        self.p_uncond = float(t.get("p_uncond", self.p_uncond))
        self.global_step = int(ckpt["global_step"])
        if self.model._native is not None:
            self.model._native.weights_key = None

    def __del__(self):
        try:
            if self.handle:
                self.lib.ffd_train_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass
