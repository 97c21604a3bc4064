"""``fdiff.sampling.sampler`` mirror: ``DiffusionSampler``
(reference src/fdiff/sampling/sampler.py:14-228).

Same constructor, attributes and ``sample`` / ``reverse_diffusion_step`` /
``sample_prior`` contracts.  ``sample`` keeps the reference's batching rules (remainder
samples dropped, Q10), cache lifecycle (reset only for batch 0, global step keeps
counting, Q3) and returns a CPU tensor, but runs each batch's whole reverse-diffusion
loop through ``ffd_sample_batch``: every kernel of every step is enqueued on the
current HIP stream with no host synchronisation (the reference syncs several times per
step: ``.item()``, ``min == max`` assert, H2D ``diag_embed`` copies).

Noise: ``rng="torch"`` (default) draws z exactly where the reference does --
``torch.randn`` on the CPU generator for the prior, ``torch.randn_like`` on the device
generator for every step -- so a seeded run matches the reference run on the same
device.  ``rng="philox"`` generates the draws inside the step kernel (Philox4x32-10
keyed by (seed, step, global element index)): no z traffic, and the NOISE is invariant
to how samples are sharded over GPUs.

Solver (extension): ``solver="euler_maruyama"`` (default) is the reference's integrator.  ``"ode_euler"`` and
``"ode_heun"`` integrate the probability-flow ODE of the same SDE (the same marginals, Song et al. 2021) through
``ffd_sample_batch_ode``: deterministic given the prior (no step noise is drawn), over the N - 1 intervals of the
N-point grid, ending exactly at ``eps``; Heun evaluates the model twice per interval and is second order.  Batching,
cache lifecycle and prior are unchanged; the global step of the cache gate counts intervals.
``"ode_ab2"`` (Adams-Bashforth 2 on the ODE's drift) and ``"dpmpp_2m"`` (DPM-Solver++ 2M, the exponential two-step form
on the data prediction) are linear multistep solvers of the same ODE: they reuse the previous interval's evaluation and
reach second order with ONE model call per interval, the cost of ``"ode_euler"`` (the trajectory's first interval has no
history and is first order).  Both are one device operation (``SDE.ode_multistep_step``) whose five coefficients the
host computes in float64; the history lives in the native context across the calls of one trajectory.  On the
analytic Gaussian case of the tests, at 32 evaluations: VP ``ode_ab2`` 2.40e-3, ``ode_heun`` 3.93e-3, ``dpmpp_2m``
2.14e-2 (it loses to Heun on this uniform-t grid); VE 5.08e-4 / 4.78e-3 / 5.53e-4.  Which wins on a trained network is
unmeasured.

Corrector (extension): ``corrector_steps=n > 0`` makes every Euler-Maruyama step a predictor-corrector step in
score_sde's order (``ffd_sample_batch_pc``): n Langevin corrector steps at t_i (``SDE.step_correct``: each its own score
evaluation and its own draw, signal-to-noise ratio ``snr``), then the unchanged predictor at t_i, whose noise is the
noise it has without correctors.  ``rng="torch"`` and ``inject_noise`` consume n + 1 draws per step in that order.  With
the cache the first evaluation of a step follows the gate and every later one is a pure hit.  No claim about sample
quality is made: there is no trained checkpoint to measure it on.

Conditioning (extension): ``sample_conditional`` / ``impute`` draw samples that agree with an observed part of a series
-- imputation, forecasting (a prefix mask) -- by replacement (Song et al. 2021, Appendix I.2; score_sde's
``get_inpaint_update_fn``) through ``ffd_sample_batch_cond``: after every state update of the predictor-corrector step
the observation, noised to the step's time level, is blended into the state under a time-axis mask
(``SDE.cond_project``; one fused launch for models that diffuse the spectrum).  ``rng="torch"`` and ``inject_noise``
consume two draws per update: its own, then the projection's.  No claim about sample quality is made: there is no
trained checkpoint to measure it on.

Resampling (extension): replacement draws the observed part independently of the unobserved part, and on a forecast
that error stays however fine the grid.  ``sample_conditional(..., resample=r, jump=j)`` is the
"time travel" of RePaint (Lugmayr et al. 2022) through ``ffd_sample_batch_resample``.  Schedule: the N reverse steps
are cut into blocks [0, j), [j, 2j), ... (the last may be shorter; j > N is one block) and every block runs r times;
between two passes of the block [i0, e) the whole state is diffused forward from ``timesteps[e]`` (0 behind the last
step) to ``timesteps[i0]`` with the SDE's exact transition kernel (``SDE.forward_transition``), with no projection
behind it.  That is r N visits and (r - 1) ceil(N / j) transitions.  Draw order under ``rng="torch"`` and
``inject_noise``: per visit what a conditional step consumes (per update its own draw, then its projection's), then
one more draw if a transition follows the visit; under ``rng="philox"`` the visit ordinal replaces the step index in
the stream tags and transition q draws under 0xE0000000 + q.  Cost: r times the score evaluations of the plain run.
``resample=1`` takes the replacement path unchanged.  It does not run with the cache (whose gate assumes that time only
falls) or under the ODE solvers.

Guidance (extension): ``sample_conditional(..., guidance=Guidance(...))`` / ``impute(..., guidance=...)`` steer every
Euler-Maruyama step by the gradient of the reconstruction loss through the score model (``sampling/guidance.py``;
``ffd_sample_batch_guided``): per step the score, the seed of the gradient (``ffd_guide_seed``), the model's input
vector-Jacobian product -- closed form for ``MixtureScoreModule``, the training backward without weight gradients for
``ScoreModule`` and ``MLPScoreModule`` through a parameter-only native training object that the sampler owns -- and the
guided score.  Draws as a conditional step without correctors: the predictor's, then the projection's slab (read only with
``Guidance.replace``).  ``guidance=None`` is the replacement path, untouched.  It raises ``NotImplementedError`` for
``LSTMScoreModule``, ``corrector_steps > 0``, an ODE solver, the cache, FreSca and ``resample > 1``.  What it buys on a
forecast, and what a step costs, is in DESIGN.md section 6.

Class labels (extension): with a ``ClassConditionalScoreModule``, ``sample`` / ``sample_conditional`` / ``impute`` take
``labels`` ((num_samples,) integers or one int, sliced per batch like an observation; -1 / ``n_classes`` / None: the null
class) and ``guidance_scale`` g: every score evaluation of the loop is ``s_u + g (s_c - s_u)`` (classifier-free guidance,
Ho & Salimans 2022) -- g = 1 the conditional score, g = 0 the unconditional one, anything else one evaluation at twice
the rows (``ffd_class_enable`` holds the batch's labels for as long as its loop calls run).  Every solver, the
correctors, replacement conditioning, resampling and FreSca run with it; ``log_likelihood``, ``Guidance`` and
``use_cache=True`` raise ``NotImplementedError``, and a model without classes takes no labels (``AssertionError``).

Likelihoods (extension): ``log_likelihood`` integrates the same ODE the other way, from ``eps`` up to 1, with the
divergence of its drift accumulated (Song et al. 2021, section 4.3), through ``ffd_loglik_batch``: log p(x) =
``SDE.prior_logp`` of the latent + the accumulated ``delta``.  No gradient of the network is taken: Hutchinson probes
with a central finite difference of the score, one model call at (1 + 2 n_probes) x the batch per evaluation.  It
processes EVERY series (the remainder batch included), draws its probes under ``rng`` / ``inject_noise``, and does not
run with the cache or FreSca.  Measured on the closed-form mixture: 100 Heun intervals are 0.015
(VP) / 0.073 (VE) nats from the exact answer at L = 8, one probe adds 0.2 nats rms per series.  On a trained network
nothing is measured (no checkpoint).

Two batch-wide statistics of the reference make the SAMPLES depend on the batching all the
same, sharded or not (they are properties of the reference's algorithm, reproduced here per
batch / per shard): the E2-CRF tables come from the batch's element 0 (caching.py:326-328), and
FreSca's default ``energy`` cutoff is derived from ``|rfft(score)|.mean(dim=(0, 2))`` over the
local batch (fresca.py:150-158).  The corrector's default ``corrector_norm="batch"`` is a third: its step size
comes from the norms of score and noise averaged over the local batch, as in score_sde and ``diffusers``.
``corrector_norm="sample"`` takes them per sample (the paper's form) and is the only shard-invariant one, at the price
of a stationary variance inflated by O(1 / (L C)): the step is large exactly for the samples near the mode.  Measured in
float64 on a Gaussian target (VE variance at t = 0.5, Fourier G, snr 0.16, 150 steps, 4096 samples), ratio to the exact
variance: L x C = 20 x 1: 1.24-1.25 (sample) against 1.02-1.03 (batch); 20 x 4: 1.07 / 1.02; 187 x 1: 1.04-1.05 /
1.02-1.03; 5 x 1: 2.2 / 1.01-1.05 (1 + eps / 2v ~ 1.025 is the discretisation's own bias).
Without the cache, with FreSca off or on its ``spatial`` cutoff, and without correctors or with the ``sample`` norm,
a sharded philox run reproduces the unsharded one: the same noise bit for bit, the samples to fp32 rounding
(a few 1e-7 relative per score evaluation; the contract the tests hold is 1e-5 of the max-norm over a trajectory) --
not bit for bit, because the kernels a batch size selects differ in summation order (the F-split small-batch FFN pair,
the key-split attention, the 32-row-per-wave large-batch FFN, the batch-tiled LSTM recurrence; csrc/ffd_small.hip,
ffd_ffn_rows.hip), and a shard may fall into another regime than the whole batch (tests/test_gpu_parity.py).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Literal, NamedTuple, Optional

import torch

from .. import _native as N
from ..models.score_models import ScoreModule, class_labels
from ..schedulers.sde import SDE
from ..utils.dataclasses import DiffusableBatch
from .guidance import Guidance


# solver name -> libffd's FFD_SOLVER_*
SOLVERS = {"euler_maruyama": N.FFD_SOLVER_EULER_MARUYAMA, "ode_euler": N.FFD_SOLVER_ODE_EULER,
           "ode_heun": N.FFD_SOLVER_ODE_HEUN}
# the linear multistep ODE solvers (kept apart: SOLVERS names the solvers with recorded Euler / Heun cases)
MULTISTEP_SOLVERS = {"ode_ab2": N.FFD_SOLVER_ODE_AB2, "dpmpp_2m": N.FFD_SOLVER_DPMPP_2M}
CORRECTOR_NORMS = {"batch": N.FFD_LANGEVIN_NORM_BATCH, "sample": N.FFD_LANGEVIN_NORM_SAMPLE}


class LogLikelihood(NamedTuple):
    """What ``DiffusionSampler.log_likelihood`` returns; CPU tensors, float64 but ``latent``.
    ``logp`` = ``prior_logp`` + ``delta`` (n,); ``bpd`` = -logp / (L C ln 2): bits per dimension of the DIFFUSED
    representation; ``latent``: the x_T (n, L, C) the ODE arrives at, or None."""
    logp: torch.Tensor
    prior_logp: torch.Tensor
    delta: torch.Tensor
    bpd: torch.Tensor
    latent: Optional[torch.Tensor]

    @classmethod
    def from_parts(cls, prior_logp: torch.Tensor, delta: torch.Tensor, L: int, Cn: int,
                   latent: Optional[torch.Tensor] = None) -> "LogLikelihood":
        prior_logp = prior_logp.to(torch.float64).cpu()
        delta = delta.to(torch.float64).cpu()
        logp = prior_logp + delta
        return cls(logp, prior_logp, delta, -logp / (L * Cn * math.log(2.0)), latent)


def _observation_and_mask(observed, mask, num_samples: int, L: int, Cn: int, what: str):
    """The shapes ``sample_conditional`` and ``impute`` take: ``observed`` (L, C) or (num_samples, L, C) -> (1 | n, L, C);
    ``mask`` (L,), (L, 1), (L, C) or the same with a leading 1 | n -> expanded to ``observed``'s shape.  fp32."""
    observed = torch.as_tensor(observed, dtype=torch.float32)
    mask = torch.as_tensor(mask, dtype=torch.float32)
    if observed.dim() == 2:
        observed = observed.unsqueeze(0)
    if observed.dim() != 3 or tuple(observed.shape[1:]) != (L, Cn) or observed.shape[0] not in (1, num_samples):
        raise ValueError(f"{what} must be (L, C) = {(L, Cn)} or (num_samples, L, C), got {tuple(observed.shape)}")
    if mask.dim() == 1:
        mask = mask.unsqueeze(-1)
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if mask.dim() != 3 or mask.shape[1] != L or mask.shape[2] not in (1, Cn) or mask.shape[0] not in (1, observed.shape[0]):
        raise ValueError(f"mask must be (L,), (L, 1), (L, C) or (num_samples, L, C) matching {what} "
                         f"{tuple(observed.shape)}, got {tuple(mask.shape)}")
    return observed, mask.expand(observed.shape)


class DiffusionSampler:
    def __init__(self, score_model: ScoreModule, sample_batch_size: int, use_cache: bool = False,
                 cache_kwargs: Optional[dict] = None, use_fresca: bool = False, fresca_low_scale: float = 1.0,
                 fresca_high_scale: float = 1.5, fresca_cutoff_ratio: float = 0.5,
                 fresca_cutoff_strategy: Literal["spatial", "energy"] = "energy",
                 rng: Literal["torch", "philox"] = "torch", seed: int = 42, sample_offset: int = 0,
                 z_chunk_steps: int = 50,
                 solver: Literal["euler_maruyama", "ode_euler", "ode_heun", "ode_ab2", "dpmpp_2m"] = "euler_maruyama",
                 corrector_steps: int = 0, snr: float = 0.16,
                 corrector_norm: Literal["batch", "sample"] = "batch") -> None:
        self.score_model = score_model
        self.noise_scheduler = score_model.noise_scheduler
        self.sample_batch_size = sample_batch_size
        self.n_channels = score_model.n_channels
        self.max_len = score_model.max_len

        self.use_cache = use_cache
        if use_cache:
            cache_kwargs = cache_kwargs or {}
            self.score_model.enable_caching(**cache_kwargs)  # sampler.py:37-39

        self.use_fresca = use_fresca
        self.fresca_low_scale = fresca_low_scale
        self.fresca_high_scale = fresca_high_scale
        self.fresca_cutoff_ratio = fresca_cutoff_ratio
        self.fresca_cutoff_strategy = fresca_cutoff_strategy
        if fresca_cutoff_strategy not in ("spatial", "energy"):
            self.fresca_cutoff_strategy = "spatial"  # sampler.py:83-85 maps anything but "energy" to "spatial"
        # extensions (not in the reference signature)
        assert rng in ("torch", "philox")
        self.rng = rng
        self.seed = int(seed)
        self.sample_offset = int(sample_offset)
        self.z_chunk_steps = int(z_chunk_steps)
        if not isinstance(solver, str) or (solver not in SOLVERS and solver not in MULTISTEP_SOLVERS):
            raise ValueError(f"solver must be one of {sorted(SOLVERS) + sorted(MULTISTEP_SOLVERS)}, got {solver!r}")
        self.solver = solver
        if corrector_steps < 0:
            raise ValueError(f"corrector_steps must be >= 0, got {corrector_steps!r}")
        if not snr > 0:
            raise ValueError(f"snr must be > 0, got {snr!r}")
        if corrector_norm not in CORRECTOR_NORMS:
            raise ValueError(f"corrector_norm must be one of {sorted(CORRECTOR_NORMS)}, got {corrector_norm!r}")
        if corrector_steps > 0 and solver != "euler_maruyama":
            raise ValueError("the ODE solvers are deterministic given the prior: corrector_steps > 0 needs "
                             "solver='euler_maruyama'")
        self.corrector_steps = int(corrector_steps)
        self.snr = float(snr)
        self.corrector_norm = corrector_norm
        self._injected = None
        self._multistep = None  # reverse_diffusion_step's (history, t, t_next) of its previous call
        self._guide_net = None  # guided sampling: the model's parameter-only native training object and what it is bound to

    def inject_noise(self, draws) -> None:
        """Parity hook: take every N(0,1) draw (one (B,L,C) array for each batch's prior,
        then one per step) from the iterable ``draws`` instead of torch's generators --
        the product-side twin of the noise patching in oracle/gen_golden.py."""
        self._injected = iter(draws) if draws is not None else None

    def _next_injected(self, shape, device) -> torch.Tensor:
        z = next(self._injected)
        z = torch.as_tensor(z, dtype=torch.float32)
        assert tuple(z.shape) == tuple(shape), (tuple(z.shape), tuple(shape))
        return z.to(device)

    # ------------------------------------------------------------------
    def reverse_diffusion_step(self, batch: DiffusableBatch, step: int = 0,
                               recompute_tokens: Optional[set] = None) -> torch.Tensor:
        """sampler.py:48-103 (single-step API; ``sample`` uses the fused loop)."""
        X = batch.X
        timesteps = batch.timesteps
        assert timesteps is not None and timesteps.size(0) == len(batch)
        t_lo, t_hi = float(torch.min(timesteps)), float(torch.max(timesteps))
        assert t_lo == t_hi  # sampler.py:59-60
        sch = self.noise_scheduler
        needs_grid = self.solver == "ode_heun" or self.solver in MULTISTEP_SOLVERS  # the interval's end is read from it
        t_next = self._next_grid_time(timesteps[0]) if needs_grid else None
        if self.corrector_steps > 0:
            return self._predictor_corrector_step(batch, t_lo, step, recompute_tokens)
        score = self._evaluate_score(batch, t_lo, step, recompute_tokens, update_crf=True)
        if self.solver == "euler_maruyama":
            output = sch.step(model_output=score, timestep=timesteps[0].item(), sample=X)
        elif self.solver == "ode_euler":
            output = sch.ode_step(model_output=score, timestep=timesteps[0].item(), sample=X)
        elif self.solver in MULTISTEP_SOLVERS:
            # the previous call's history continues the trajectory when this call starts where that one ended
            prev = self._multistep
            if prev is not None and (prev[2] != t_lo or prev[0].shape != X.shape or prev[0].device != X.device):
                prev = None
            output, hist = sch.ode_multistep_step(model_output=score, timestep=t_lo, timestep_next=t_next, sample=X,
                                                  method=self.solver, history=None if prev is None else prev[0],
                                                  timestep_prev=None if prev is None else prev[1])
            self._multistep = (hist, t_lo, t_next)
        else:  # Heun: a second model call at the predicted state and the interval's end (with the cache: a pure hit)
            X_pred, drift = sch.ode_heun_predict(model_output=score, timestep=timesteps[0].item(), sample=X)
            batch_pred = DiffusableBatch(X=X_pred, y=batch.y, timesteps=torch.full_like(timesteps, t_next))
            score_pred = self._evaluate_score(batch_pred, t_next, step, None if recompute_tokens is None else set(),
                                              update_crf=False)
            output = sch.ode_heun_correct(model_output_pred=score_pred, timestep_next=t_next, sample=X,
                                          sample_pred=X_pred, drift=drift)
        X_prev = output.prev_sample
        assert isinstance(X_prev, torch.Tensor)
        return X_prev

    def _predictor_corrector_step(self, batch: DiffusableBatch, t: float, step: int,
                                  recompute_tokens: Optional[set]) -> torch.Tensor:
        """``corrector_steps`` Langevin corrector steps at ``t``, then the Euler-Maruyama predictor at ``t`` on a fresh
        evaluation.  The step's first evaluation takes ``recompute_tokens`` and updates the CRF; the later ones
        recompute nothing.  Injected noise is consumed one draw per corrector, then the predictor's."""
        sch = self.noise_scheduler
        X = batch.X
        for k in range(self.corrector_steps + 1):
            cur = DiffusableBatch(X=X, y=batch.y, timesteps=batch.timesteps)
            first = k == 0
            score = self._evaluate_score(cur, t, step, recompute_tokens if first or recompute_tokens is None else set(),
                                         update_crf=first)
            noise = self._next_injected(X.shape, X.device) if self._injected is not None else None
            if k < self.corrector_steps:
                X = sch.step_correct(score, X, self.snr, t, noise=noise, norm=self.corrector_norm).prev_sample
            else:
                X = sch.step(model_output=score, timestep=batch.timesteps[0].item(), sample=X, noise=noise).prev_sample
        return X

    def _evaluate_score(self, batch: DiffusableBatch, t: float, step: int, recompute_tokens: Optional[set],
                        update_crf: bool) -> torch.Tensor:
        """One model call of ``reverse_diffusion_step`` with its cache bookkeeping and FreSca (sampler.py:62-93)."""
        if self.use_cache and recompute_tokens is not None:
            score, crf = self.score_model(batch, recompute_tokens=recompute_tokens, step=step, return_crf=True)
            if self.score_model.cache is not None and update_crf:
                self.score_model.cache.update_crf(crf, timestep=t)
                self.score_model.cache.current_step = step
        else:
            score = self.score_model(batch)
        if self.use_fresca:  # sampler.py:79-93
            from ..utils.fresca import apply_fresca_to_score

            score = apply_fresca_to_score(score, low_scale=self.fresca_low_scale, high_scale=self.fresca_high_scale,
                                          cutoff_ratio=self.fresca_cutoff_ratio,
                                          cutoff_strategy="energy" if self.fresca_cutoff_strategy == "energy" else "spatial",
                                          timestep=t, num_steps=getattr(self, "_num_diffusion_steps", None))
        return score

    def _next_grid_time(self, t: torch.Tensor) -> float:
        """The grid point after ``t``: Heun's corrector evaluates the model there, and the multistep solvers' interval
        ends there."""
        grid = getattr(self.noise_scheduler, "timesteps", None)
        if grid is None:
            raise ValueError(f"solver={self.solver!r} needs the scheduler's grid: call noise_scheduler.set_timesteps(n) "
                             "first")
        hit = torch.nonzero(grid.to(torch.float32) == t.detach().to(torch.float32).cpu()).flatten()
        if hit.numel() == 0 or int(hit[0]) >= grid.numel() - 1:
            raise ValueError(f"solver={self.solver!r} steps from a point of the scheduler's grid other than the last one; "
                             f"got t={float(t)!r}")
        return float(grid[int(hit[0]) + 1])

    def _solver_code(self) -> int:
        return SOLVERS[self.solver] if self.solver in SOLVERS else MULTISTEP_SOLVERS[self.solver]

    # ------------------------------------------------------------------
    def sample(self, num_samples: int, num_diffusion_steps: Optional[int] = None, *, labels=None,
               guidance_scale: float = 1.0) -> torch.Tensor:
        """sampler.py:105-215.  ``labels`` / ``guidance_scale`` (keyword only, an extension; a
        ``ClassConditionalScoreModule``): ``labels`` is ``(num_samples,)`` integers or one int, sliced per batch like an
        observation (-1 / ``n_classes`` / None: the null class); the score is ``s_u + g (s_c - s_u)`` -- g = 1 the
        conditional score, g = 0 the unconditional one, anything else one evaluation at twice the rows per step."""
        return self._sample(num_samples, num_diffusion_steps, None, self._class_args(labels, guidance_scale, num_samples))

    def _class_args(self, labels, guidance_scale, num_samples: int, guidance=None):
        """(labels as (num_samples,) int32 on the device or None, g) for a class-conditional model, else None; what
        labels cannot go with is refused here, before any device work."""
        n_classes = getattr(self.score_model, "n_classes", None)
        if n_classes is None:
            assert labels is None, f"{type(self.score_model).__name__} has no classes: labels must be None"
            assert float(guidance_scale) == 1.0, f"{type(self.score_model).__name__} has no classes: guidance_scale must be 1"
            return None
        if guidance is not None:
            raise NotImplementedError("a class-conditional model has no guided (reconstruction-guidance) form")
        if self.use_cache:
            raise NotImplementedError("a class-conditional model cannot run with use_cache=True: the E2-CRF tables are "
                                      "batch element 0's, which carry that sample's label")
        g = float(guidance_scale)
        if not math.isfinite(g):
            raise ValueError(f"guidance_scale must be finite, got {guidance_scale!r}")
        return class_labels(labels, num_samples, n_classes, self.score_model.device), g

    @staticmethod
    def _label_slice(labels: Optional[torch.Tensor], lo: int, n: int) -> Optional[torch.Tensor]:
        """the labels of the batch of samples [lo, lo + n)"""
        return None if labels is None else labels[lo:lo + n].contiguous()

    def _sample(self, num_samples: int, num_diffusion_steps: Optional[int], cond: Optional[dict],
                cls: Optional[tuple] = None) -> torch.Tensor:
        """``sample``; ``cond`` (``sample_conditional``): obs / mask (1 or num_samples, L, C) and std on the device,
        domain, final_replace; ``cls`` (``_class_args``): the labels and the guidance scale."""
        if num_diffusion_steps is not None:
            self._num_diffusion_steps = num_diffusion_steps
        self.score_model.eval()
        num_diffusion_steps = (self.score_model.num_training_steps if num_diffusion_steps is None
                               else num_diffusion_steps)
        # Euler-Maruyama takes one step per grid point; the ODE solvers walk the intervals between them and end at eps
        ode = self.solver != "euler_maruyama"
        if ode and num_diffusion_steps < 2:
            raise ValueError("the ODE solvers need a grid of at least two points")
        n_iter = num_diffusion_steps - 1 if ode else num_diffusion_steps
        self.noise_scheduler.set_timesteps(num_diffusion_steps)
        sch = self.noise_scheduler
        ts = sch.timesteps.to(torch.float32).contiguous()
        ts_c = (C.c_float * num_diffusion_steps)(*ts.tolist())
        step_size = float(sch.step_size)

        model = self.score_model
        ctx = model._ctx()
        if self.use_fresca:
            cfg = N.FrescaCfg(float(self.fresca_low_scale), float(self.fresca_high_scale),
                              float(self.fresca_cutoff_ratio),
                              1 if self.fresca_cutoff_strategy == "energy" else 0,
                              int(getattr(self, "_num_diffusion_steps", 0) or 0))
            N.check(ctx.lib.ffd_fresca_enable(ctx.handle, C.byref(cfg)), ctx.handle, "ffd_fresca_enable")
        else:
            N.check(ctx.lib.ffd_fresca_disable(ctx.handle), ctx.handle, "ffd_fresca_disable")
        device = model.device
        stream = N.current_stream_ptr(device)
        # resampled conditional sampling walks the visits of the host schedule: followed[u] = a transition follows visit u
        resample, jump = (cond["resample"], cond["jump"]) if cond is not None else (1, 1)
        followed = None
        if resample > 1:
            n_iter = ctx.lib.ffd_host_resample_visits(num_diffusion_steps, jump, resample)
            N.check(min(n_iter, 0), ctx.handle, "ffd_host_resample_visits")
            followed = []
            step_out, back_to = C.c_int(), C.c_int()
            for u in range(n_iter):
                N.check(ctx.lib.ffd_host_resample_visit(num_diffusion_steps, jump, resample, u, C.byref(step_out),
                                                        C.byref(back_to)), ctx.handle, "ffd_host_resample_visit")
                followed.append(back_to.value >= 0)
        # the draws the host hands over per iteration: every update's own (the correctors' in order, then the predictor's)
        # and, conditioned, its projection's behind it.  The ODE solvers draw nothing; philox draws inside the kernels.
        draws = 0
        if not ode and (self.rng == "torch" or self._injected is not None):
            draws = (self.corrector_steps + 1) * (2 if cond is not None else 1)
        all_samples = []
        num_batches = max(1, num_samples // self.sample_batch_size)  # remainder dropped (Q10)
        global_step = 0
        sample_cursor = self.sample_offset
        with torch.no_grad():
            for batch_idx in range(num_batches):
                batch_size = min(num_samples - batch_idx * self.sample_batch_size, self.sample_batch_size)
                X = self.sample_prior(batch_size, _sample_offset=sample_cursor)
                if self.use_cache and model.cache is not None and batch_idx == 0:
                    model.cache.reset()  # sampler.py:151-153
                    global_step = 0
                use_cache = int(self.use_cache and model.cache is not None)
                if use_cache:  # the gate reads K, R of the current cache object (sampler.py:179-200)
                    model._native_cache_configure(model.cache)
                cap = self._crf_capture_begin(ctx, device) if use_cache else None
                cond_cfg = guide = None
                if cond is not None:  # this batch's slice of the observation
                    lo = batch_idx * self.sample_batch_size
                    shared = cond["obs"].shape[0] == 1
                    obs = cond["obs"] if shared else cond["obs"][lo:lo + batch_size]
                    msk = cond["mask"] if shared else cond["mask"][lo:lo + batch_size]
                    cond_cfg = N.CondCfg(obs.data_ptr(), msk.data_ptr(),
                                         cond["std"].data_ptr() if cond["std"] is not None else None,
                                         1 if shared else batch_size, cond["domain"], int(cond["final_replace"]), 0)
                    if cond.get("guide") is not None:
                        g = cond["guide"]
                        guide = (N.GuideCfg(float(g.scale), float(g.obs_var), float(g.rho), int(g.replace), 0),
                                 self._guide_net_handle())
                done = 0
                scope = contextlib.nullcontext()
                if cls is not None:  # this batch's labels, for as long as its loop calls run
                    scope = model.class_state(self._label_slice(cls[0], batch_idx * self.sample_batch_size, batch_size),
                                              cls[1])
                with scope:
                    while done < n_iter:
                        n, n_draws = self._next_chunk(done, n_iter, draws, followed)
                        z = self._draw(n_draws, X.shape, device) if n_draws else None
                        self._loop_call(ctx, X, (ts_c, num_diffusion_steps, step_size), done, n,
                                        (self.seed, sample_cursor, z.data_ptr() if z is not None else None),
                                        (use_cache, (global_step + done) if use_cache else 0), cond_cfg, resample, jump,
                                        stream, guide)
                        if cap is not None:
                            self._crf_capture_collect(cap, global_step + done, n, ts, done)
                        done += n
                if use_cache:
                    N.check(ctx.lib.ffd_cache_crf_capture(ctx.handle, None), ctx.handle, "ffd_cache_crf_capture")
                    global_step += n_iter
                    model.cache.current_step = n_iter - 1  # sampler.py:73-74 leaves step_idx
                all_samples.append(X.cpu())
                # (the copy has drained the stream) a kernel-side time-out of this batch's launches is an error here
                N.check(ctx.lib.ffd_async_status(ctx.handle), ctx.handle, "sampling loop")
                sample_cursor += batch_size
        return torch.cat(all_samples, dim=0)

    def _next_chunk(self, done: int, n_iter: int, draws: int, followed: Optional[list]):
        """(iterations, draws) of the next loop call, which starts at iteration ``done``: whole iterations -- each
        ``draws`` draws, one more when a transition follows it (``followed``: resampling's visits) -- for as long as
        the z buffer stays within ``z_chunk_steps`` draws, and one at the least.  Nothing to hand over: all that is left."""
        if draws == 0:
            return n_iter - done, 0
        n = n_draws = 0
        while done + n < n_iter:
            more = draws + (int(followed[done + n]) if followed is not None else 0)
            if n > 0 and n_draws + more > self.z_chunk_steps:
                break
            n, n_draws = n + 1, n_draws + more
        return n, n_draws

    def _draw(self, n_draws: int, shape, device) -> torch.Tensor:
        """``n_draws`` N(0, 1) slabs in consumption order: the injected ones, or one ``normal_`` per draw, as the
        reference consumes its generator."""
        z = torch.empty((n_draws,) + tuple(shape), device=device, dtype=torch.float32)
        for i in range(n_draws):
            if self._injected is not None:
                z[i].copy_(self._next_injected(shape, device))
            else:
                z[i].normal_()
        return z

    def _loop_call(self, ctx, X, grid, first: int, n: int, noise, cache, cfg, resample: int, jump: int, stream,
                   guide=None) -> None:
        """Iterations [first, first + n) of the native loop on ``X``, through the entry this sampler's configuration
        selects.  ``grid``: (timesteps, n_steps, step_size); ``noise``: (seed, sample_offset, z_inject); ``cache``:
        (use_cache, global_step0); ``cfg``: the batch's ``CondCfg`` or None."""
        corrector = (self.corrector_steps, self.snr, CORRECTOR_NORMS[self.corrector_norm])
        if guide is not None:  # guided sampling: (GuideCfg, the network's training object or None)
            guide_cfg, net = guide
            rc = ctx.lib.ffd_sample_batch_guided(ctx.handle, net, X.data_ptr(), X.shape[0], *grid, first, n, *noise,
                                                 C.byref(cfg), C.byref(guide_cfg), None, stream)
            N.check(rc, ctx.handle, "ffd_sample_batch_guided")
            return
        if self.solver != "euler_maruyama":  # deterministic given the prior: no noise arguments
            name, rest = "ffd_sample_batch_ode", (self._solver_code(), *cache)
        elif cfg is not None and resample > 1:  # (no cache: _check_resampling)
            name, rest = "ffd_sample_batch_resample", (jump, resample, *corrector, *noise, C.byref(cfg))
        elif cfg is not None:
            name, rest = "ffd_sample_batch_cond", (*corrector, *noise, *cache, C.byref(cfg))
        elif self.corrector_steps > 0:
            name, rest = "ffd_sample_batch_pc", (*corrector, *noise, *cache)
        else:
            name, rest = "ffd_sample_batch", (*noise, *cache)
        rc = getattr(ctx.lib, name)(ctx.handle, X.data_ptr(), X.shape[0], *grid, first, n, *rest, stream)
        N.check(rc, ctx.handle, name)

    # ------------------------------------------------------------------
    # log-likelihoods through the probability-flow ODE (extension)
    @staticmethod
    def _likelihood_batches(n: int, batch_size: int) -> list:
        """(first row, rows) of every batch of ``log_likelihood``: the remainder is a batch too -- every series gets a
        number (``sample`` drops it, as the reference does)."""
        return [(lo, min(batch_size, n - lo)) for lo in range(0, n, batch_size)]

    def _draw_probes(self, n_draws: int, shape, device) -> torch.Tensor:
        """``n_draws`` probe slabs in consumption order: the injected ones (any finite values), or Rademacher draws on
        the device generator."""
        z = torch.empty((n_draws,) + tuple(shape), device=device, dtype=torch.float32)
        for i in range(n_draws):
            if self._injected is not None:
                z[i].copy_(self._next_injected(shape, device))
            else:
                z[i].copy_(torch.randint(0, 2, tuple(shape), device=device).to(torch.float32).mul_(2.0).sub_(1.0))
        return z

    def log_likelihood(self, X: torch.Tensor, num_diffusion_steps: Optional[int] = None, *, solver: str = "ode_heun",
                       n_probes: int = 1, fd_rel: float = 1e-2, return_latent: bool = False,
                       labels=None) -> "LogLikelihood":
        """log p(x) of every series of ``X`` (n, L, C) under the model, by the instantaneous change of variables along
        the probability-flow ODE (Song et al. 2021, section 4.3): the ODE of ``solver="ode_euler"`` / ``"ode_heun"``
        integrated the other way, from ``eps`` up to 1, over the N - 1 intervals of the scheduler's N-point grid, with
        the divergence of its drift accumulated (``ffd_loglik_batch``), plus ``SDE.prior_logp`` of the latent it arrives
        at.  No gradient of the network is taken: the divergence is Hutchinson's estimate from ``n_probes`` fresh
        Rademacher probes per evaluation with a central finite difference of the score of step ``fd_rel`` x the
        marginal's standard deviation, one model call at (1 + 2 n_probes) x the batch per evaluation.
        ``X`` lives in the DIFFUSED domain -- for a spectral model what ``dft`` / ``ffd_dft_standardize`` produce -- and the
        likelihood is that of this representation: the constant log-determinant of the packed transform and of the
        standardization is not added, so ``bpd`` is not comparable across domains (or with time-domain models).
        Batches of ``sample_batch_size``, the remainder included.  Honours ``rng`` (``"philox"``: probes drawn in the
        kernels under ``seed`` / ``sample_offset``; ``"torch"``: Rademacher slabs from the device generator, handed over in
        chunks of ``z_chunk_steps``) and ``inject_noise`` (one (B, L, C) slab per (evaluation, probe) in consumption
        order; any finite values -- ``sqrt(D) e_j`` with ``n_probes = D`` gives the exact trace).  The sampler's own
        ``solver`` and ``corrector_steps`` are not consulted.  Raises ``ValueError`` with the cache or FreSca: a rescaled
        score is not the model's ODE, and the cache's gate assumes falling time.  Returns a ``LogLikelihood``."""
        if labels is not None or getattr(self.score_model, "n_classes", None) is not None:
            raise NotImplementedError("log_likelihood has no class-conditional form")
        if self.use_cache:
            raise ValueError("log_likelihood cannot run with use_cache=True: the E2-CRF cache's gate and tables assume "
                             "that the diffusion time only falls")
        if self.use_fresca:
            raise ValueError("log_likelihood cannot run with use_fresca=True: a rescaled score is not the model's "
                             "probability-flow ODE")
        if solver not in ("ode_euler", "ode_heun"):
            raise ValueError(f"solver must be 'ode_euler' or 'ode_heun', got {solver!r}")
        if isinstance(n_probes, bool) or not isinstance(n_probes, int) or n_probes < 1:
            raise ValueError(f"n_probes must be an integer >= 1, got {n_probes!r}")
        try:
            fd_ok = 0.0 < float(fd_rel) < float("inf")
        except (TypeError, ValueError):
            fd_ok = False
        if not fd_ok:
            raise ValueError(f"fd_rel must be > 0 and finite, got {fd_rel!r}")
        steps = self.score_model.num_training_steps if num_diffusion_steps is None else num_diffusion_steps
        if steps < 2:
            raise ValueError("log_likelihood needs a grid of at least two points")
        L, Cn = self.max_len, self.n_channels
        X = torch.as_tensor(X, dtype=torch.float32)
        if X.dim() != 3 or tuple(X.shape[1:]) != (L, Cn) or X.shape[0] < 1:
            raise ValueError(f"X must be (n, L, C) with (L, C) = {(L, Cn)} and n >= 1, got {tuple(X.shape)}")
        self.score_model.eval()
        sch = self.noise_scheduler
        sch.set_timesteps(steps)
        ts_c = (C.c_float * steps)(*sch.timesteps.to(torch.float32).tolist())
        model = self.score_model
        ctx = model._ctx()
        N.check(ctx.lib.ffd_fresca_disable(ctx.handle), ctx.handle, "ffd_fresca_disable")
        device = model.device
        stream = N.current_stream_ptr(device)
        heun = solver == "ode_heun"
        n_iter = steps - 1
        handed = self.rng == "torch" or self._injected is not None
        draws = (2 if heun else 1) * n_probes if handed else 0  # probe slabs the host hands over per interval
        priors, deltas, latents = [], [], []
        sample_cursor = self.sample_offset
        with torch.no_grad():
            for lo, B in self._likelihood_batches(X.shape[0], self.sample_batch_size):
                x = X[lo:lo + B].to(device).contiguous().clone()
                delta = torch.zeros(B, device=device, dtype=torch.float64)
                done = 0
                while done < n_iter:
                    n, n_draws = self._next_chunk(done, n_iter, draws, None)
                    z = self._draw_probes(n_draws, x.shape, device) if n_draws else None
                    rc = ctx.lib.ffd_loglik_batch(ctx.handle, x.data_ptr(), delta.data_ptr(), B, ts_c, steps, done, n,
                                                  SOLVERS[solver], n_probes, float(fd_rel),
                                                  z.data_ptr() if z is not None else None, self.seed, sample_cursor, stream)
                    N.check(rc, ctx.handle, "ffd_loglik_batch")
                    done += n
                priors.append(sch.prior_logp(x).cpu())
                deltas.append(delta.cpu())
                if return_latent:
                    latents.append(x.cpu())
                # (the copies have drained the stream) a kernel-side time-out of this batch's launches is an error here
                N.check(ctx.lib.ffd_async_status(ctx.handle), ctx.handle, "log-likelihood loop")
                sample_cursor += B
        return LogLikelihood.from_parts(torch.cat(priors), torch.cat(deltas), L, Cn,
                                        torch.cat(latents) if return_latent else None)

    # ------------------------------------------------------------------
    # conditional sampling by replacement (extension)
    def _check_resampling(self, resample, jump) -> None:
        for name, v in (("resample", resample), ("jump", jump)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        if resample > 1 and self.use_cache:
            raise ValueError("resample > 1 cannot run with use_cache=True: the E2-CRF cache's gate and tables assume that "
                             "the diffusion time only falls, and resampling moves it back up")

    def _check_conditional(self, resample, jump) -> None:
        """What ``sample_conditional`` and ``impute`` refuse before any device work."""
        if self.solver != "euler_maruyama":
            raise ValueError("conditional sampling by replacement is defined for the predictor-corrector sampler: "
                             "it needs solver='euler_maruyama'")
        self._check_resampling(resample, jump)

    def _check_guidance(self, guidance, resample) -> None:
        """What guided sampling refuses before any device work."""
        if guidance is None:
            return
        if not isinstance(guidance, Guidance):
            raise TypeError(f"guidance must be a Guidance or None, got {type(guidance).__name__}")
        kind = getattr(self.score_model, "_kind", None)
        if kind == N.FFD_MODEL_LSTM:
            raise NotImplementedError("guided sampling needs the gradient through the score model: LSTMScoreModule has no "
                                      "backward pass")
        if kind not in (N.FFD_MODEL_TRANSFORMER, N.FFD_MODEL_MLP, N.FFD_MODEL_MIXTURE):
            raise NotImplementedError(f"guided sampling is not defined for {type(self.score_model).__name__}")
        if self.corrector_steps > 0:
            raise NotImplementedError("guided sampling runs without correctors: corrector_steps must be 0")
        if self.solver != "euler_maruyama":
            raise NotImplementedError("guided sampling is an Euler-Maruyama step: it needs solver='euler_maruyama'")
        if self.use_cache:
            raise NotImplementedError("guided sampling cannot run with use_cache=True: the vector-Jacobian product is the "
                                      "uncached network's")
        if self.use_fresca:
            raise NotImplementedError("guided sampling cannot run with use_fresca=True: the vector-Jacobian product is the "
                                      "unscaled score's")
        if resample > 1:
            raise NotImplementedError("guided sampling has no resampled form: resample must be 1")

    def _guide_net_handle(self):
        """The native training object guided sampling takes the network's forward and input VJP from: one per sampler
        (its model), bound to the parameters alone (``ffd_train_bind_params``) and bound again when their storage has
        moved.  The mixture evaluates both in closed form: None."""
        model = self.score_model
        if getattr(model, "_kind", None) == N.FFD_MODEL_MIXTURE:
            return None
        lib = N.lib()

        def check(rc, what):
            if rc:
                raw = lib.ffd_train_last_error(self._guide_net["handle"])
                exc = {-1: AssertionError, -2: NotImplementedError}.get(rc, N.FFDError)
                raise exc(f"libffd {what} failed (status {rc}): {raw.decode() if raw else ''}")

        if self._guide_net is None:
            dev = model.device
            self._guide_net = {"handle": C.c_void_p(), "bound": None}
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            check(lib.ffd_train_create(C.byref(self._guide_net["handle"]), C.byref(model._desc()), 0.0, idx), "ffd_train_create")
        ptrs = [(name, p.data_ptr()) for name, p in model.named_parameters()]
        if ptrs != self._guide_net["bound"]:
            for name, p in model.named_parameters():
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise AssertionError(f"{name} must be contiguous float32")
                check(lib.ffd_train_bind_params(self._guide_net["handle"], name.encode(), p.data_ptr(), p.numel()),
                      f"ffd_train_bind_params({name})")
            self._guide_net["bound"] = ptrs
        return self._guide_net["handle"]

    def __del__(self):
        try:
            if self._guide_net is not None and self._guide_net["handle"]:
                N.lib().ffd_train_destroy(self._guide_net["handle"])
                self._guide_net = None
        except Exception:
            pass

    def sample_conditional(self, observed: torch.Tensor, mask: torch.Tensor, num_samples: int,
                           num_diffusion_steps: Optional[int] = None, resample: int = 1, jump: int = 1, *,
                           domain: Optional[str] = None, feature_std: Optional[torch.Tensor] = None,
                           final_replace: bool = True, **extensions) -> torch.Tensor:
        """``sample`` conditioned on ``observed`` where ``mask`` is 1: after every state update of every reverse step the
        observation, noised to that step's time, replaces the observed part of the state (``SDE.cond_project``).
        ``observed`` lives in the diffused domain (for a spectral model: the packed, standardized spectrum of the series,
        its unobserved time points filled with anything finite); ``mask`` lives on the time axis.  Both are (L, C) --
        shared by all samples: many completions of one series -- or (num_samples, L, C), sliced per batch; a mask of
        shape (L,) or (L, 1) is broadcast over the channels.  ``domain=None`` picks "frequency" when the model scales its
        noise for the spectrum (``score_model.scale_noise``), else "time".  ``feature_std`` (L, C): the dataset's
        standardization of the spectrum (frequency domain only).  ``final_replace`` ends with one noiseless
        replacement, so that the observed points come back exact to transform rounding.  Honours ``corrector_steps``,
        ``snr``, ``corrector_norm``, ``rng``, ``seed``, ``sample_offset``, ``inject_noise``, the cache and FreSca;
        batching, cache lifecycle and prior are those of ``sample``.  Returns a CPU tensor in the diffused domain.
        A forecast is the prefix mask ``mask[:n_known] = 1``.  ``resample=r > 1`` runs every block of ``jump`` steps r
        times with a forward transition in between (the module docstring's "Resampling"), at r times the evaluations;
        ``resample=1`` is plain replacement whatever ``jump`` is.
        ``labels`` / ``guidance_scale`` (keyword only, through ``extensions``): as in ``sample``.
        ``guidance=None`` (keyword only, the one name ``extensions`` takes: a ``Guidance``; the module docstring's
        "Guidance") steers every step by the gradient of the reconstruction loss through the score model instead of (or,
        with ``Guidance.replace``, before) the replacement; ``final_replace`` still ends the run with one noiseless
        replacement.  None: the replacement path, untouched."""
        guidance = extensions.pop("guidance", None)
        labels, guidance_scale = extensions.pop("labels", None), extensions.pop("guidance_scale", 1.0)
        if extensions:
            raise TypeError(f"sample_conditional() got an unexpected keyword argument {next(iter(extensions))!r}")
        self._check_guidance(guidance, resample)
        self._check_conditional(resample, jump)
        cls = self._class_args(labels, guidance_scale, num_samples, guidance)
        if domain is None:
            domain = "frequency" if getattr(self.score_model, "scale_noise", False) else "time"
        if domain not in ("frequency", "time"):
            raise ValueError(f"domain must be 'frequency' or 'time', got {domain!r}")
        if domain == "time" and feature_std is not None:
            raise ValueError("feature_std belongs to the frequency domain")
        L, Cn = self.max_len, self.n_channels
        observed, mask = _observation_and_mask(observed, mask, num_samples, L, Cn, "observed")
        if feature_std is not None:
            feature_std = torch.as_tensor(feature_std, dtype=torch.float32)
            if tuple(feature_std.shape) != (L, Cn):
                raise ValueError(f"feature_std must be (L, C) = {(L, Cn)}, got {tuple(feature_std.shape)}")
        device = self.score_model.device
        cond = dict(obs=observed.to(device).contiguous(), mask=mask.to(device).contiguous(),
                    std=feature_std.to(device).contiguous() if feature_std is not None else None,
                    domain=N.FFD_COND_FREQUENCY if domain == "frequency" else N.FFD_COND_TIME,
                    final_replace=bool(final_replace), resample=resample, jump=jump, guide=guidance)
        return self._sample(num_samples, num_diffusion_steps, cond, cls)

    def impute(self, series_time: torch.Tensor, mask: torch.Tensor, num_samples: int,
               num_diffusion_steps: Optional[int] = None, resample: int = 1, jump: int = 1, *,
               feature_mean: Optional[torch.Tensor] = None, feature_std: Optional[torch.Tensor] = None,
               final_replace: bool = True, guidance: Optional[Guidance] = None, labels=None,
               guidance_scale: float = 1.0) -> torch.Tensor:
        """Complete a time series with a model that diffuses its spectrum: ``series_time`` (L, C) or
        (num_samples, L, C) holds the series, ``mask`` (as in ``sample_conditional``) is 1 at its observed points.
        The unobserved points are zero-filled, the series goes through ``dft`` (with the dataset's ``feature_mean`` /
        ``feature_std`` (L, C): ``ffd_dft_standardize``), ``sample_conditional`` runs in the frequency domain, and the
        samples come back as TIME series (``ffd_unstandardize_idft`` / ``idft``) on the CPU.  Forecasting is the
        prefix mask: ``mask[:n_known] = 1`` draws ``num_samples`` continuations of the first ``n_known`` points.
        ``resample`` / ``jump`` / ``guidance`` / ``labels`` / ``guidance_scale``: as in ``sample_conditional``."""
        if (feature_mean is None) != (feature_std is None):
            raise ValueError("feature_mean and feature_std go together")
        self._check_guidance(guidance, resample)
        self._check_conditional(resample, jump)  # (sample_conditional's refusals, before the transform below)
        self._class_args(labels, guidance_scale, num_samples, guidance)
        L, Cn = self.max_len, self.n_channels
        series, m = _observation_and_mask(series_time, mask, num_samples, L, Cn, "series_time")
        device = self.score_model.device
        if device.type != "cuda":
            raise N.FFDError("sampling needs an MI355X (gfx950) device; there is no CPU fallback")
        lib, stream = N.lib(), N.current_stream_ptr(device)
        filled = (series * m).to(device).contiguous()  # zero fill: the fill does not reach the result beyond rounding
        obs = torch.empty_like(filled)
        Bo = filled.shape[0]
        mean_d = std_d = None
        if feature_mean is not None:
            mean_d = torch.as_tensor(feature_mean, dtype=torch.float32).to(device).contiguous()
            std_d = torch.as_tensor(feature_std, dtype=torch.float32).to(device).contiguous()
            if tuple(mean_d.shape) != (L, Cn) or tuple(std_d.shape) != (L, Cn):
                raise ValueError(f"feature_mean / feature_std must be (L, C) = {(L, Cn)}")
            N.check(lib.ffd_dft_standardize(filled.data_ptr(), obs.data_ptr(), mean_d.data_ptr(), std_d.data_ptr(), Bo, L,
                                            Cn, stream), None, "ffd_dft_standardize")
        else:
            N.check(lib.ffd_dft(filled.data_ptr(), obs.data_ptr(), Bo, L, Cn, stream), None, "ffd_dft")
        out = self.sample_conditional(obs, m, num_samples, num_diffusion_steps, domain="frequency",
                                      feature_std=std_d, final_replace=final_replace, resample=resample, jump=jump,
                                      guidance=guidance, labels=labels, guidance_scale=guidance_scale)
        xf = out.to(device).contiguous()
        xt = torch.empty_like(xf)
        if mean_d is not None:
            N.check(lib.ffd_unstandardize_idft(xf.data_ptr(), xt.data_ptr(), mean_d.data_ptr(), std_d.data_ptr(),
                                               xf.shape[0], L, Cn, stream), None, "ffd_unstandardize_idft")
        else:
            N.check(lib.ffd_idft(xf.data_ptr(), xt.data_ptr(), xf.shape[0], L, Cn, stream), None, "ffd_idft")
        return xt.cpu()

    # ------------------------------------------------------------------
    # cache.update_crf (sampler.py:70-73) for the fused loop: the native loop writes the CRF of the steps the
    # reference would have stored (E2CRFCache.update_crf, caching.py:474-522) into these buffers.
    def _crf_capture_begin(self, ctx, device):
        cache = self.score_model.cache
        m = self.score_model
        shape = (m.num_layers, m.max_len, m.d_model)
        last = torch.empty(shape, device=device, dtype=torch.float32)
        ring = None
        if cache.use_freqca:
            ring = torch.empty((max(1, int(cache.max_history)),) + shape, device=device, dtype=torch.float32)
        cfg = N.CrfCaptureCfg(ring.data_ptr() if ring is not None else None, ring.shape[0] if ring is not None else 0,
                              max(1, int(cache.freq_decomp_interval)) if ring is not None else 0, last.data_ptr(),
                              1 if cache.use_freqca else max(1, int(cache.R)), 0)
        N.check(ctx.lib.ffd_cache_crf_capture(ctx.handle, C.byref(cfg)), ctx.handle, "ffd_cache_crf_capture")
        return {"last": last, "ring": ring, "cfg": cfg}

    def _crf_capture_collect(self, cap, g0: int, n: int, ts: torch.Tensor, step0: int) -> None:
        """Fold what ffd_sample_batch captured over global steps [g0, g0+n) into the cache object."""
        cache = self.score_model.cache
        cfg = cap["cfg"]
        if any(g % cfg.last_every == 0 for g in range(g0, g0 + n)):
            cache.crf_cache = cap["last"].clone()
        if cap["ring"] is not None:
            from ..utils.fourier import frequency_decompose_dct, frequency_decompose_fft

            fn = frequency_decompose_fft if cache.freq_decomp == "fft" else frequency_decompose_dct
            hits = [g for g in range(g0, g0 + n) if g % cfg.every == 0][-cfg.n_slots:]
            for g in hits:  # only the newest max_history decompositions can survive in the history
                slot = (g // cfg.every) % cfg.n_slots
                low, high = fn(cap["ring"][slot], cache.low_freq_ratio)
                cache._push_decomposition(low, high, float(ts[step0 + (g - g0)]))

    def sample_prior(self, batch_size: int, _sample_offset: int = 0) -> torch.Tensor:
        """sampler.py:217-228."""
        if not isinstance(self.noise_scheduler, SDE):
            raise NotImplementedError("Scheduler not recognized.")
        device = self.score_model.device
        shape = (batch_size, self.max_len, self.n_channels)
        if self._injected is None and self.rng == "torch":
            X = self.noise_scheduler.prior_sampling(shape, device=device)
        else:  # ffd_prior: from the injected draw, or (philox) drawn in the kernel under (seed, sample offset)
            if device.type != "cuda":
                raise N.FFDError("sampling needs an MI355X (gfx950) device; there is no CPU fallback")
            sch = self.noise_scheduler
            z = self._next_injected(shape, device) if self._injected is not None else None
            z_ptr, seed, offset = (z.data_ptr(), 0, 0) if z is not None else (None, self.seed, _sample_offset)
            X = torch.empty(shape, device=device, dtype=torch.float32)
            desc = sch._desc()
            rc = N.lib().ffd_prior(C.byref(desc), X.data_ptr(), z_ptr, sch._G_on(device).data_ptr(), seed, offset,
                                   batch_size, self.max_len, self.n_channels, N.current_stream_ptr(device))
            N.check(rc, None, "ffd_prior")
        assert isinstance(X, torch.Tensor)
        return X
