"""``fdiff.schedulers.sde`` mirror: SDE / VPScheduler / VEScheduler.

Same constructor arguments, attributes (``G``, ``G_matrix``, ``timesteps``,
``step_size``, ``T``, ``eps``, ``noise_scaling``) and methods as the reference
(src/fdiff/schedulers/sde.py:13-246).  The host keeps the small tables as torch CPU
tensors exactly like the reference; the per-step arithmetic (``step``,
``prior_sampling`` on device tensors) runs in libffd's fused HIP kernel
(csrc/ffd_elem.hip) instead of the reference's dense diag(L x L) matmuls.
"""
from __future__ import annotations

import abc
import ctypes as C
import math
from collections import namedtuple
from typing import Optional

import torch

from .. import _native as N

SamplingOutput = namedtuple("SamplingOutput", ["prev_sample"])
# multistep method name -> libffd's FFD_SOLVER_*
MULTISTEP_METHODS = {"ode_ab2": N.FFD_SOLVER_ODE_AB2, "dpmpp_2m": N.FFD_SOLVER_DPMPP_2M}


class SDE(abc.ABC):
    """sde.py:13-87."""

    _sde_kind = -1

    def __init__(self, fourier_noise_scaling: bool = False, eps: float = 1e-5):
        super().__init__()
        self.noise_scaling = fourier_noise_scaling
        self.eps = eps
        self.G: Optional[torch.Tensor] = None
        self._G_dev = {}

    def __getstate__(self):
        """The scheduler travels in a checkpoint's ``hyper_parameters``: without its per-device copies of G, which a load
        with ``map_location="cpu"`` would bring back as HOST tensors under a device's key."""
        state = dict(self.__dict__)
        state["_G_dev"] = {}
        return state

    @property
    def T(self) -> float:
        return 1.0

    # -- tables (host, torch CPU: identical ops to the reference) ------------
    def set_noise_scaling(self, max_len: int) -> None:
        """sde.py:42-60."""
        G = torch.ones(max_len)
        if self.noise_scaling:
            G = 1 / (math.sqrt(2)) * G
            G[0] *= math.sqrt(2)
            if max_len % 2 == 0:
                G[max_len // 2] *= math.sqrt(2)
        self.G = G
        self.G_matrix = torch.diag(G)
        self._G_dev = {}
        assert G.shape[0] == max_len

    def set_timesteps(self, num_diffusion_steps: int) -> None:
        """sde.py:62-64."""
        self.timesteps = torch.linspace(1.0, self.eps, num_diffusion_steps)
        self.step_size = self.timesteps[0] - self.timesteps[1]

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """sde.py:66-77 (training-side helper; plain tensor arithmetic)."""
        mean, _ = self.marginal_prob(original_samples, timesteps)
        return mean + noise

    @abc.abstractmethod
    def marginal_prob(self, x: torch.Tensor, t: torch.Tensor):
        ...

    @abc.abstractmethod
    def marginal_coeffs(self, t: torch.Tensor):
        """(mean_coeff, sigma), both shaped like ``t``: the per-sample factors of ``marginal_prob`` --
        mean = mean_coeff * x and std = sigma[:, None] * G -- formed by its own expressions on the device ``t`` lives
        on.  The score-matching loss kernels (csrc/ffd_loss.hip) take them as inputs."""

    @abc.abstractmethod
    def _sde_ab(self) -> tuple:
        ...

    # -- device plumbing -------------------------------------------------------
    def _desc(self) -> N.SdeDesc:
        a, b = self._sde_ab()
        return N.SdeDesc(self._sde_kind, 0, float(a), float(b))

    def _G_on(self, device: torch.device) -> torch.Tensor:
        assert self.G is not None, "call set_noise_scaling(max_len) first (sde.py:113-114 sets it lazily only in marginal_prob)"
        key = str(device)
        g = self._G_dev.get(key)
        if g is None or g.numel() != self.G.numel() or g.device != torch.device(device):  # (never a pointer off the device)
            g = self.G.to(device=device, dtype=torch.float32).contiguous()
            self._G_dev[key] = g
        return g

    def prior_sampling(self, shape: tuple, device: Optional[torch.device] = None) -> torch.Tensor:
        """sde.py:79-87 (VE: 125-127).  Like the reference, the N(0,1) draw comes from
        torch's CPU generator (``torch.randn(*shape)``) so that seeds line up; the
        G-scaling (the reference's dense G_matrix @ z) runs in the HIP kernel.  With
        ``device=None`` the result is returned on the CPU as in the reference; passing a
        cuda device (extension) keeps it resident."""
        assert self.G is not None
        z = torch.randn(*shape)
        if not torch.cuda.is_available():
            raise N.FFDError("prior_sampling needs an MI355X (gfx950) device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        zd = z.to(dev)
        x = torch.empty_like(zd)
        B, L, Cn = shape
        desc = self._desc()
        rc = N.lib().ffd_prior(C.byref(desc), x.data_ptr(), zd.data_ptr(), self._G_on(dev).data_ptr(), 0, 0, B, L,
                               Cn, N.current_stream_ptr(dev))
        N.check(rc, None, "ffd_prior")
        return x.cpu() if device is None else x

    def _prior_scale(self) -> float:
        return 1.0

    def prior_logp(self, x: torch.Tensor) -> torch.Tensor:
        """log-density of ``x`` (B, L, C) under the distribution ``prior_sampling`` draws from (extension):
        sum over (l, c) of log N(x; 0, (sigma_p G_l)^2), sigma_p = 1 (VP) or ``sigma_max`` (VE).  fp32 terms summed in
        float64 in a fixed order (``ffd_prior_logp``); returns a (B,) float64 tensor on ``x``'s device."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError(f"x must be a (B, L, C) tensor, got {tuple(getattr(x, 'shape', ()))}")
        B, L, Cn = x.shape
        if self.G is None or self.G.numel() != L:
            raise ValueError(f"x has length {L}, but the noise scaling is set for "
                             f"{None if self.G is None else self.G.numel()}: call set_noise_scaling({L}) first")
        x = N.require_gpu_tensor(x, "x")
        out = torch.empty(B, device=x.device, dtype=torch.float64)
        desc = self._desc()
        rc = N.lib().ffd_prior_logp(C.byref(desc), x.data_ptr(), self._G_on(x.device).data_ptr(), out.data_ptr(), B, L, Cn,
                                    N.current_stream_ptr(x.device))
        N.check(rc, None, "ffd_prior_logp")
        return out

    def step(self, model_output: torch.Tensor, timestep: float, sample: torch.Tensor,
             noise: Optional[torch.Tensor] = None) -> SamplingOutput:
        """sde.py:129-165 / 215-246.  ``noise`` (extension) injects z; by default
        z = torch.randn_like(sample), exactly where the reference draws it."""
        sample = N.require_gpu_tensor(sample, "sample")
        model_output = N.require_gpu_tensor(model_output, "model_output")
        assert self.step_size > 0
        B, L, Cn = sample.shape
        z = torch.randn_like(sample) if noise is None else N.require_gpu_tensor(noise, "noise")
        x = sample.clone()
        desc = self._desc()
        rc = N.lib().ffd_sde_step(C.byref(desc), x.data_ptr(), model_output.data_ptr(),
                                  self._G_on(sample.device).data_ptr(), float(timestep), float(self.step_size),
                                  z.data_ptr(), 0, 0, 0, B, L, Cn, N.current_stream_ptr(sample.device))
        N.check(rc, None, "ffd_sde_step")
        return SamplingOutput(prev_sample=x)

    # -- probability-flow ODE (extension: the reference has ``step`` only) ------
    def _ode_args(self, sample: torch.Tensor, model_output: torch.Tensor):
        sample = N.require_gpu_tensor(sample, "sample")
        model_output = N.require_gpu_tensor(model_output, "model_output")
        assert self.step_size > 0
        assert sample.shape == model_output.shape
        return sample, model_output, self._G_on(sample.device).data_ptr(), N.current_stream_ptr(sample.device)

    def ode_step(self, model_output: torch.Tensor, timestep: float, sample: torch.Tensor) -> SamplingOutput:
        """One Euler interval of the probability-flow ODE from ``timestep`` down by ``step_size``:
        x - (f(x, t) - (g(t) G)^2 score / 2) * step_size, with f, g and G of ``step``.  No noise is drawn."""
        sample, model_output, G, stream = self._ode_args(sample, model_output)
        B, L, Cn = sample.shape
        x = sample.clone()
        desc = self._desc()
        rc = N.lib().ffd_ode_step(C.byref(desc), x.data_ptr(), model_output.data_ptr(), G, float(timestep),
                                  float(self.step_size), B, L, Cn, stream)
        N.check(rc, None, "ffd_ode_step")
        return SamplingOutput(prev_sample=x)

    def ode_heun_predict(self, model_output: torch.Tensor, timestep: float, sample: torch.Tensor):
        """Heun's first stage at ``timestep``: (the Euler prediction, the drift there)."""
        sample, model_output, G, stream = self._ode_args(sample, model_output)
        B, L, Cn = sample.shape
        x_pred, drift = torch.empty_like(sample), torch.empty_like(sample)
        desc = self._desc()
        rc = N.lib().ffd_ode_heun_predict(C.byref(desc), sample.data_ptr(), model_output.data_ptr(), G, float(timestep),
                                          float(self.step_size), x_pred.data_ptr(), drift.data_ptr(), B, L, Cn, stream)
        N.check(rc, None, "ffd_ode_heun_predict")
        return x_pred, drift

    def ode_heun_correct(self, model_output_pred: torch.Tensor, timestep_next: float, sample: torch.Tensor,
                         sample_pred: torch.Tensor, drift: torch.Tensor) -> SamplingOutput:
        """Heun's second stage: ``model_output_pred`` is the score at (``sample_pred``, ``timestep_next``), ``sample``
        the state ``ode_heun_predict`` started from."""
        sample, model_output_pred, G, stream = self._ode_args(sample, model_output_pred)
        sample_pred = N.require_gpu_tensor(sample_pred, "sample_pred")
        drift = N.require_gpu_tensor(drift, "drift")
        B, L, Cn = sample.shape
        x = sample.clone()
        desc = self._desc()
        rc = N.lib().ffd_ode_heun_correct(C.byref(desc), x.data_ptr(), sample_pred.data_ptr(), model_output_pred.data_ptr(),
                                          drift.data_ptr(), G, float(timestep_next), float(self.step_size), B, L, Cn,
                                          stream)
        N.check(rc, None, "ffd_ode_heun_correct")
        return SamplingOutput(prev_sample=x)

    # -- linear multistep ODE steps (extension: second order at one model call per interval) ------
    def multistep_coefficients(self, method: str, timestep: float, timestep_next: float,
                               timestep_prev: Optional[float] = None) -> tuple:
        """The five float64 coefficients (qa, qb, cxm1, cn, cp) of ``ode_multistep_step`` for the interval from
        ``timestep`` to ``timestep_next`` (``ffd_host_multistep_coef``; needs no device).  ``timestep_prev=None``: the
        first interval of a trajectory."""
        if method not in MULTISTEP_METHODS:
            raise ValueError(f"method must be one of {sorted(MULTISTEP_METHODS)}, got {method!r}")
        coef = (C.c_double * 5)()
        desc = self._desc()
        have_prev = timestep_prev is not None
        rc = N.lib().ffd_host_multistep_coef(C.byref(desc), MULTISTEP_METHODS[method],
                                             float(timestep_prev) if have_prev else 0.0, float(timestep),
                                             float(timestep_next), float(self.step_size), int(have_prev), coef)
        if rc != 0:
            raise ValueError(f"no {method} coefficients for t_prev={timestep_prev!r}, t={timestep!r}, "
                             f"t_next={timestep_next!r}: the times must decrease strictly, with sigma(t) > 0")
        return tuple(coef)

    def ode_multistep_step(self, model_output: torch.Tensor, timestep: float, timestep_next: float, sample: torch.Tensor,
                           method: str, history: Optional[torch.Tensor] = None, timestep_prev: Optional[float] = None):
        """One interval of a linear multistep solver of the probability-flow ODE, from ``timestep`` to
        ``timestep_next``: ``method="ode_ab2"`` (Adams-Bashforth 2 on the drift of ``ode_step``; uniform grid of width
        ``step_size``) or ``"dpmpp_2m"`` (DPM-Solver++ 2M on the data prediction).  Both reuse the previous interval's
        evaluation: ``history`` is the second value this method returned for the interval from ``timestep_prev`` to
        ``timestep``; without it (a trajectory's first interval) the step is first order.  Returns
        (SamplingOutput, history for the next interval).  No noise is drawn; the inputs are not modified."""
        if method not in MULTISTEP_METHODS:
            raise ValueError(f"method must be one of {sorted(MULTISTEP_METHODS)}, got {method!r}")
        if (history is None) != (timestep_prev is None):
            raise ValueError("history and timestep_prev go together")
        sample, model_output, G, stream = self._ode_args(sample, model_output)
        coef = (C.c_double * 5)(*self.multistep_coefficients(method, timestep, timestep_next, timestep_prev))
        B, L, Cn = sample.shape
        x = sample.clone()
        if history is not None:
            history = N.require_gpu_tensor(history, "history")
            assert history.shape == sample.shape
            hist = history.clone()
        else:
            hist = torch.empty_like(sample)
        rc = N.lib().ffd_ode_multistep_step(x.data_ptr(), model_output.data_ptr(), G, hist.data_ptr(), coef,
                                            int(history is not None), B, L, Cn, stream)
        N.check(rc, None, "ffd_ode_multistep_step")
        return SamplingOutput(prev_sample=x), hist

    # -- Langevin corrector (extension: predictor-corrector sampling) ----------
    def step_correct(self, model_output: torch.Tensor, sample: torch.Tensor, snr: float, timestep: float,
                     noise: Optional[torch.Tensor] = None, norm: str = "batch", *, seed: Optional[int] = None,
                     sample_offset: int = 0, tag: int = 0x80000000, return_step_sizes: bool = False):
        """One Langevin corrector step at ``timestep`` (Song et al. 2021, Algorithms 4 / 5; the argument order of
        ``diffusers``' ``ScoreSdeVeScheduler.step_correct``): x + eps G^2 score + sqrt(2 eps) G z with
        eps = 2 alpha (snr ||G z|| / ||G^2 score||)^2, alpha = 1 (VE) or max(1 - beta(t) step_size, 0) (VP; it needs
        ``timestep``).  ``norm="batch"`` takes both norms as means over the batch (score_sde / diffusers: the step of a
        sample depends on its batch), ``norm="sample"`` per sample (the paper's form; its stationary variance is
        biased by O(1 / (L C))).  ``noise`` injects z; by default z = torch.randn_like(sample) as
        in ``step``; with ``seed`` the draw is made on the device instead (Philox stream ``tag``, global sample index
        ``sample_offset`` + b).  ``return_step_sizes`` adds the (B) tensor of eps to the result."""
        if norm not in ("batch", "sample"):
            raise ValueError(f"norm must be 'batch' or 'sample', got {norm!r}")
        if not snr > 0:
            raise ValueError(f"snr must be > 0, got {snr!r}")
        sample, model_output, G, stream = self._ode_args(sample, model_output)
        B, L, Cn = sample.shape
        if noise is not None:
            z = N.require_gpu_tensor(noise, "noise")
            assert z.shape == sample.shape
        else:
            z = torch.randn_like(sample) if seed is None else None
        x = sample.clone()
        lib = N.lib()
        work = torch.empty(int(lib.ffd_langevin_work_bytes(B, L)) // 8 + 1, device=sample.device, dtype=torch.float64)
        eps = torch.empty(B, device=sample.device, dtype=torch.float32)
        desc = self._desc()
        rc = lib.ffd_langevin_step(C.byref(desc), x.data_ptr(), model_output.data_ptr(), G, float(timestep),
                                   float(self.step_size), float(snr),
                                   N.FFD_LANGEVIN_NORM_BATCH if norm == "batch" else N.FFD_LANGEVIN_NORM_SAMPLE,
                                   z.data_ptr() if z is not None else None, int(seed or 0), int(sample_offset), int(tag),
                                   B, L, Cn, eps.data_ptr(), work.data_ptr(), stream)
        N.check(rc, None, "ffd_langevin_step")
        out = SamplingOutput(prev_sample=x)
        return (out, eps) if return_step_sizes else out

    # -- conditional sampling by replacement (extension: Song et al. 2021, Appendix I.2) --------
    def cond_project(self, sample: torch.Tensor, observed: torch.Tensor, mask: torch.Tensor, timestep: float, *,
                     std: Optional[torch.Tensor] = None, domain: str = "frequency",
                     noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, sample_offset: int = 0,
                     tag: int = 0xC0000000, noiseless: bool = False) -> SamplingOutput:
        """One replacement step at ``timestep``: the observation, noised to the forward SDE's marginal there
        (y_t = mean_coeff observed + sigma G z), is blended into ``sample`` under a time-axis ``mask`` (1 = observed):
        ``domain="frequency"``: x + dft(mask * idft((y_t - x) * std)) / std on packed spectra (``std`` the dataset's
        ``feature_std`` (L, C) or None; its mean cancels); ``domain="time"``: x + mask * (y_t - x).  ``observed`` and
        ``mask`` are (L, C) / (1, L, C) (shared by the batch) or (B, L, C).  ``noise`` injects z; by default
        z = torch.randn_like(sample); with ``seed`` the draw is made on the device (Philox stream ``tag``, global
        sample index ``sample_offset`` + b).  ``noiseless`` blends the observation itself and draws nothing."""
        if domain not in ("frequency", "time"):
            raise ValueError(f"domain must be 'frequency' or 'time', got {domain!r}")
        if domain == "time" and std is not None:
            raise ValueError("std belongs to the frequency domain (the time-domain blend is pointwise)")
        sample = N.require_gpu_tensor(sample, "sample")
        if sample.dim() != 3:
            raise ValueError(f"sample must be (B, L, C), got {tuple(sample.shape)}")
        B, L, Cn = sample.shape
        observed = N.require_gpu_tensor(observed, "observed")
        mask = N.require_gpu_tensor(mask, "mask")
        if observed.dim() == 2:
            observed = observed.unsqueeze(0)
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if tuple(observed.shape) not in ((1, L, Cn), (B, L, Cn)) or mask.shape != observed.shape:
            raise ValueError(f"observed / mask must both be (L, C), (1, L, C) or (B, L, C) of the sample "
                             f"{tuple(sample.shape)}; got {tuple(observed.shape)} and {tuple(mask.shape)}")
        if std is not None:
            std = N.require_gpu_tensor(std, "std")
            if tuple(std.shape) != (L, Cn):
                raise ValueError(f"std must be (L, C) = {(L, Cn)}, got {tuple(std.shape)}")
        z = None
        if not noiseless:
            if noise is not None:
                z = N.require_gpu_tensor(noise, "noise")
                if z.shape != sample.shape:
                    raise ValueError(f"noise must have the sample's shape, got {tuple(z.shape)}")
            elif seed is None:
                z = torch.randn_like(sample)
        x = sample.clone()
        desc = self._desc()
        rc = N.lib().ffd_cond_project(C.byref(desc), x.data_ptr(), observed.data_ptr(), mask.data_ptr(),
                                      std.data_ptr() if std is not None else None, self._G_on(sample.device).data_ptr(),
                                      float(timestep), int(bool(noiseless)), z.data_ptr() if z is not None else None,
                                      int(seed or 0), int(sample_offset), int(tag), int(observed.shape[0]),
                                      N.FFD_COND_FREQUENCY if domain == "frequency" else N.FFD_COND_TIME, B, L, Cn,
                                      N.current_stream_ptr(sample.device))
        N.check(rc, None, "ffd_cond_project")
        return SamplingOutput(prev_sample=x)

    # -- reconstruction guidance (extension; sampling/guidance.py) --------
    def guide_coeffs(self, timestep: float, scale: float = 1.0, obs_var: float = 1e-2, rho: float = 1.0):
        """(alpha, sigma^2, lambda) at ``timestep`` in float64 on the host (``ffd_host_guide_coef``; no device needed):
        the marginal's mean coefficient and variance (without G) and the guidance weight
        lambda = scale / (obs_var + rho sigma^2 / (alpha^2 + sigma^2))."""
        out = (C.c_double * 3)()
        desc = self._desc()
        rc = N.lib().ffd_host_guide_coef(C.byref(desc), float(timestep), float(scale), float(obs_var), float(rho), out)
        N.check(rc, None, "ffd_host_guide_coef")
        return float(out[0]), float(out[1]), float(out[2])

    def denoise(self, score: torch.Tensor, timestep: float, sample: torch.Tensor) -> torch.Tensor:
        """Tweedie's estimate of the clean sample from a score at ``timestep``: x0hat = (x + sigma^2 G_l^2 score) / alpha,
        (B, L, C) on the sample's device: a convenience in plain tensor arithmetic (alpha and sigma^2 from
        ``guide_coeffs`` in float64), not the sampling path -- the guided loop forms the estimate inside ``ffd_guide_seed``,
        whose ``x0hat_out`` has that kernel's own roundings."""
        if sample.dim() != 3 or score.shape != sample.shape:
            raise ValueError(f"score and sample must both be (B, L, C), got {tuple(score.shape)} and {tuple(sample.shape)}")
        alpha, sigma2, _ = self.guide_coeffs(timestep)
        G = self.G.to(device=sample.device, dtype=sample.dtype)
        c = (sigma2 * (G * G)).reshape(1, -1, 1)
        return (sample + c * score) / alpha

    def transition_coeffs(self, timestep_from: float, timestep_to: float):
        """(a, sg) of the forward transition x_t = a x_s + (sg G) z from s = ``timestep_from`` to t = ``timestep_to`` >= s,
        in float64 on the host (``ffd_host_transition_coef``; no device needed)."""
        out = (C.c_double * 2)()
        desc = self._desc()
        rc = N.lib().ffd_host_transition_coef(C.byref(desc), float(timestep_from), float(timestep_to), out)
        N.check(rc, None, "ffd_host_transition_coef")
        return float(out[0]), float(out[1])

    def forward_transition(self, sample: torch.Tensor, timestep_from: float, timestep_to: float,
                           noise: Optional[torch.Tensor] = None, *, seed: Optional[int] = None, sample_offset: int = 0,
                           tag: int = 0xE0000000) -> SamplingOutput:
        """Diffuse ``sample`` (B, L, C), a state at ``timestep_from`` = s, FORWARD to ``timestep_to`` = t >= s with the
        SDE's exact transition kernel: x_t = a x_s + (sg G) z (``transition_coeffs``); the re-noising step of resampled
        conditional sampling (``DiffusionSampler.sample_conditional(resample=...)``).  ``noise`` injects z; by default
        z = torch.randn_like(sample); with ``seed`` the draw is made on the device (Philox stream ``tag``, global sample
        index ``sample_offset`` + b).  s == t returns the sample bit for bit."""
        if not (0.0 <= float(timestep_from) <= float(timestep_to)):
            raise ValueError(f"need 0 <= timestep_from <= timestep_to, got {timestep_from!r}, {timestep_to!r}")
        sample = N.require_gpu_tensor(sample, "sample")
        if sample.dim() != 3:
            raise ValueError(f"sample must be (B, L, C), got {tuple(sample.shape)}")
        B, L, Cn = sample.shape
        z = None
        if noise is not None:
            z = N.require_gpu_tensor(noise, "noise")
            if z.shape != sample.shape:
                raise ValueError(f"noise must have the sample's shape, got {tuple(z.shape)}")
        elif seed is None:
            z = torch.randn_like(sample)
        x = sample.clone()
        desc = self._desc()
        rc = N.lib().ffd_forward_transition(C.byref(desc), x.data_ptr(), self._G_on(sample.device).data_ptr(),
                                            float(timestep_from), float(timestep_to), z.data_ptr() if z is not None else None,
                                            int(seed or 0), int(sample_offset), int(tag), B, L, Cn,
                                            N.current_stream_ptr(sample.device))
        N.check(rc, None, "ffd_forward_transition")
        return SamplingOutput(prev_sample=x)


class VEScheduler(SDE):
    """sde.py:90-165."""

    _sde_kind = N.FFD_SDE_VE

    def __init__(self, sigma_min: float = 0.01, sigma_max: float = 50.0, fourier_noise_scaling: bool = False,
                 eps: float = 1e-5):
        super().__init__(fourier_noise_scaling=fourier_noise_scaling, eps=eps)
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max

    def _sde_ab(self):
        return self.sigma_min, self.sigma_max

    def _prior_scale(self) -> float:
        return float(self.sigma_max)

    def marginal_prob(self, x: torch.Tensor, t: torch.Tensor):
        """sde.py:106-123 (training-side; plain tensor arithmetic)."""
        if self.G is None:
            self.set_noise_scaling(x.shape[1])
        sigma_min = torch.tensor(self.sigma_min).type_as(t)
        sigma_max = torch.tensor(self.sigma_max).type_as(t)
        std = (sigma_min * (sigma_max / sigma_min) ** t).view(-1, 1) * self.G.to(x.device)
        return x, std

    def marginal_coeffs(self, t: torch.Tensor):
        sigma_min = torch.tensor(self.sigma_min).type_as(t)
        sigma_max = torch.tensor(self.sigma_max).type_as(t)
        return torch.ones_like(t), sigma_min * (sigma_max / sigma_min) ** t


class VPScheduler(SDE):
    """sde.py:168-246."""

    _sde_kind = N.FFD_SDE_VP

    def __init__(self, beta_min: float = 0.1, beta_max: float = 20.0, fourier_noise_scaling: bool = False,
                 eps: float = 1e-5):
        super().__init__(fourier_noise_scaling=fourier_noise_scaling, eps=eps)
        self.beta_0 = beta_min
        self.beta_1 = beta_max

    def _sde_ab(self):
        return self.beta_0, self.beta_1

    def get_beta(self, timestep: float) -> float:
        return self.beta_0 + timestep * (self.beta_1 - self.beta_0)

    def marginal_prob(self, x: torch.Tensor, t: torch.Tensor):
        """sde.py:186-210 (training-side; plain tensor arithmetic)."""
        if self.G is None:
            self.set_noise_scaling(x.shape[1])
        log_mean_coeff = -0.25 * t ** 2 * (self.beta_1 - self.beta_0) - 0.5 * t * self.beta_0
        mean = torch.exp(log_mean_coeff[(...,) + (None,) * len(x.shape[1:])]) * x
        std = torch.sqrt((1.0 - torch.exp(2.0 * log_mean_coeff.view(-1, 1)))) * self.G.to(x.device)
        return mean, std

    def marginal_coeffs(self, t: torch.Tensor):
        log_mean_coeff = -0.25 * t ** 2 * (self.beta_1 - self.beta_0) - 0.5 * t * self.beta_0
        return torch.exp(log_mean_coeff), torch.sqrt(1.0 - torch.exp(2.0 * log_mean_coeff))
