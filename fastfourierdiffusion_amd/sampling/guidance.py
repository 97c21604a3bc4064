"""Reconstruction guidance for ``DiffusionSampler.sample_conditional`` / ``impute`` (extension: Ho et al. 2022, Chung et
al. 2023 "DPS", Kollovieh et al. 2023 "observation self-guidance"; include/ffd.h ``ffd_sample_batch_guided``).

Replacement conditioning draws the observed part of the state independently of the unobserved part; guidance steers the
WHOLE state instead.  At every reverse step the score s is replaced by

    s~ = s - lambda(t) grad_x 1/2 |mask (x0hat(x) - observed)|^2,    x0hat = (x + sigma^2 G^2 s) / alpha   (Tweedie)
    lambda(t) = scale / (obs_var + rho sigma^2 / (alpha^2 + sigma^2))

and the gradient goes through the score model (its input vector-Jacobian product: closed form for the mixture, the
training backward without weight gradients for the transformer and the MLP).
"""
from __future__ import annotations

import math
from dataclasses import dataclass


@dataclass(frozen=True)
class Guidance:
    """``scale``: overall strength (0 switches guidance off: the unguided trajectory).  ``obs_var``: the observation
    noise variance, IN THE UNITS OF THE DIFFUSED DOMAIN (for a spectral model: of the packed, standardized spectrum's
    time-axis image).  At small t the step is multiplied by lambda ~ scale / obs_var: too small a value overshoots the
    observation and the trajectory oscillates; the data's own bandwidth squared is the natural size.  ``rho``: weight of
    the denoiser's own uncertainty sigma^2 / (alpha^2 + sigma^2), which keeps lambda bounded by scale / rho early on.
    ``replace``: also project onto the noised observation after every step (replacement on top of guidance)."""
    scale: float = 1.0
    obs_var: float = 1e-2
    rho: float = 1.0
    replace: bool = False

    def __post_init__(self) -> None:
        for name in ("scale", "obs_var", "rho"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        if self.obs_var == 0 and self.rho == 0:
            raise ValueError("obs_var and rho cannot both be 0: lambda(t) would have a zero denominator")
