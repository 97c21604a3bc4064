"""``fdiff.visualization.spectral_interpretation`` mirror: the per-dataset statistics of ``process_dataset``
(reference spectral_interpretation.py:34-148) without pandas and without the plots.

``spectral_profile`` returns the four curves as tensors (ffd_spectral_profile: fixed-order fp64 batch reductions on the
device); ``process_dataset`` returns the reference's four tables as lists of records with its column names, so that
``pd.DataFrame(records)`` is the frame the reference returns.
"""
from __future__ import annotations

import torch

from .. import _native as N
from ..utils.fourier import _on_gpu, _work, localization_metrics


def spectral_profile(X: torch.Tensor):
    """``(spec_mean, spec_se, energy_mean, energy_std)`` of X (B, L, C), spectral_interpretation.py:55-94: the batch mean
    of the normalized spectral density over the ceil((L+1)/2) bins and its std / sqrt(B) (:58-68); the batch mean of the
    normalized energy over time and its plain std, which is what the reference's temporal "SE" column holds (:85-94).
    EPS = 1e-15 enters the denominators of the means only; the std is unbiased (NaN for B = 1)."""
    assert X.dim() == 3, f"expected (batch_size, max_len, n_channels), got {tuple(X.shape)}"
    src_device = X.device
    xd = _on_gpu(X, "spectral_profile")
    B, L, Cn = xd.shape
    nf = L // 2 + 1
    spec = torch.empty((2, nf), device=xd.device, dtype=torch.float32)
    energy = torch.empty((2, L), device=xd.device, dtype=torch.float32)
    work = _work(N.lib().ffd_spectral_profile_work_bytes(B, L, Cn), xd.device)
    rc = N.lib().ffd_spectral_profile(xd.data_ptr(), spec[0].data_ptr(), spec[1].data_ptr(), energy[0].data_ptr(),
                                      energy[1].data_ptr(), work.data_ptr(), work.numel() * 8, B, L, Cn,
                                      N.current_stream_ptr(xd.device))
    N.check(rc, None, "ffd_spectral_profile")
    if src_device.type != "cuda":
        spec, energy = spec.to(src_device), energy.to(src_device)
    return spec[0], spec[1], energy[0], energy[1]


def process_dataset(dataset_name: str, datamodule):
    """spectral_interpretation.py:34-148 for a datamodule (anything with ``X_train``; ``prepare_data`` / ``setup`` are
    called when present, :48-49) or for the training tensor itself.  Returns the record lists of
    ``(spectral_df, temporal_df, localization_df, localization_joint_df)``."""
    if isinstance(datamodule, torch.Tensor):
        X_train = datamodule
    else:
        for hook in ("prepare_data", "setup"):
            if callable(getattr(datamodule, hook, None)):
                getattr(datamodule, hook)()
        X_train = datamodule.X_train
    spec_mean, spec_se, energy_mean, energy_std = (t.cpu().tolist() for t in spectral_profile(X_train))
    X_loc, X_spec_loc = (t.cpu().tolist() for t in localization_metrics(X_train))
    nf, L = len(spec_mean), len(energy_mean)
    freq_norm = [k / (nf - 1) for k in range(nf)]  # :71 (a single bin divides by zero there too)
    time_norm = [k / (L - 1) for k in range(L)]    # :97
    spectral = [{"Dataset": dataset_name, "Normalized Frequency": freq_norm[k],
                 "Normalized Spectral Density": spec_mean[k], "SE": spec_se[k]} for k in range(nf)]
    temporal = [{"Dataset": dataset_name, "Normalized Time": time_norm[k], "Normalized Energy": energy_mean[k],
                 "SE": energy_std[k]} for k in range(L)]
    localization = [{"Dataset": dataset_name, "Delocalization": v, "Domain": "Time"} for v in X_loc]
    localization += [{"Dataset": dataset_name, "Delocalization": v, "Domain": "Frequency"} for v in X_spec_loc]
    joint = [{"Dataset": dataset_name, "Delocalization Time": a, "Delocalization Frequency": b}
             for a, b in zip(X_loc, X_spec_loc)]
    return spectral, temporal, localization, joint
