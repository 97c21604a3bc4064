"""ctypes binding of libffd.so (the C ABI declared in include/ffd.h).

The shared library is built in-tree by ``fastfourierdiffusion_amd.build`` (hipcc,
gfx950 only) and lives next to this file.  There is no CPU or PyTorch fallback: if
the library is missing or no gfx950 device is usable, every compute entry point
raises ``FFDError`` loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libffd.so")

FFD_MODEL_TRANSFORMER, FFD_MODEL_LSTM, FFD_MODEL_MLP = 0, 1, 2
FFD_MODEL_MIXTURE = 3  # the closed-form Gaussian-mixture score (dim_feedforward carries K)
FFD_SDE_VP, FFD_SDE_VE = 0, 1
FFD_SOLVER_EULER_MARUYAMA, FFD_SOLVER_ODE_EULER, FFD_SOLVER_ODE_HEUN, FFD_SOLVER_PC = 0, 1, 2, 3
FFD_SOLVER_ODE_AB2, FFD_SOLVER_DPMPP_2M = 4, 5
FFD_LANGEVIN_NORM_BATCH, FFD_LANGEVIN_NORM_SAMPLE = 0, 1
FFD_COND_FREQUENCY, FFD_COND_TIME = 0, 1
FFD_LOGLIK_EULER, FFD_LOGLIK_PREDICT, FFD_LOGLIK_CORRECT = 0, 1, 2
# kernel classes (include/ffd.h FFD_K_*)
K_FFN, K_ATTN, K_OUTPROJ, K_LSTM_REC, K_LSTM_GATES, K_SDE, K_EMBED, K_UNEMBED = range(8)


class FFDError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_channels", C.c_int32), ("max_len", C.c_int32), ("d_model", C.c_int32),
        ("n_head", C.c_int32), ("num_layers", C.c_int32), ("dim_feedforward", C.c_int32), ("sde", C.c_int32),
        ("sde_a", C.c_double), ("sde_b", C.c_double), ("fourier_noise_scaling", C.c_int32), ("eps", C.c_double),
    ]


class SdeDesc(C.Structure):
    _fields_ = [("sde", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


class FrescaCfg(C.Structure):
    _fields_ = [("low_scale", C.c_float), ("high_scale", C.c_float), ("cutoff_ratio", C.c_double),
                ("strategy", C.c_int32), ("num_steps", C.c_int32)]


class CrfCaptureCfg(C.Structure):
    _fields_ = [("ring", C.c_void_p), ("n_slots", C.c_int32), ("every", C.c_int32), ("last", C.c_void_p),
                ("last_every", C.c_int32), ("reserved", C.c_int32)]


class CondCfg(C.Structure):
    """ffd_cond_cfg: the observation of ffd_sample_batch_cond (device pointers; std None or (L, C))."""
    _fields_ = [("obs", C.c_void_p), ("mask", C.c_void_p), ("std", C.c_void_p), ("obs_batch", C.c_int32),
                ("domain", C.c_int32), ("final_replace", C.c_int32), ("reserved", C.c_int32)]


class GuideCfg(C.Structure):
    """ffd_guide_cfg: lambda(t) = scale / (obs_var + rho sigma^2 / (alpha^2 + sigma^2)) of ffd_sample_batch_guided."""
    _fields_ = [("scale", C.c_double), ("obs_var", C.c_double), ("rho", C.c_double), ("replace", C.c_int32),
                ("reserved", C.c_int32)]


class ClassCfg(C.Structure):
    """ffd_class_cfg: the table (device, read live), the device labels with their host copy (both None: every sample
    null), and the classifier-free guidance scale g of s_u + g (s_c - s_u)."""
    _fields_ = [("table", C.c_void_p), ("labels", C.c_void_p), ("labels_host", C.c_void_p), ("n_classes", C.c_int32),
                ("n_labels", C.c_int32), ("guidance_scale", C.c_float), ("reserved", C.c_int32)]


class CacheCfg(C.Structure):
    _fields_ = [("K", C.c_int32), ("R", C.c_int32)]


class PartitionHalf(C.Structure):
    """ffd_partition_half: one plan of ffd_partition_plan (a half for half the CUs, or the whole batch)."""
    _fields_ = [("nb", C.c_int), ("nw", C.c_int), ("cps", C.c_int), ("mb", C.c_int), ("persist", C.c_int), ("hpw", C.c_int),
                ("qg", C.c_int), ("kspl", C.c_int), ("ffn_tiles", C.c_int), ("ffn_grid", C.c_int), ("one_per_tile", C.c_int),
                ("part_floats", C.c_longlong), ("ffn", C.c_char * 64), ("attn", C.c_char * 48)]


class PartitionInfo(C.Structure):
    _fields_ = [("parts", C.c_int), ("cu_budget", C.c_int), ("halves_planned", C.c_int), ("whole_planned", C.c_int),
                ("half", PartitionHalf * 2), ("whole", PartitionHalf)]


class CacheStats(C.Structure):
    _fields_ = [("recompute_count", C.c_int64), ("cache_hit_count", C.c_int64), ("current_step", C.c_int64),
                ("table_allocated", C.c_int32), ("reserved", C.c_int32)]


class AdamWCfg(C.Structure):
    """ffd_adamw_cfg: one AdamW step's scalars (step counts from 1)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("max_norm", C.c_double), ("step", C.c_longlong)]


_P = C.c_void_p
_F = C.POINTER(C.c_float)
# how every ffd_sample_batch* entry begins: ctx, x, B, timesteps, n_steps, step_size, first, n_run
_LOOP = [_P, _P, C.c_int, _F, C.c_int, C.c_float, C.c_int, C.c_int]

# name -> (restype, argtypes); must list every symbol include/ffd.h declares
SIGNATURES = {
    "ffd_freq_decompose": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P]),
    "ffd_hermite_predict": (C.c_int, [_P, C.POINTER(C.c_double), C.c_double, C.c_int, _P, C.c_int, C.c_size_t, _P]),
    "ffd_spectral_density": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_localization_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_localization": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_smooth_frequency_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_smooth_frequency": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_double, _P]),
    "ffd_spectral_profile_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_spectral_profile": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_localization_lds_max_len": (C.c_int, []),
    "ffd_localization_bench": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F,
                                         _P]),
    "ffd_w2_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "ffd_w2_sliced": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_w2_marginal": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_w2_prepare": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_w2_against_prepared": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P,
                                          C.c_size_t, _P]),
    "ffd_w2_summary": (C.c_int, [_P, C.c_int, _P, _P]),
    "ffd_col_mean_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_col_mean": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_w2_bench_kernels": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, _F, _P]),
    "ffd_ens_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "ffd_ens_pointwise": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int,
                                    _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "ffd_ens_energy": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_ens_bench_energy": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, C.c_int,
                                       _F, _P]),
    "ffd_nn_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "ffd_nn_search": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "ffd_nn_ball_count": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_nn_radius": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ffd_nn_scores": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ffd_mmd_centre_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_mmd_centre": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_mmd_bandwidth_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_mmd_bandwidth": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_mmd_rowsums_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ffd_mmd_rowsums": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_mmd_scores": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "ffd_mmd_gram_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_mmd_gram": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_size_t, _P]),
    "ffd_mmd_permute_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_mmd_permute": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_sinkhorn_softmin_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_sinkhorn_softmin": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_double, _P, _P, _P, C.c_size_t, _P]),
    "ffd_sinkhorn_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_sinkhorn": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "ffd_sinkhorn_diameter2_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_sinkhorn_diameter2": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "ffd_host_sinkhorn_schedule": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int, _P, C.c_int]),
    "ffd_cov_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_cov": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "ffd_sym_eig_work_bytes": (C.c_size_t, [C.c_int]),
    "ffd_sym_eig": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "ffd_sym_root_work_bytes": (C.c_size_t, [C.c_int]),
    "ffd_sym_root": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_frechet_work_bytes": (C.c_size_t, [C.c_int]),
    "ffd_frechet": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "ffd_pca_variances_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_pca_variances": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "ffd_pca_transform": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "ffd_dtw_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "ffd_dtw_search": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t,
                                 _P]),
    "ffd_dtw_pairs": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ffd_dtw_scores": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "ffd_sm_draw_times":(C.c_int, [_P, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, _P]),
    "ffd_sm_perturb": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_sm_loss": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_sm_eval_batch": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, _P, C.c_int, _P]),
    "ffd_dense_dgrad": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_dense_wgrad_chunks": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "ffd_dense_wgrad_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ffd_dense_wgrad": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ffd_sm_loss_grad": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint64, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                   _P]),
    "ffd_sm_draw_times_at": (C.c_int, [_P, _P, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, _P]),
    "ffd_layernorm_stats_fwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_double, _P]),
    "ffd_layernorm_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "ffd_attention_lse_fwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_attention_bwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_adamw": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, C.POINTER(AdamWCfg), _P]),
    "ffd_host_lr_schedule": (C.c_double, [C.c_double, C.c_longlong, C.c_longlong, C.c_longlong]),
    "ffd_train_create": (C.c_int, [C.POINTER(_P), C.POINTER(ModelDesc), C.c_double, C.c_int]),
    "ffd_train_destroy": (None, [_P]),
    "ffd_train_last_error": (C.c_char_p, [_P]),
    "ffd_train_work_bytes": (C.c_size_t, [C.POINTER(ModelDesc), C.c_int]),
    "ffd_train_bind": (C.c_int, [_P, C.c_char_p, _P, _P, _P, _P, C.c_size_t]),
    "ffd_train_forward": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "ffd_train_bind_params": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    "ffd_train_input_vjp": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "ffd_train_loss_grad": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, _P, C.c_int, _P]),
    "ffd_train_grad_sqnorm": (C.c_int, [_P, _P, _P]),
    "ffd_train_adamw": (C.c_int, [_P, _P, C.POINTER(AdamWCfg), _P]),
    "ffd_train_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, _P, C.c_int,
                                 C.POINTER(AdamWCfg), _P]),
    "ffd_cache_crf_capture": (C.c_int, [_P, C.POINTER(CrfCaptureCfg)]),
    "ffd_create": (C.c_int, [C.POINTER(_P), C.POINTER(ModelDesc), C.c_int]),
    "ffd_destroy": (None, [_P]),
    "ffd_last_error": (C.c_char_p, [_P]),
    "ffd_version": (C.c_char_p, []),
    "ffd_load_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    "ffd_finalize_weights": (C.c_int, [_P]),
    "ffd_host_noise_scaling": (C.c_int, [C.c_int, C.c_int, _F]),
    "ffd_host_timesteps": (C.c_int, [C.c_int, C.c_double, _F, _F]),
    "ffd_host_gate": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ffd_host_attn_score_bound": (C.c_int, [_F, _F, _F, _F, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "ffd_score_forward": (C.c_int, [_P, _P, C.c_float, _P, C.c_int, _P]),
    "ffd_score_forward_cached": (C.c_int, [_P, _P, C.c_float, _P, _P, C.c_int, C.c_int, _P]),
    "ffd_sde_step": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, C.c_double, C.c_float, _P, C.c_uint64, C.c_uint64,
                               C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_ode_step": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, C.c_double, C.c_float, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_ode_heun_predict": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, C.c_double, C.c_float, _P, _P, C.c_int, C.c_int,
                                       C.c_int, _P]),
    "ffd_ode_heun_correct": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, _P, _P, C.c_double, C.c_float, C.c_int, C.c_int,
                                       C.c_int, _P]),
    "ffd_host_multistep_coef": (C.c_int, [C.POINTER(SdeDesc), C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_int, C.POINTER(C.c_double)]),
    "ffd_ode_multistep_step": (C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_langevin_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ffd_langevin_step": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, C.c_double, C.c_float, C.c_float, C.c_int, _P,
                                    C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "ffd_cond_project": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, _P, _P, C.c_double, C.c_int, _P, C.c_uint64, C.c_uint64,
                                   C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_host_transition_coef": (C.c_int, [C.POINTER(SdeDesc), C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "ffd_forward_transition": (C.c_int, [C.POINTER(SdeDesc), _P, _P, C.c_double, C.c_double, _P, C.c_uint64, C.c_uint64,
                                         C.c_uint32, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_mixture_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ffd_mixture_score": (C.c_int, [C.POINTER(SdeDesc), _P, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int,
                                    C.c_int, _P, C.c_size_t, _P]),
    "ffd_host_mixture_check": (C.c_int, [_F, _F, _F, C.c_int, C.c_int, C.c_int]),
    "ffd_mixture_vjp_work_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ffd_mixture_score_vjp": (C.c_int, [C.POINTER(SdeDesc), _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int,
                                        C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "ffd_guide_seed": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, _P, _P, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, _P, _P, _P, _P, _P]),
    "ffd_guide_combine": (C.c_int, [_P, _P, _P, C.c_float, C.c_float, _P, C.c_size_t, _P]),
    "ffd_host_guide_coef": (C.c_int, [C.POINTER(SdeDesc), C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.POINTER(C.c_double)]),
    "ffd_mixture_tiling": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ffd_prior": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_host_loglik_h": (C.c_int, [C.POINTER(SdeDesc), C.c_double, C.c_double, _F]),
    "ffd_prior_logp": (C.c_int, [C.POINTER(SdeDesc), _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_loglik_perturb": (C.c_int, [_P, _P, C.c_float, C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P, C.c_int,
                                     C.c_int, C.c_int, _P]),
    "ffd_loglik_tail": (C.c_int, [C.POINTER(SdeDesc), C.c_int, _P, _P, _P, _P, _P, C.c_double, C.c_double, C.c_float,
                                  C.c_int, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P, _P, _P, C.c_int, C.c_int, C.c_int,
                                  _P]),
    "ffd_loglik_batch": (C.c_int, [_P, _P, _P, C.c_int, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _P,
                                   C.c_uint64, C.c_uint64, _P]),
    "ffd_dft": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_idft": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_unstandardize_idft": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_dft_standardize": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_positional_encoding": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "ffd_time_encoding": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ffd_fresca": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double, C.c_int, _P]),
    "ffd_lstm_trace": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    "ffd_fresca2d": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double, C.c_int, _P]),
    "ffd_fresca_enable": (C.c_int, [_P, C.POINTER(FrescaCfg)]),
    "ffd_fresca_disable": (C.c_int, [_P]),
    "ffd_cache_enable": (C.c_int, [_P, C.POINTER(CacheCfg)]),
    "ffd_cache_disable": (C.c_int, [_P]),
    "ffd_cache_reset": (C.c_int, [_P]),
    "ffd_cache_stats_get": (C.c_int, [_P, C.POINTER(CacheStats)]),
    "ffd_cache_tables_read": (C.c_int, [_P, _P, _P, _P]),
    "ffd_sample_batch": (C.c_int, _LOOP + [C.c_uint64, C.c_uint64, _P, C.c_int, C.c_int, _P]),
    "ffd_sample_batch_ode": (C.c_int, _LOOP + [C.c_int, C.c_int, C.c_int, _P]),
    "ffd_sample_batch_pc": (C.c_int, _LOOP + [C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint64, _P, C.c_int, C.c_int, _P]),
    "ffd_sample_batch_cond": (C.c_int, _LOOP + [C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint64, _P, C.c_int, C.c_int,
                                                C.POINTER(CondCfg), _P]),
    "ffd_host_resample_visits": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "ffd_host_resample_visit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ffd_sample_batch_resample": (C.c_int, _LOOP + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint64, _P,
                                                    C.POINTER(CondCfg), _P]),
    "ffd_sample_batch_guided": (C.c_int, [_P, _P, _P, C.c_int, _F, C.c_int, C.c_float, C.c_int, C.c_int, C.c_uint64,
                                          C.c_uint64, _P, C.POINTER(CondCfg), C.POINTER(GuideCfg), _P, _P]),
    "ffd_class_enable": (C.c_int, [_P, C.POINTER(ClassCfg)]),
    "ffd_class_disable": (C.c_int, [_P]),
    "ffd_class_temb": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ffd_cfg_combine": (C.c_int, [_P, _P, C.c_float, C.c_size_t, _P]),
    "ffd_class_drop": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_uint64, C.c_uint64, _P, _P]),
    "ffd_class_table_grad": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ffd_train_classes": (C.c_int, [_P, C.c_int]),
    "ffd_train_labels": (C.c_int, [_P, _P, C.c_size_t, C.c_double]),
    "ffd_flops_per_sample_step": (C.c_double, [_P, C.c_int]),
    "ffd_ffn_flops_per_launch": (C.c_double, [_P, C.c_int]),
    "ffd_kernel_timing_begin": (C.c_int, [_P, C.c_uint32, C.c_int]),
    "ffd_kernel_timing_end": (C.c_int, [_P]),
    "ffd_kernel_timing_get": (C.c_int, [_P, C.c_int, _F, C.POINTER(C.c_int)]),
    "ffd_host_cu_masks": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    "ffd_partition_status": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "ffd_partition_plan": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(PartitionInfo)]),
    "ffd_kernel_work": (C.c_char_p, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ffd_score_forward_ts": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "ffd_cache_configure": (C.c_int, [_P, C.POINTER(CacheCfg)]),
    "ffd_tune": (C.c_int, [C.c_char_p, C.c_int]),
    "ffd_tune_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "ffd_bench_ffn": (C.c_int, [_P, C.c_int, C.c_int, _F, _P]),
    "ffd_probe_ffn_clock": (C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int), _P]),
    "ffd_async_status": (C.c_int, [_P]),
    "ffd_probe_attn": (C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_int, _F, C.POINTER(C.c_uint64), C.c_int,
                                 C.POINTER(C.c_int), _P]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libffd.so (once).  torch is imported first so that the HIP runtime already
    mapped by PyTorch-ROCm (same SONAME, libamdhip64.so.7) is the one libffd binds to --
    streams and device pointers are then shared with torch tensors."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FFDError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C fastfourierdiffusion_amd/csrc`). There is no CPU / PyTorch fallback.")
    try:
        import torch  # noqa: F401  (maps torch's bundled HIP runtime first)
    except Exception:  # pragma: no cover - torch is optional for the pure C ABI
        pass
    try:
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise FFDError(f"failed to load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise FFDError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return handle


def check(rc: int, ctx=None, what: str = "") -> None:
    if rc == 0:
        return
    msg = ""
    if ctx:
        raw = lib().ffd_last_error(ctx)
        msg = raw.decode() if raw else ""
    exc = {-1: AssertionError, -2: NotImplementedError}.get(rc, FFDError)
    raise exc(f"libffd {what} failed (status {rc}): {msg}")


def current_stream_ptr(device) -> int:
    import torch

    return int(torch.cuda.current_stream(device).cuda_stream)


def require_gpu_tensor(t, name: str = "tensor"):
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise FFDError(
            f"{name} lives on {t.device}: fastfourierdiffusion_amd computes only on an MI355X (gfx950) device; "
            "move the model/tensors to cuda (there is no CPU fallback).")
    if t.dtype != torch.float32:
        raise AssertionError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()
