"""Host-side LCMScheduler tables for the HIP path (the per-step arithmetic itself is the
``lcm_scheduler_step`` kernel).  Mirrors ``LCMScheduler.from_config`` / ``set_timesteps`` as used at
backends/cuda_worker.py:88 and backends/rknnlcm.py:559-560; values in a checkpoint's
``scheduler/scheduler_config.json`` (backends/base.py:45-46) override the defaults.  SURVEY.md A.3.
"""
from __future__ import annotations

import json
import os

import numpy as np


PREDICTION_TYPES = ("epsilon", "v_prediction", "sample")

# scheduler_config.json of SD 2.1-768 (v-prediction; set_alpha_to_one never matters to LCM: its last step uses its own t)
SD21_768_SCHEDULE = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                         set_alpha_to_one=False, prediction_type="v_prediction")


class LCMSchedule:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 original_inference_steps=50, timestep_scaling=10.0, sigma_data=0.5, set_alpha_to_one=True,
                 prediction_type="epsilon", **_ignored):
        if beta_schedule != "scaled_linear":
            raise ValueError(f"unsupported beta_schedule {beta_schedule!r}")
        # what the UNet predicts (LCMScheduler.step): epsilon (SD1.5, SD 2.x-base), v_prediction (SD 2.x-768), sample
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"unsupported prediction_type {prediction_type!r}: expected one of {', '.join(PREDICTION_TYPES)}")
        self.prediction_type = prediction_type
        self.num_train_timesteps = int(num_train_timesteps)
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, self.num_train_timesteps, dtype=np.float32) ** 2
        self.alphas_cumprod = np.cumprod((1.0 - betas).astype(np.float32), dtype=np.float32)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.original_inference_steps = int(original_inference_steps)
        self.timestep_scaling = float(timestep_scaling)
        self.sigma_data = float(sigma_data)
        self.init_noise_sigma = 1.0

    @classmethod
    def from_config_file(cls, path: str):
        if not os.path.exists(path):
            return cls()
        with open(path) as f:
            cfg = json.load(f)
        keys = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "original_inference_steps",
                "timestep_scaling", "sigma_data", "set_alpha_to_one", "prediction_type")
        return cls(**{k: cfg[k] for k in keys if k in cfg})

    def timesteps(self, n: int, strength: float = 1.0) -> np.ndarray:
        """``LCMScheduler.set_timesteps(n, strength=strength)``: the LCM training schedule cut to its last
        ``int(original_inference_steps * strength)`` timesteps, ``n`` of them taken at even spacing.  strength 1.0 is the
        text-to-image schedule."""
        if n < 1:
            raise ValueError("num_inference_steps must be >= 1")
        k = self.num_train_timesteps // self.original_inference_steps
        if strength == 1.0:
            origin = (np.arange(1, self.original_inference_steps + 1) * k - 1)[::-1].copy()
            if n > len(origin):
                raise ValueError(f"num_inference_steps={n} exceeds original_inference_steps={len(origin)}")
        else:
            m = int(self.original_inference_steps * float(strength))
            origin = (np.arange(1, m + 1) * k - 1)[::-1].copy()
            if n > m:
                raise ValueError(f"The combined original_steps x strength: {m} is smaller than num_inference_steps: {n}. Make sure "
                                 f"to either reduce num_inference_steps to a value smaller than {m} or increase strength to a "
                                 f"value higher than {float(n) / self.original_inference_steps}.")
        idx = np.floor(np.linspace(0, len(origin), num=n, endpoint=False)).astype(np.int64)
        return origin[idx].astype(np.int64)

    def renoise_coefficients(self, t: int):
        """-> (sqrt(alphas_cumprod[t]), sqrt(1 - alphas_cumprod[t])): ``add_noise`` at timestep t (a refinement pass's start)."""
        a_t = float(self.alphas_cumprod[int(t)])
        return a_t ** 0.5, (1 - a_t) ** 0.5

    def step_coefficients(self, ts: np.ndarray, i: int):
        """-> ([sqrt_a_t, sqrt_b_t, c_skip, c_out, sqrt_a_prev, sqrt_b_prev], last)."""
        t = int(ts[i])
        last = i == len(ts) - 1
        tp = t if last else int(ts[i + 1])
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[tp]) if tp >= 0 else self.final_alpha_cumprod
        s = t * self.timestep_scaling
        c_skip = self.sigma_data ** 2 / (s ** 2 + self.sigma_data ** 2)
        c_out = s / (s ** 2 + self.sigma_data ** 2) ** 0.5
        return [a_t ** 0.5, (1 - a_t) ** 0.5, c_skip, c_out, a_p ** 0.5, (1 - a_p) ** 0.5], last
