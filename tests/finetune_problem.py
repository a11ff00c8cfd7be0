"""The seeded fine-tuning problems that tests/test_online_finetune_host.py and tests/test_gpu_online_finetune.py share (a
helper, not a test module)."""
import numpy as np

from contrastiveprosthetics_amd.finetune import round_bf16


def synthetic_problem(n: int, k: int, seed: int = 0, bf16: bool = False) -> dict:
    """n windows and k classes: u (n, 512) non-negative like an fc7 activation, with a pattern per class and noise on top (as
    stored: rounded to bf16 on request, else float32 values), W, b, E (float32 values) and slots over the classes 0..k-2, so
    that class k-1 has no window when k > 1.  All float64 arrays but slots (int32)."""
    rng = np.random.default_rng([seed, n, k])
    slots = (rng.integers(0, max(k - 1, 1), size=n)).astype(np.int32)
    pattern = rng.standard_normal((k, 512))
    u = np.maximum(pattern[slots] + 0.7 * rng.standard_normal((n, 512)), 0.0).astype(np.float32)
    u = round_bf16(u) if bf16 else u.astype(np.float64)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    return dict(u=u, W=f32(0.05 * rng.standard_normal((16, 512))), b=f32(0.1 * rng.standard_normal(16)),
                E=f32(rng.standard_normal((k, 16))), slots=slots)
