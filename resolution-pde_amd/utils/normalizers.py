"""What the rollout (utils/autoregressive_step.py) and the equation-residual objective (rpde/entry.py) both ask of a data
set's normaliser."""
from __future__ import annotations


def scalar_stats(norm):
    """(mean, std + eps) when the normaliser is one global affine map (SimpleNormalizer), else None"""
    try:
        m, s, e = norm.mean, norm.std, getattr(norm, "eps", 0.0)
        if isinstance(m, (int, float)) and isinstance(s, (int, float)):
            return float(m), float(s) + float(e)
    except AttributeError:
        pass
    return None
