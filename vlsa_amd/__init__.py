"""vlsa_amd -- MI355X-native (gfx950) language-guided patch aggregation for VLSA.

Host side mirrors the reference's model interface (VLFAN / FeatMIL / DeepMIL / VLSA); the arithmetic lives
in hand-written HIP kernels behind the C ABI of include/vlsa_hip.h.  There is no CPU fallback.
"""
from ._native import VlsaNativeError  # noqa: F401

__all__ = ["VlsaNativeError", "DeepAttnMISL", "ILRA", "SurvEvaluator", "CoxSurvEvaluator", "RegSurvEvaluator", "concordance_index_censored", "concordance_counts",
           "SurvIFMLE", "SurvMLE", "SurvEMD", "SurvT2I", "SurvObjective", "SurvPLE", "rank_loss", "recon_loss", "MSE_loss", "SurvPairObjective"]


def __getattr__(name):
    if name == "DeepAttnMISL":          # imported on first use: the package itself needs no torch
        from .deepmil import DeepAttnMISL
        return DeepAttnMISL
    if name == "ILRA":
        from .deepmil import ILRA
        return ILRA
    if name in ("SurvEvaluator", "CoxSurvEvaluator", "RegSurvEvaluator", "concordance_index_censored", "concordance_counts"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("SurvIFMLE", "SurvMLE", "SurvEMD", "SurvT2I", "SurvObjective", "SurvPLE", "rank_loss", "recon_loss", "MSE_loss", "SurvPairObjective"):
        from . import losses
        return getattr(losses, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
