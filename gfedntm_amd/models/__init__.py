from .networks import (DecoderNetwork, CTMDecoderNetwork, InferenceNetwork,
                       CombinedInferenceNetwork, ContextualInferenceNetwork)
from .avitm import AVITM
from .ctm import CTM, ZeroShotTM, CombinedTM
from .gibbs_lda import GibbsLDA

__all__ = ["DecoderNetwork", "CTMDecoderNetwork", "InferenceNetwork",
           "CombinedInferenceNetwork", "ContextualInferenceNetwork", "AVITM", "CTM",
           "ZeroShotTM", "CombinedTM", "GibbsLDA"]
