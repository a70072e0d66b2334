from .vit import (FactorisedLinear, MixerBlock, MultiLayerPredictor, TokenAggregator, TransformerSeqEncoder,  # noqa: F401
                  VisionTransformer, VisionTransformer1D)
