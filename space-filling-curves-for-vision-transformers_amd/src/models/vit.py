from sfcvit.models.vit import (FactorisedLinear, MixerBlock, MultiLayerPredictor, PooledHead, TokenAggregator, TransformerSeqEncoder,  # noqa: F401
                               VisionTransformer, VisionTransformer1D)
