from .vit import (FactorisedLinear, MixerBlock, MultiLayerPredictor, PooledHead, TokenAggregator, TransformerSeqEncoder,  # noqa: F401
                  VisionTransformer, VisionTransformer1D, permute_pos_embed, posemb_sincos_2d)
