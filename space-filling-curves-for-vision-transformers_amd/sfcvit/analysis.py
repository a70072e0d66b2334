"""Where a model attends: attention maps and attention-distance statistics per layer, on the HIP path.

What the reference's commented-out CustomTransformerEncoder (src/models/vit.py:48-174) returned -- `(output,
[attn_weights per layer])` -- without leaving the flash attention kernels: the forward keeps the log-sum-exp of every
score row, and sfcvit_attention_probs / sfcvit_attention_stats rebuild the probabilities from it (csrc/attention_probe.hip).
The statistics never write an N x N map:
    distance           sum_j P_ij ||pos_i - pos_j||   mean attention distance in the image, in pixels
    sequence_distance  sum_j P_ij |i - j|             the same along the token sequence, i.e. along the curve
    entropy            -sum_j P_ij ln P_ij            nats
Analysis runs eagerly under no_grad with every dropout off, whatever `model.training` says; module state is not touched
and the activations carried from layer to layer are those of the ordinary eval forward (same kernel launches).
"""
import numpy as np
import torch

from . import functional as F
from . import ops
from .models import altvit
from .models.vit import PooledHead, VisionTransformer, VisionTransformer1D
from .tokenizers import embeddings


def _grid_positions(gh, gw, ph, pw, order=None):
    """Centres of the ph x pw patches of a gh x gw grid, in raster order or in `order` (flat r * gw + c per token)."""
    flat = np.arange(gh * gw, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
    pos = np.stack(((flat // gw) * ph + (ph - 1) / 2.0, (flat % gw) * pw + (pw - 1) / 2.0), axis=1)
    return torch.from_numpy(pos.astype(np.float32))


def token_positions(patch_embed):
    """[N, 2] fp32 (row, col) centre of every token of a tokenizer: the mean integer pixel coordinate over the token's
    pixels, taken from the tokenizer's own pixel table (sfcvit_pixel_table), so it holds for every curve and any
    (pre-patch, group) geometry.  Hierarchical tokenizers answer with level 0, whose token count is the sequence length.
    A tokenizer whose order changes per call (RandomEmbedding) has no positions: ValueError.  CPU tensor."""
    levels = getattr(patch_embed, "levels", None)
    if levels is not None:
        return token_positions(levels[0])
    if isinstance(patch_embed, altvit.HilbertPatchEmbedding):
        return _grid_positions(patch_embed.grid_h, patch_embed.grid_w, patch_embed.patch_height, patch_embed.patch_width,
                               patch_embed.hilbert_indices.numpy())
    if not isinstance(patch_embed, embeddings._FusedTokenizer):
        raise TypeError(f"token_positions: {type(patch_embed).__name__} is not a tokenizer of this package")
    if not patch_embed._static_order:
        raise ValueError(f"token_positions: {type(patch_embed).__name__} draws a new token order on every call; "
                         "there is no fixed position per token index")
    img, p, g = patch_embed._geom
    grid = img // p
    buf = patch_embed._flat_table()
    flat = np.arange(grid * grid, dtype=np.int32) if buf is None else buf.detach().cpu().numpy()
    pix = embeddings._pixel_table(flat, img, p, g).astype(np.int64)          # [N, P] flat offsets row * img + col
    P = pix.shape[1]
    pos = np.stack(((pix // img).sum(axis=1), (pix % img).sum(axis=1)), axis=1).astype(np.float64) / P
    return torch.from_numpy(pos.astype(np.float32))


def _model_positions(model):
    if isinstance(model, altvit.SimpleViT):
        pat = model.to_patch_embedding[0]
        n = model.pos_embedding.shape[0]
        # SimpleViT keeps no grid shape; square images (every fixture) give it back from the token count
        g = int(round(n ** 0.5))
        if g * g != n:
            raise ValueError("attention_report: pass positions= for a SimpleViT on a non-square patch grid")
        return _grid_positions(g, g, pat.p1, pat.p2)
    if isinstance(model, altvit.HilbertViT):
        return token_positions(model.to_patch_embedding)
    return token_positions(model.patch_embed)


def _head_eval(head, x):
    """MultiLayerPredictor at dropout 0 without reading or writing `head.training`; a PooledHead has no dropout."""
    if isinstance(head, PooledHead):
        return head(x)
    if head._n_layers == 2:
        ln, fact, fc = head[0], head[1], head[4]
        return F.predictor_head(x, ln.weight, ln.bias, fact.W_emb, fact.W_seq, fc.weight, fc.bias, ln.eps, dropout_p=0.0)
    if head.training:
        raise ValueError("attention_report: a MultiLayerPredictor with n_layers != 2 must be in eval mode")
    return head(x)


def _vit_layers(model, images):
    """VisionTransformer / VisionTransformer1D: yields (qkv, lse, n_heads, scale) per encoder layer, then the logits."""
    x = model.patch_embed(images)
    if hasattr(model, "ta"):                 # token_aggregator=...: directly after the tokenizer, as the model's forward
        x = model.ta(x)
    if hasattr(model, "pos_embed"):          # pos_embed=...: after the tokenizer and `ta`, as the model's forward
        x = F.pos_embed(x, model.pos_embed)
    if isinstance(model, VisionTransformer1D):
        x = model.mlp_mixer(x)
    enc = model.encoder
    if getattr(enc, "norm_first", False):    # pre-norm layers: the encoder's own stack on the probe launches, the final norm last
        for _, x, qkv, lse, scale in enc.pre_norm_layers(x, probe=True):
            yield qkv, lse, enc.n_head, scale
        yield _head_eval(model.mlp_head, x)
        return
    for l, layer in enumerate(enc.transformer.layers):
        a = layer.self_attn
        # QK-norm: the probe returns the normalised q, k -- what the attention kernels consumed
        qk = dict(qk_norm=enc.qk_norm[l], qk_norm_eps=enc.qk_norm_eps) if hasattr(enc, "qk_norm") else {}
        if getattr(enc, "rope", None) is not None:              # RoPE: likewise the rotated q, k
            qk["rope"] = enc.rope
        x, qkv, lse, scale = F.encoder_layer_probe(x, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                                                   layer.norm1.weight, layer.norm1.bias, layer.linear1.weight,
                                                   layer.linear1.bias, layer.linear2.weight, layer.linear2.bias,
                                                   layer.norm2.weight, layer.norm2.bias, enc.n_head, layer.norm1.eps, **qk)
        yield qkv, lse, enc.n_head, scale
    yield _head_eval(model.mlp_head, x)


def _altvit_layers(model, images):
    """SimpleViT / HilbertViT (pre-norm blocks, no dropout anywhere): altvit.Attention.forward with F.attention opened up
    -- the same ops.attention_fwd call on the same (zero-padded where the head dim needs it) projection."""
    if isinstance(model, altvit.SimpleViT):
        pat, ln1, lin, ln2 = model.to_patch_embedding
        x = F.layer_norm(pat(images), ln1.weight, ln1.bias, ln1.eps)
        x = F.layer_norm(F.linear(x, lin.weight, lin.bias), ln2.weight, ln2.bias, ln2.eps)
    else:
        x = model.to_patch_embedding(images)
    x = x + model.pos_embedding.to(x.device, dtype=x.dtype)
    tr = model.transformer
    for attn, ff in tr.layers:
        xn = F.layer_norm(x, attn.norm.weight, attn.norm.bias, attn.norm.eps)
        qkv = F._bf(F.linear(xn, attn.to_qkv.weight))
        H, D = attn.heads, qkv.shape[-1] // 3
        hd, hp = F._head_padding(D, H)
        lead, scale = qkv.shape[:-1], None
        if hp != hd:
            qkv = torch.nn.functional.pad(qkv.reshape(*lead, 3, H, hd), (0, hp - hd)).reshape(*lead, 3 * H * hp)
            scale = hd ** -0.5
        qkv = F._c(qkv)
        o, lse = ops.attention_fwd(qkv, H, scale=scale, any_length=True)
        if hp != hd:
            o = o.reshape(*lead, H, hp)[..., :hd].reshape(*lead, D)
        x = F.linear(o, attn.to_out.weight) + x
        x = ff(x) + x
        yield qkv, lse, H, scale
    x = F.layer_norm(x, tr.norm.weight, tr.norm.bias, tr.norm.eps)
    x = x.float().mean(dim=1).to(x.dtype)
    x = model.to_latent(x)
    yield F.linear(x, model.linear_head.weight, model.linear_head.bias)


def attention_report(model, images, layers=None, maps=False, head_mean=True, rows=False, positions=None):
    """One forward of `model` on `images` with the attention of every encoder layer (or of those in `layers`) measured.

    Returns {"logits": the eval forward's logits (same bits), "positions": [N, 2] fp32 on the device,
             "layers": [{"layer": index, "distance": [B, H], "sequence_distance": [B, H], "entropy": [B, H]
                         (means over the query rows), "mass_error": max |sum_j P_ij - 1| (float),
                         "rows": {name: [B, H, N]}           with rows=True,
                         "map": [B, N, N] mean over heads, or [B, H, N, N] with head_mean=False   with maps=True}, ...]}
    maps: True (fp32) or a dtype (torch.float32 / torch.bfloat16).  positions: [N, 2] token centres when the model's
    tokenizer cannot say (default: token_positions).  Supports VisionTransformer, VisionTransformer1D, SimpleViT, HilbertViT."""
    if hasattr(getattr(model, "encoder", None), "cls_token"):
        raise NotImplementedError("attention_report: the model was built with pool='cls'; the CLS token has no place in the "
                                  "image, so distances over its N + 1 tokens would be wrong")
    if getattr(model, "attn_mask", None) is not None:
        raise NotImplementedError("attention_report: the model was built with attn_mask=; the probe kernels rebuild the attention "
                                  "map from q, k and lse WITHOUT a mask and would report wrong maps and distances")
    if getattr(getattr(model, "encoder", None), "rel_pos_bias", None) is not None:
        raise NotImplementedError("attention_report: the model was built with rel_pos_bias=; the probe kernels rebuild the attention "
                                  "map from q, k and lse WITHOUT the bias and would report wrong maps and distances "
                                  "(rel_pos_bias_tables reads the learned reach out of the tables themselves)")
    if isinstance(model, (VisionTransformer, VisionTransformer1D)):
        walk = _vit_layers
    elif isinstance(model, (altvit.SimpleViT, altvit.HilbertViT)):
        walk = _altvit_layers
    else:
        raise TypeError(f"attention_report: unsupported model {type(model).__name__}")
    pos = _model_positions(model) if positions is None else positions
    pos = pos.to(device=images.device, dtype=torch.float32).contiguous()
    want = None if layers is None else {int(i) for i in layers}
    map_dtype = torch.float32 if maps is True else maps
    report = {"positions": pos, "layers": []}
    with torch.no_grad():
        for index, item in enumerate(walk(model, images)):
            if not isinstance(item, tuple):
                report["logits"] = item
                break
            if want is not None and index not in want:
                continue
            qkv, lse, n_heads, scale = item
            st = ops.attention_stats(qkv, lse, n_heads, pos=pos, scale=scale)
            entry = {"layer": index,
                     "distance": st["distance"].mean(dim=2),
                     "sequence_distance": st["sequence_distance"].mean(dim=2),
                     "entropy": st["entropy"].mean(dim=2),
                     "mass_error": float((st["mass"] - 1.0).abs().max())}
            if rows:
                entry["rows"] = st
            if maps:
                entry["map"] = ops.attention_probs(qkv, lse, n_heads, scale=scale, head_mean=head_mean, dtype=map_dtype)
            report["layers"].append(entry)
    return report


def report_summary(report):
    """Per-layer, per-head batch means of an attention_report as plain lists (what main.py --attention-report writes)."""
    return {"tokens": int(report["positions"].shape[0]),
            "layers": [{"layer": e["layer"],
                        "distance": e["distance"].mean(dim=0).tolist(),
                        "sequence_distance": e["sequence_distance"].mean(dim=0).tolist(),
                        "entropy": e["entropy"].mean(dim=0).tolist(),
                        "mass_error": e["mass_error"]} for e in report["layers"]]}


def rel_pos_bias_tables(model):
    """The learned relative position bias of a model built with rel_pos_bias=: {"kind": "curve" | "image", "window": the
    model's rel_pos_window, "cell": pixels per cell ("image" only), "offsets": what each bucket means (relpos.bucket_offsets:
    j - i along the sequence, or (d_row, d_col) in cells; names for the three CLS buckets), "tables": per layer [H, T] fp32 on
    the CPU}.  How far head h of layer l looks, in the geometry the model was given, is the shape of tables[l][h] over
    `offsets`."""
    from . import relpos
    enc = getattr(model, "encoder", None)
    tables = getattr(enc, "rel_pos_bias", None)
    if tables is None:
        raise ValueError("rel_pos_bias_tables: the model was built without rel_pos_bias=")
    kind, window = model.rel_pos_kind, model.rel_pos_window
    cls = hasattr(enc, "cls_token")
    T = enc.rel_pos_index.n_buckets
    out = {"kind": kind, "window": window,
           "offsets": relpos.bucket_offsets(kind, T, n_tokens=enc.max_len, window=window if kind == "curve" else None, cls_token=cls),
           "tables": [t.detach().to("cpu", torch.float32) for t in tables]}
    if kind == "image":
        from .models.vit import rel_pos_cell
        out["cell"] = rel_pos_cell(model.patch_embed)
    return out
