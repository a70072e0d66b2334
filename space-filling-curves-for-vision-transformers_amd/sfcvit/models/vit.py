"""VisionTransformer / VisionTransformer1D on HIP kernels, drop-in for
src/models/vit.py:177-458 of the reference: same constructor signatures, module
tree and state_dict keys, including the token-mix
parameters (unused unless token_mix=True) and the tokenizer registered a second time under `encoder`.

Parameters live in stock torch containers (nn.Linear, nn.LayerNorm,
nn.TransformerEncoder as a *parameter holder*: identical keys and identical
initialisation for a given seed); the arithmetic never goes through them -- every
forward here calls sfcvit.functional, i.e. libsfcvit_hip.so.
"""
import math

import torch
import torch.nn as nn

from .. import functional as F
from .. import ops
from ..tokenizers.base_patch_embedding import BasePatchEmbedding


class TokenAggregator(nn.Module):
    """vit.py:20-42: depth-wise Conv1d(dim, dim, k, s, padding=k//2, groups=dim) along the token sequence, point-wise
    Conv1d, erf-GELU, LayerNorm.  A k-tap window over neighbours in curve order: with a Hilbert tokenizer it covers a
    2-D neighbourhood, with a raster one a row segment.  The reference transposes to [B, D, N] around the convolutions;
    here the activation stays [B, N, D] (F.token_aggregator)."""

    def __init__(self, dim: int, k: int = 3, s: int = 1):
        super().__init__()
        self.dw = nn.Conv1d(dim, dim, k, s, padding=k // 2, groups=dim)
        self.pw = nn.Conv1d(dim, dim, 1, 1)
        self.act = nn.GELU()
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        return F.token_aggregator(x, self.dw.weight, self.dw.bias, self.pw.weight, self.pw.bias, self.norm.weight,
                                  self.norm.bias, stride=self.dw.stride[0], eps=self.norm.eps)


def _make_aggregator(option, embed_dim):
    """The models' `token_aggregator` keyword: False / None = none (the reference as shipped), True = the reference's
    default kernel size 3, an int = that kernel size.  Inside a model the token count must not change: odd k only."""
    if option is None or option is False:
        return None
    k = 3 if option is True else int(option)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"token_aggregator={option!r}: the kernel size must be odd (an even one changes the token count)")
    return TokenAggregator(embed_dim, k)


def _attach_aggregator(model, option, embed_dim):
    """`self.ta = TokenAggregator(embed_dim)` (vit.py:362, commented out there), on request only and constructed LAST: every
    other parameter then draws the same initial values as without it, and the default module tree is today's."""
    ta = _make_aggregator(option, embed_dim)
    if ta is not None:
        model.ta = ta


POS_EMBED_KINDS = ("learned", "sincos1d", "sincos2d")


def posemb_sincos_2d(positions, dim, temperature: float = 10000.0, dtype=torch.float32):
    """Sinusoidal table of token centres `positions` [N, 2] (row, col) in pixels: columns
    [sin(col w) | cos(col w) | sin(row w) | cos(row w)], w_k = temperature^(-k / (dim / 4)), k = 0 .. dim / 4 - 1.  Angles
    are formed in float64 and the table is rounded once.  A function of where a token IS, not of its index: two
    tokenizers over the same centres give the same rows in their own orders."""
    if dim % 4:
        raise ValueError("posemb_sincos_2d: dim must be a multiple of 4")
    q = dim // 4
    freq = torch.pow(torch.tensor(float(temperature), dtype=torch.float64), -torch.arange(q, dtype=torch.float64) / q)
    pos = positions.to(torch.float64)
    col, row = torch.outer(pos[:, 1], freq), torch.outer(pos[:, 0], freq)
    return torch.cat((col.sin(), col.cos(), row.sin(), row.cos()), dim=1).to(dtype)


def _attach_pos_embed(model, kind, std):
    """The models' `pos_embed` keyword (vit.py:360-361, commented out there), on request only and constructed LAST, after
    `ta`: every other parameter then draws the same initial values as without it, and the default module tree is today's.
    "learned" is the reference's line, a Parameter [1, N, D] = randn * std; "sincos1d" / "sincos2d" are persistent buffers
    under the same key (no gradient, nothing launched in backward)."""
    if kind is None or kind is False:
        return
    if kind not in POS_EMBED_KINDS:
        raise ValueError(f"pos_embed={kind!r}: None, {', '.join(map(repr, POS_EMBED_KINDS))} expected")
    n, d = model.patch_embed.n_patches, model.patch_embed.embed_dim
    if d % 8:
        raise ValueError(f"pos_embed={kind!r}: embed_dim={d} must be a multiple of 8 (the kernels move 16-byte vectors of 8 channels)")
    if kind == "learned":
        model.pos_embed = nn.Parameter(torch.randn(1, n, d) * std)
        return
    if kind == "sincos1d":
        from .altvit import posemb_sincos_1d
        table = posemb_sincos_1d(n, d)
    else:
        from ..analysis import token_positions                  # (analysis imports this module: resolved at call time)
        table = posemb_sincos_2d(token_positions(model.patch_embed), d)
    model.register_buffer("pos_embed", table.unsqueeze(0), persistent=True)


def permute_pos_embed(table, from_tokenizer, to_tokenizer):
    """A positional table ([1, N, D] or [N, D]) carried from one token order to another: row i of the result is the row
    of `table` whose token has the centre of `to_tokenizer`'s token i.  Both tokenizers must cover the same set of token
    centres (Hilbert -> Z -> raster at one geometry): anything else is a ValueError.  This is what lets a checkpoint
    trained along one curve start a run along another; a change of resolution is not handled.  Host-only."""
    from ..analysis import token_positions
    src, dst = token_positions(from_tokenizer), token_positions(to_tokenizer)
    if src.shape != dst.shape or table.shape[-2] != src.shape[0] or table.dim() not in (2, 3):
        raise ValueError(f"permute_pos_embed: a table of {table.shape[-2] if table.dim() >= 2 else '?'} rows between tokenizers of "
                         f"{src.shape[0]} and {dst.shape[0]} tokens")
    where = {(float(r), float(c)): i for i, (r, c) in enumerate(src.tolist())}
    if len(where) != src.shape[0]:
        raise ValueError("permute_pos_embed: two tokens of the source tokenizer share a centre")
    try:
        index = torch.tensor([where[(float(r), float(c))] for r, c in dst.tolist()], dtype=torch.long)
    except KeyError:
        raise ValueError("permute_pos_embed: the tokenizers do not cover the same token centres (different geometry)") from None
    if len(set(index.tolist())) != index.numel():
        raise ValueError("permute_pos_embed: two tokens of the target tokenizer share a centre")
    return table.index_select(table.dim() - 2, index.to(table.device))


def drop_path_rates(drop_path_rate, n_layers):
    """The stochastic-depth rate of each encoder layer: linear in depth from 0 to drop_path_rate (timm's rule); one layer gets
    drop_path_rate itself."""
    r = float(drop_path_rate)
    if not 0.0 <= r < 1.0:
        raise ValueError(f"drop_path_rate={drop_path_rate} must be in [0, 1)")
    return [r * l / (n_layers - 1) if n_layers > 1 else r for l in range(n_layers)]


class TransformerSeqEncoder(nn.Module):
    """vit.py:177-242: `depth` post-norm nn.TransformerEncoderLayer (relu, eps 1e-5).  forward(x, mask=None) mirrors
    nn.TransformerEncoder.forward(src, mask): the mask goes to every layer (the reference's CustomTransformerEncoder,
    vit.py:152-174).  A mask is not a parameter or a buffer: it never enters state_dict."""

    def __init__(self, input_dim, max_len, n_head, hidden_dim, method, dropout_p=0.1, n_layers=1, cls_token=False,
                 drop_path_rate=0.0, rel_pos_bias=None, norm_first=False, activation="relu", layer_scale=None, qk_norm=False,
                 qk_norm_eps=1e-6, rope=None, rope_base=None):
        """norm_first=True: pre-norm layers, x + f(LN(x)), and a final LayerNorm after the last one -- torch's
        nn.TransformerEncoderLayer(norm_first=True, activation=...) under nn.TransformerEncoder(norm=nn.LayerNorm(D)), so the
        state_dict keys are torch's own (`transformer.layers.<l>.*`, `transformer.norm.weight|bias`); F.pre_norm_layer runs them.
        activation: "relu" or "gelu" (erf) in the MLP; "gelu" needs norm_first.  layer_scale: None, or the initial value
        (e.g. 1e-4) of LayerScale (CaiT / DeiT-III): `layer_scale`, a ParameterList of one [2, input_dim] tensor per layer, row 0
        scaling the attention branch and row 1 the MLP branch per channel; needs norm_first.  The final norm and LayerScale are
        constructed last and draw no random number; with norm_first=False the encoder is what it is without the three keywords.
        qk_norm=True: QK-norm (ViT-22B; timm's qk_norm=True), a LayerNorm(head_dim, eps=qk_norm_eps) on the queries and keys of
        every head before q k^T, in post- and pre-norm layers alike: `qk_norm`, a ParameterList of one [4, head_dim] tensor per
        layer with rows q_weight, q_bias, k_weight, k_bias = 1, 0, 1, 0 (timm's blocks.<l>.attn.q_norm.weight | .bias and
        k_norm.weight | .bias), shared by the heads of a layer.  Constructed after everything else of the encoder, no draw;
        False: the encoder as it is without the keyword.
        rope: None (the encoder as it is without the keyword), "curve" or "image": rotary position embedding on the queries and
        keys of every layer, after QK-norm (attach_rope, which the models call after everything else is constructed); rope_base:
        None for the kind's default.  No parameter and no state_dict key.
        rel_pos_bias: None, or an ops.AttentionBiasIndex (or (index, init_std)): every layer adds a learned relative
        position bias per head to its attention scores, one table `rel_pos_bias.<l>` [n_head, T] per layer in a ParameterList
        (attach_rel_pos_bias; the models call it after everything else is constructed).
        drop_path_rate: stochastic depth (DropPath) in training mode.  Layer l of L drops each of its two residual branches
        per image with probability drop_path_rates[l] = drop_path_rate * l / (L - 1) (0 for the first layer; a single layer
        gets drop_path_rate) and scales the kept ones by 1 / (1 - rate).  No parameter, buffer or state_dict key; eval mode and
        rate 0 run the launches they run without it.
        cls_token=True: a learnable [CLS] token `cls_token` [1, 1, input_dim] of zeros (vit.py:209-210, commented out
        there) that forward puts in front of the sequence before the first layer (vit.py:237-238): [B, N, D] in,
        [B, N + 1, D] out.  Constructed last: every other parameter draws what it draws without it."""
        super().__init__()
        self.max_len = max_len
        self.grid_size = int(math.sqrt(max_len))
        self.n_head = n_head
        self.dropout_p = dropout_p
        self.drop_path_rates = drop_path_rates(drop_path_rate, n_layers)
        self.norm_first, self.activation = bool(norm_first), activation
        self.qk_norm_eps = float(qk_norm_eps)
        if qk_norm:
            if input_dim % n_head:
                raise ValueError(f"qk_norm=True: input_dim={input_dim} is not a multiple of n_head={n_head}")
            if not (self.qk_norm_eps >= 0.0 and math.isfinite(self.qk_norm_eps)):
                raise ValueError(f"qk_norm_eps={qk_norm_eps} must be finite and >= 0")
            if ops.padded_head_dim(input_dim // n_head) is None:
                raise ValueError(f"qk_norm=True: head dim {input_dim // n_head} exceeds the largest supported one, "
                                 f"{max(ops.SUPPORTED_HEAD_DIMS)}")
        if activation not in ("relu", "gelu"):
            raise ValueError(f"activation={activation!r} must be 'relu' or 'gelu'")
        if not norm_first and activation != "relu":
            raise ValueError(f"activation={activation!r} needs norm_first=True: the post-norm layer has the ReLU MLP only")
        if not norm_first and layer_scale is not None:
            raise ValueError("layer_scale needs norm_first=True: the post-norm layer has no LayerScale")
        if norm_first:
            F._check_pre_norm_width(input_dim, "norm_first=True")
            if layer_scale is not None and not math.isfinite(float(layer_scale)):
                raise ValueError(f"layer_scale={layer_scale} must be a finite initial value")
        extra = dict(norm_first=True, activation=activation) if norm_first else {}      # else: the constructor call as it was
        encoder_layer = nn.TransformerEncoderLayer(d_model=input_dim, nhead=n_head,
                                                   dim_feedforward=hidden_dim, dropout=dropout_p,
                                                   batch_first=True, **extra)
        self.transformer = nn.TransformerEncoder(encoder_layer, num_layers=n_layers,
                                                 enable_nested_tensor=False)
        self.to_patch_embedding = method
        if cls_token:
            if input_dim % 8:
                raise ValueError(f"cls_token=True: input_dim={input_dim} must be a multiple of 8 (the kernels move 16-byte "
                                 "vectors of 8 channels)")
            self.cls_token = nn.Parameter(torch.zeros(1, 1, input_dim))
        if rel_pos_bias is not None:
            index, std = rel_pos_bias if isinstance(rel_pos_bias, tuple) else (rel_pos_bias, 0.0)
            self.attach_rel_pos_bias(index, std)
        if norm_first:
            self.transformer.norm = nn.LayerNorm(input_dim)     # nn.TransformerEncoder(norm=): ones and zeros, no draw
            if layer_scale is not None:
                self.layer_scale = nn.ParameterList(nn.Parameter(torch.full((2, input_dim), float(layer_scale)))
                                                    for _ in range(n_layers))
        if qk_norm:
            row = torch.tensor([1.0, 0.0, 1.0, 0.0]).unsqueeze(1)
            self.qk_norm = nn.ParameterList(nn.Parameter(row.expand(4, input_dim // n_head).clone()) for _ in range(n_layers))
        self.input_dim = input_dim
        if rope is not None and rope is not False:
            self.attach_rope(rope, rope_base)

    def attach_rope(self, kind, base=None):
        """Rotary position embedding for every layer.  "curve": the angle grows with the index along the token sequence
        (sfcvit.rope.curve_table, base 10000 by default), so q_i . k_j depends on the offset j - i along the curve; "image":
        half of the channel pairs turn with the column and half with the row of the token's centre in the image, in cells of
        sqrt(pixels per token) pixels (sfcvit.rope.image_table, base 100 by default; a hierarchical tokenizer answers with level
        0), whatever the curve.  With a CLS token the table gets an identity row in front: the CLS token is not rotated.  The
        table is fixed: `rope_table`, a NON-persistent buffer [N, head_dim / 2, 2] -- no state_dict key, so checkpoints load with
        and without the option -- and `rope`, the validated ops.RopeTable whose device copy the kernels read."""
        from .. import rope as rope_tables
        if kind not in ROPE_KINDS:
            raise ValueError(f"rope={kind!r}: None, {', '.join(map(repr, ROPE_KINDS))} expected")
        D, H = self.input_dim, self.n_head
        if D % H:
            raise ValueError(f"rope={kind!r}: input_dim={D} is not a multiple of n_head={H}")
        hd = D // H
        if hd % 2:
            raise ValueError(f"rope={kind!r}: head dim {hd} must be even: channels rotate in pairs")
        if kind == "image" and hd % 4:
            raise ValueError(f"rope='image': head dim {hd} must be a multiple of 4: half of the pairs turn with the column, half "
                             "with the row")
        if ops.padded_head_dim(hd) is None:
            raise ValueError(f"rope={kind!r}: head dim {hd} exceeds the largest supported one, {max(ops.SUPPORTED_HEAD_DIMS)}")
        base = rope_tables.DEFAULT_BASE[kind] if base is None else float(base)
        if not (math.isfinite(base) and base > 0):
            raise ValueError(f"rope_base={base} must be finite and > 0")
        pe = self.to_patch_embedding
        if kind == "curve":
            table = rope_tables.curve_table(self.max_len, hd, base)
        else:
            from ..analysis import token_positions              # (analysis imports this module: resolved at call time)
            table = rope_tables.image_table(token_positions(pe), rel_pos_cell(pe), hd, base)
        if hasattr(self, "cls_token"):
            table = rope_tables.with_cls_token(table)
        self.rope_kind, self.rope_base = kind, base
        self.rope = ops.RopeTable(table)
        self.register_buffer("rope_table", self.rope.table.clone(), persistent=False)

    def attach_rel_pos_bias(self, bias_index, init_std=0.0):
        """One table [n_head, T] per layer, zeros or randn * init_std (init_std = 0 draws nothing: the model then computes
        at initialisation what it computes without the bias).  The index is static and held outside state_dict."""
        if not isinstance(bias_index, ops.AttentionBiasIndex):
            raise ValueError("rel_pos_bias: an ops.AttentionBiasIndex is expected (sfcvit.relpos builds the index)")
        n = self.max_len + (1 if hasattr(self, "cls_token") else 0)
        if bias_index.n_tokens != n:
            raise ValueError(f"rel_pos_bias: index for {bias_index.n_tokens} tokens on an encoder of {n}")
        shape = (self.n_head, bias_index.n_buckets)
        self.rel_pos_index = bias_index
        self.rel_pos_bias = nn.ParameterList(
            nn.Parameter(torch.randn(shape) * init_std if init_std > 0 else torch.zeros(shape)) for _ in self.transformer.layers)

    def _mask(self, mask):
        """The AttentionMask of `mask`; a tensor is validated and uploaded at its first use and remembered while the same
        tensor object keeps coming."""
        if mask is None or isinstance(mask, ops.AttentionMask):
            return mask
        cached = self.__dict__.get("_mask_cache")
        if cached is None or cached[0] is not mask:
            cached = self.__dict__["_mask_cache"] = (mask, ops.as_attention_mask(mask))
        return cached[1]

    def forward(self, x, mask=None):
        p = self.dropout_p if self.training else 0.0
        mask = self._mask(mask)
        tables, qks, rope = getattr(self, "rel_pos_bias", None), getattr(self, "qk_norm", None), getattr(self, "rope", None)
        if tables is not None and mask is not None:
            raise ValueError("TransformerSeqEncoder: rel_pos_bias and a mask cannot be combined; the window belongs in the "
                             "bias index (rel_pos_window)")
        if hasattr(self, "cls_token"):
            x = F.cls_prepend(x, self.cls_token)                # vit.py:237-238
        if self.norm_first:
            for out in self.pre_norm_layers(x, mask, p):
                pass
            return out[1]
        for l, (layer, rate) in enumerate(zip(self.transformer.layers, self.drop_path_rates)):
            a = layer.self_attn
            path = {"drop_path": rate} if self.training and rate > 0 else {}      # else: the call as it is without the feature
            if tables is not None:
                path["rel_bias"] = (tables[l], self.rel_pos_index)
            if qks is not None:
                path["qk_norm"], path["qk_norm_eps"] = qks[l], self.qk_norm_eps
            if rope is not None:
                path["rope"] = rope
            x = F.encoder_layer(x, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                                layer.norm1.weight, layer.norm1.bias, layer.linear1.weight, layer.linear1.bias,
                                layer.linear2.weight, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias,
                                self.n_head, layer.norm1.eps, dropout_p=p, attn_mask=mask, **path)
        return x

    def pre_norm_layers(self, x, mask=None, p=0.0, probe=False):
        """The pre-norm stack, one F.pre_norm_layer per layer: each takes the residual stream s and n = norm1(s) and returns s'
        and the FOLLOWING norm of s' (the next layer's norm1, the final norm after the last layer).  Yields (s', n') per layer
        -- the last n' is the encoder's output -- or, with probe=True (eval launches, no autograd), F.pre_norm_layer_probe's
        (s', n', qkv, lse, scale)."""
        if F._traced():                                         # before the first launch: layer 0's norm1 runs ahead of its layer
            raise NotImplementedError("pre_norm_layer: the pre-norm layer has no traced form (torch.compile); run the model eagerly")
        layers = list(self.transformer.layers)
        follow =[l.norm1 for l in layers[1:]] + [self.transformer.norm]
        tables, scales = getattr(self, "rel_pos_bias", None), getattr(self, "layer_scale", None)
        s = x
        n = F.layer_norm(s, layers[0].norm1.weight, layers[0].norm1.bias, layers[0].norm1.eps)
        for l, (layer, nxt, rate) in enumerate(zip(layers, follow, self.drop_path_rates)):
            a = layer.self_attn
            w = (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, layer.norm2.weight, layer.norm2.bias,
                 layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, nxt.weight, nxt.bias)
            kw = dict(activation=self.activation, layer_scale=scales[l] if scales is not None else None)
            if hasattr(self, "qk_norm"):
                kw["qk_norm"], kw["qk_norm_eps"] = self.qk_norm[l], self.qk_norm_eps
            if getattr(self, "rope", None) is not None:
                kw["rope"] = self.rope
            if probe:
                out = F.pre_norm_layer_probe(s, n, *w, self.n_head, layer.norm2.eps, **kw)
            else:
                if self.training and rate > 0:
                    kw["drop_path"] = rate
                if tables is not None:
                    kw["rel_bias"] = (tables[l], self.rel_pos_index)
                out = F.pre_norm_layer(s, n, *w, self.n_head, layer.norm2.eps, dropout_p=p, attn_mask=mask, **kw)
            s, n = out[0], out[1]
            yield out


class MixerBlock(nn.Module):
    """vit.py:250-273.  token_mix=False (the reference as shipped, :269-271 commented out): only the channel-mix branch
    is live; the token-mix parameters exist (state_dict compatibility) and never receive a gradient.  token_mix=True: the
    token-mix branch runs first, x + token_mix(token_mix_ln(x)^T)^T along the token axis (F.token_mix, no transposes), and
    its six parameters train like every other.  The parameters are the same either way: same keys, same seeded values."""

    def __init__(self, seq_len, embed_dim, hidden_dim, out_dim, token_mix=False):
        super().__init__()
        self.seq_len, self.use_token_mix = seq_len, bool(token_mix)
        self.token_mix_ln = nn.LayerNorm(embed_dim)
        self.channel_mix_ln = nn.LayerNorm(embed_dim)
        self.token_mix = nn.Sequential(nn.Linear(seq_len, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, seq_len))
        self.channel_mix = nn.Sequential(nn.Linear(embed_dim, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, out_dim))

    def forward(self, x):
        ln, fc1, fc2 = self.channel_mix_ln, self.channel_mix[0], self.channel_mix[2]
        tm = None
        if self.use_token_mix:
            if x.shape[1] != self.seq_len:
                raise ValueError(f"MixerBlock(token_mix=True) was built for {self.seq_len} tokens and got {x.shape[1]}: the "
                                 "token-mix weights fix the token count (a stride-changing TokenAggregator in front of it "
                                 "is not supported)")
            tln, t1, t2 = self.token_mix_ln, self.token_mix[0], self.token_mix[2]
            tm = (tln.weight, tln.bias, t1.weight, t1.bias, t2.weight, t2.bias)
        return F.mixer_block(x, ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, ln.eps, token_mix=tm)


class FactorisedLinear(nn.Module):
    """vit.py:276-292: y[b, o] = sum_{n, r} (x[b, n, :] . W_emb[r, :]) * W_seq[o, n, r]."""

    def __init__(self, seq_len, embed_dim, rank, out_dim):
        super().__init__()
        self.W_emb = nn.Parameter(torch.empty(rank, embed_dim))
        self.W_seq = nn.Parameter(torch.empty(out_dim, seq_len, rank))
        nn.init.xavier_normal_(self.W_emb)
        nn.init.xavier_normal_(self.W_seq)

    def forward(self, x):
        b, n, _ = x.shape
        h = F.linear(x, self.W_emb)
        return F.linear(h.reshape(b, n * self.W_emb.shape[0]), self.W_seq.reshape(self.W_seq.shape[0], -1))


class MultiLayerPredictor(nn.Sequential):
    """vit.py:295-319.  The n_layers = 2 form the models use runs as one fused function."""

    def __init__(self, embed_dim, seq_len, n_layers=2, rank=64, dropout_p=0.5, num_classes=10, mix=False):
        super().__init__()
        if mix:
            raise TypeError("MultiLayerPredictor(mix=True) cannot be constructed in the reference either "
                            "(vit.py:301 passes 3 of MixerBlock's 4 arguments)")
        self.append(nn.LayerNorm(embed_dim))
        fact_out = embed_dim * 2
        self.append(FactorisedLinear(seq_len, embed_dim, rank, fact_out))
        self.append(nn.GELU())
        self.append(nn.Dropout(dropout_p))
        prev_dim = fact_out
        for _ in range(n_layers - 2):
            next_dim = prev_dim // 2
            self.append(nn.Linear(prev_dim, next_dim))
            self.append(nn.GELU())
            self.append(nn.Dropout(dropout_p))
            prev_dim = next_dim
        self.append(nn.Linear(prev_dim, num_classes))
        self._n_layers = n_layers
        self._dropout_p = dropout_p

    def forward(self, x):
        p = self._dropout_p if self.training else 0.0
        if self._n_layers == 2:
            ln, fact, fc = self[0], self[1], self[4]
            return F.predictor_head(x, ln.weight, ln.bias, fact.W_emb, fact.W_seq, fc.weight, fc.bias, ln.eps,
                                    dropout_p=p)
        # any depth (vit.py:310-318): every nn.GELU here is followed by its nn.Dropout -- one fused pass per pair
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.LayerNorm):
                x = F.layer_norm(x, m.weight, m.bias, m.eps)
            elif isinstance(m, nn.Linear):
                x = F.linear(x, m.weight, m.bias)
            elif isinstance(m, nn.GELU) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.Dropout):
                x = F.gelu_dropout(x, p)
                i += 1
            elif isinstance(m, nn.GELU):
                x = F.gelu(x)
            elif isinstance(m, nn.Dropout):
                if p > 0:
                    raise NotImplementedError("a Dropout that does not follow a GELU")
            else:
                x = m(x)
            i += 1
        return x


POOL_KINDS = ("cls", "mean")


class PooledHead(nn.Sequential):
    """The head of a pooled classifier: LayerNorm(D), Linear(D, num_classes) on ONE vector per image -- token 0 of a model
    with a CLS token (pool="cls") or the mean of the tokens (pool="mean").  Unlike MultiLayerPredictor it holds no weight
    per token index: its size and its checkpoint do not depend on N, and it has no view of a token's place on the curve."""

    def __init__(self, embed_dim, num_classes=10, pool="mean"):
        super().__init__(nn.LayerNorm(embed_dim), nn.Linear(embed_dim, num_classes))
        self.pool = pool

    def forward(self, x):
        x = F.token_pool(x, 0, 1) if self.pool == "cls" else F.token_pool(x)
        ln, fc = self[0], self[1]
        return F.pooled_head(x, ln.weight, ln.bias, fc.weight, fc.bias, ln.eps)


def _check_pool(pool, embed_dim):
    if pool is None:
        return
    if pool not in POOL_KINDS:
        raise ValueError(f"pool={pool!r}: None, {', '.join(map(repr, POOL_KINDS))} expected")
    if embed_dim % 8:
        raise ValueError(f"pool={pool!r}: embed_dim={embed_dim} must be a multiple of 8 (the kernels move 16-byte vectors of 8 channels)")


def _model_mask(attn_mask, n_patches, pool):
    """The models' attn_mask: N x N, or (N + 1) x (N + 1) with pool="cls" (masks.with_cls_token carries a window over)."""
    n = n_patches + 1 if pool == "cls" else n_patches
    if attn_mask is None:
        return None
    rows = attn_mask.n_tokens if isinstance(attn_mask, ops.AttentionMask) else torch.as_tensor(attn_mask).shape[0]
    if pool == "cls" and rows == n_patches:
        raise ValueError(f"attn_mask has {n_patches} rows and pool='cls' gives the encoder {n} tokens: pass "
                         "sfcvit.masks.with_cls_token(mask)")
    return ops.as_attention_mask(attn_mask, n)


REL_POS_KINDS = ("curve", "image")
ROPE_KINDS = ("curve", "image")


def _attach_rel_pos_bias(model, kind, window, init_std, attn_mask, pool):
    """The models' `rel_pos_bias` keyword, on request only and constructed LAST, after `ta`, `pos_embed` and `cls_token`:
    every other parameter then draws the same initial values as without it, and the default module tree is today's.
    "curve": the offset j - i along the token sequence, rel_pos_window in tokens; "image": the displacement of the token
    centres in cells of sqrt(pixels per token) pixels, rel_pos_window in pixels.  One table per encoder layer,
    `encoder.rel_pos_bias.<l>` [H, T]."""
    if kind is None or kind is False:
        if window is not None:
            raise ValueError("rel_pos_window needs rel_pos_bias='curve' or 'image'")
        return
    if kind not in REL_POS_KINDS:
        raise ValueError(f"rel_pos_bias={kind!r}: None, {', '.join(map(repr, REL_POS_KINDS))} expected")
    if attn_mask is not None:
        raise ValueError("rel_pos_bias and attn_mask cannot be combined: pass the window as rel_pos_window (tokens for 'curve', "
                         "pixels for 'image'); the bias index then hides the pairs outside it")
    from .. import relpos
    pe = model.patch_embed
    if kind == "curve":
        index, T = relpos.curve_offsets(pe.n_patches, window)
    else:
        from ..analysis import token_positions                  # (analysis imports this module: resolved at call time)
        pos = token_positions(pe)
        index, T = relpos.image_offsets(pos, rel_pos_cell(pe), window)
    if pool == "cls":
        index, T = relpos.with_cls_token(index, T)
    model.rel_pos_kind, model.rel_pos_window = kind, window
    model.encoder.attach_rel_pos_bias(ops.AttentionBiasIndex(index, T), float(init_std))


def _attach_rope(model, kind, base):
    """The models' `rope` keyword, on request only and constructed LAST, after `ta`, `pos_embed`, `cls_token` and the relative
    position bias: no parameter, no draw, no state_dict key (TransformerSeqEncoder.attach_rope)."""
    if kind is None or kind is False:
        if base is not None:
            raise ValueError("rope_base needs rope='curve' or 'image'")
        return
    model.encoder.attach_rope(kind, base)


def rel_pos_cell(patch_embed):
    """The pixel pitch image offsets are counted in: the square root of the pixels per token."""
    levels = getattr(patch_embed, "levels", None)               # hierarchical: level 0 is the sequence (analysis.token_positions)
    pe = levels[0] if levels is not None else patch_embed
    geom = getattr(pe, "_geom", None)                           # (image side, pre-patch side, group)
    if geom is None:
        raise ValueError(f"rel_pos_bias='image': {type(pe).__name__} does not say how many pixels a token covers")
    return math.sqrt(geom[0] * geom[0] / pe.n_patches)


def _make_head(pool, embed_dim, n_patches, num_classes, head_dropout_p):
    if pool is None:
        return MultiLayerPredictor(embed_dim, n_patches, n_layers=2, num_classes=num_classes, dropout_p=head_dropout_p)
    return PooledHead(embed_dim, num_classes, pool)


class VisionTransformer(nn.Module):
    """vit.py:325-385 (`embed_dim` is ignored there too: taken from the tokenizer, :351)."""

    def __init__(self, patch_embed: BasePatchEmbedding, embed_dim=128, depth=6, n_heads=4, mlp_dim=256,
                 num_classes=10, dropout_p=0.1, head_dropout_p=0.5, token_aggregator=False, attn_mask=None,
                 pos_embed=None, pos_embed_std=1.0, pool=None, drop_path_rate=0.0, rel_pos_bias=None, rel_pos_window=None,
                 rel_pos_init_std=0.0, norm_first=False, activation="relu", layer_scale=None, qk_norm=False, qk_norm_eps=1e-6,
                 rope=None, rope_base=None):
        """rel_pos_bias: None (the model as it is without the keyword), "curve" or "image": every encoder layer adds a learned
        relative position bias per head to its attention scores, softmax(q k^T / sqrt(hd) + b_h[offset(i, j)]), the offset taken
        along the token sequence (j - i) or in the image (the displacement of the token centres in cells of sqrt(pixels per
        token) pixels, whatever the curve).  rel_pos_window: None, or the window the index hides pairs beyond -- tokens for
        "curve", pixels for "image" (the windows of sfcvit.masks); not together with attn_mask.  One table per layer,
        `encoder.rel_pos_bias.<l>` [H, T], constructed last; rel_pos_init_std = 0 (zeros: the model starts out computing what
        it computes without the bias) or the std of a normal draw.  With pool="cls" the CLS token gets three buckets of its own
        (sfcvit.relpos.with_cls_token).
        drop_path_rate: stochastic depth over the encoder layers (TransformerSeqEncoder; `encoder.drop_path_rates`).
        norm_first, activation, layer_scale: pre-norm encoder layers with a final norm, a GELU MLP and LayerScale
        (TransformerSeqEncoder: the DeiT / timm block; `encoder.transformer.norm`, `encoder.layer_scale.<l>` [2, D]).
        qk_norm, qk_norm_eps: QK-norm, a LayerNorm over the head dim on the queries and keys of every head
        (TransformerSeqEncoder; `encoder.qk_norm.<l>` [4, head_dim]).
        rope, rope_base: None (the model as it is without the keyword), "curve" or "image": rotary position embedding on the
        queries and keys of every encoder layer, the angle taken from the index along the token sequence or from the token's
        centre in the image (TransformerSeqEncoder.attach_rope); rope_base None = the kind's default (10000 / 100).  Built last;
        a fixed table in a non-persistent buffer, so state_dict is unchanged by it; with pool="cls" the CLS token is not rotated.
        attn_mask: None, or a mask for every encoder layer (ops.as_attention_mask's forms; sfcvit.masks builds windows).
        Held outside state_dict: checkpoint keys are the reference's with or without it.
        pos_embed: None / False (the reference as shipped), "learned" (vit.py:360-361: a Parameter [1, N, D] = randn *
        pos_embed_std), "sincos1d" (fixed, of the token index along the curve) or "sincos2d" (fixed, of the token's centre in
        the image: the same whatever curve orders the tokens).  Added directly after the tokenizer and, if present, `ta`
        (vit.py:380-383): before the encoder here, before `mlp_mixer` in VisionTransformer1D -- one place for both models.
        pool: None (the reference as shipped: the factorised head over all tokens), "cls" (the encoder owns a learnable
        `encoder.cls_token`, vit.py:209-210, :237-238, put in front of the N patch tokens; `ta` and `pos_embed` act on the patch
        tokens only, the CLS row gets no positional row; the head reads token 0; attn_mask must then be (N + 1) x (N + 1):
        sfcvit.masks.with_cls_token) or "mean" (no extra token; the head reads the mean of the N tokens).  Both pooled kinds
        use `mlp_head = PooledHead`: LayerNorm(D), Linear(D, num_classes); head_dropout_p is unused with a pooled head."""
        super().__init__()
        self.patch_embed = patch_embed
        embed_dim = patch_embed.embed_dim
        _check_pool(pool, embed_dim)
        self.attn_mask = _model_mask(attn_mask, patch_embed.n_patches, pool)
        self.encoder = TransformerSeqEncoder(input_dim=embed_dim, max_len=self.patch_embed.n_patches,
                                             method=self.patch_embed, n_head=n_heads, hidden_dim=mlp_dim,
                                             n_layers=depth, dropout_p=dropout_p, cls_token=pool == "cls",
                                             drop_path_rate=drop_path_rate, norm_first=norm_first, activation=activation,
                                             layer_scale=layer_scale, qk_norm=qk_norm, qk_norm_eps=qk_norm_eps)
        self.mlp_head = _make_head(pool, embed_dim, self.patch_embed.n_patches, num_classes, head_dropout_p)
        _attach_aggregator(self, token_aggregator, embed_dim)
        _attach_pos_embed(self, pos_embed, pos_embed_std)
        _attach_rel_pos_bias(self, rel_pos_bias, rel_pos_window, rel_pos_init_std, self.attn_mask, pool)
        _attach_rope(self, rope, rope_base)

    def forward(self, x, mix=None):
        """mix: a sfcvit.training.BatchMix applied to the image batch by the tokenizer, or None."""
        x = self.patch_embed(x) if mix is None else self.patch_embed(x, mix=mix)
        if hasattr(self, "ta"):
            x = self.ta(x)                                      # vit.py:381
        if hasattr(self, "pos_embed"):
            x = F.pos_embed(x, self.pos_embed)                  # vit.py:382
        x = self.encoder(x, mask=self.attn_mask)
        return self.mlp_head(x)


class VisionTransformer1D(nn.Module):
    """vit.py:392-458: tokenizer -> channel-mix block -> encoder stack -> factorised head.  token_mix=True switches the
    MixerBlock's token-mix branch on (vit.py:269-271, commented out in the reference): a learned mixing along the curve,
    the only pre-encoder component that sees absolute position in curve order."""

    def __init__(self, patch_embed: BasePatchEmbedding, embed_dim=128, depth=6, n_heads=4, mlp_dim=256,
                 num_classes=10, dropout_p=0.1, head_dropout_p=0.5, token_aggregator=False, token_mix=False, attn_mask=None,
                 pos_embed=None, pos_embed_std=1.0, pool=None, drop_path_rate=0.0, rel_pos_bias=None, rel_pos_window=None,
                 rel_pos_init_std=0.0, norm_first=False, activation="relu", layer_scale=None, qk_norm=False, qk_norm_eps=1e-6,
                 rope=None, rope_base=None):
        """attn_mask, pos_embed, pos_embed_std, pool, drop_path_rate, rel_pos_bias, rel_pos_window, rel_pos_init_std, norm_first, activation, layer_scale, qk_norm, qk_norm_eps, rope, rope_base: as in VisionTransformer (the table is added directly after the tokenizer
        and, if present, `ta`: before `mlp_mixer`; with pool="cls" the token joins after `mlp_mixer`, whose weights stay sized
        for the N patch tokens)."""
        super().__init__()
        self.patch_embed = patch_embed
        embed_dim = patch_embed.embed_dim
        _check_pool(pool, embed_dim)
        self.attn_mask = _model_mask(attn_mask, patch_embed.n_patches, pool)
        self.mlp_mixer = MixerBlock(seq_len=self.patch_embed.n_patches, embed_dim=embed_dim,
                                    hidden_dim=embed_dim * 2, out_dim=embed_dim, token_mix=token_mix)
        self.encoder = TransformerSeqEncoder(input_dim=embed_dim, max_len=self.patch_embed.n_patches,
                                             n_head=n_heads, hidden_dim=mlp_dim, n_layers=depth,
                                             method=self.patch_embed, dropout_p=dropout_p, cls_token=pool == "cls",
                                             drop_path_rate=drop_path_rate, norm_first=norm_first, activation=activation,
                                             layer_scale=layer_scale, qk_norm=qk_norm, qk_norm_eps=qk_norm_eps)
        self.mlp_head = _make_head(pool, embed_dim, self.patch_embed.n_patches, num_classes, head_dropout_p)
        _attach_aggregator(self, token_aggregator, embed_dim)
        _attach_pos_embed(self, pos_embed, pos_embed_std)
        _attach_rel_pos_bias(self, rel_pos_bias, rel_pos_window, rel_pos_init_std, self.attn_mask, pool)
        _attach_rope(self, rope, rope_base)

    def forward(self, x, mix=None):
        """mix: a sfcvit.training.BatchMix applied to the image batch by the tokenizer, or None."""
        x = self.patch_embed(x) if mix is None else self.patch_embed(x, mix=mix)
        if hasattr(self, "ta"):
            x = self.ta(x)
        if hasattr(self, "pos_embed"):
            x = F.pos_embed(x, self.pos_embed)
        x = self.mlp_mixer(x)
        x = self.encoder(x, mask=self.attn_mask)
        return self.mlp_head(x)
