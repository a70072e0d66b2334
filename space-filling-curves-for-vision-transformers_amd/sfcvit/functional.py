"""Block-level autograd functions of the hot path, built on sfcvit.ops (HIP kernels).

Granularity follows the reference's modules so that every fusion the backward
needs is local to one function:
  patch_embed    HilbertEmbedding1D / MortonEmbedding1D / RasterScan1DEmbedding / SFCEmbedding1D .forward
  mixer_block    MixerBlock.forward                     (src/models/vit.py:268-273)
  token_mix      its token-mix branch                   (src/models/vit.py:269-271)
  token_aggregator TokenAggregator.forward              (src/models/vit.py:37-42)
  pos_embed      x + self.pos_embed                     (src/models/vit.py:382, commented out there)
  cls_prepend    torch.cat([cls_token.expand(B, -1, -1), x], dim=1)  (src/models/vit.py:237-238, commented out there)
  token_pool     x[:, 0] / x[:, a:b].mean(dim=1)        (the read-out of a pooled classifier head)
  pooled_head    LayerNorm + Linear on the pooled token
  encoder_layer  nn.TransformerEncoderLayer, post-norm  (torch:nn/modules/transformer.py:951-982)
  pre_norm_layer nn.TransformerEncoderLayer(norm_first=True) + the following norm, GELU, LayerScale (same file, the norm_first branch)
  predictor_head MultiLayerPredictor(n_layers=2)        (src/models/vit.py:295-319)
  linear, layer_norm, gelu                              generic pieces
  soft_target_cross_entropy                             main.py:45-51
All activations and parameters are bf16 inside; fp32 parameters are cast on entry
(differentiably), so gradients come back in the parameter's own dtype.
"""
import math

import torch
from torch.autograd import Function

from . import ops

_BF16 = torch.bfloat16


def _bf(t):
    return t if t is None or t.dtype == _BF16 else t.to(_BF16)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _like(g, ref):
    """Gradient `g` in the dtype of the tensor it belongs to."""
    return g if g.dtype == ref.dtype else g.to(ref.dtype)


_SLOTS_OFF = False     # sfcvit.library: inside a traced custom op gradients must be fresh tensors, never views of the flat buffer


def _slot(p):
    """A fresh view of parameter `p`'s place in its optimizer's flat gradient buffer (FlatGradBuffer.slots), or None.
    Kernels write the gradient there directly and return the view: autograd, finding p.grad unset, adopts it as
    p.grad without a copy -- no fp32 -> bf16 cast and no `p.grad += g` pass per parameter (146 + 106 tiny kernels per
    ViT-B step).  Only when p.grad is None: with an existing gradient autograd would add the view to itself."""
    if _SLOTS_OFF or p is None or not p.is_leaf or p.grad is not None:
        return None
    slot = getattr(p, "_sfcvit_slot", None)
    if slot is None:
        return None
    buf, off = slot
    if getattr(p, "_sfcvit_claimed", -1) == buf.epoch:
        # second use of a shared parameter in one backward: autograd must add.  It adds (first use's slot view + this
        # use's fresh tensor) as soon as this use returns, i.e. it READS the slot now: a reduction the first use queued
        # for the end of the pass (ops._Deferring) has to land before that.
        ops.flush_deferred(end=False)
        return None
    p._sfcvit_claimed = buf.epoch
    view = buf.flat_grad[off:off + p.numel()].view(p.shape)
    view._sfcvit_deferrable = True          # ops._Deferring: a reduction that ends here may wait for the end of the backward pass
    return view


def _wgrad(dy2, x2, w=None):
    """dW[out, in] = dY^T X  (contraction over rows; both operands k-major), into w's gradient slot if it has one."""
    return ops.gemm(dy2, x2, a_kmajor=True, b_kmajor=True, out=_slot(w))


class _SideStream:
    """Weight-gradient GEMMs do not feed the rest of backward, so they run on a second HIP stream
    next to the dX chain: the tail round of one kernel (1176 tiles on 512 workgroup slots leave the
    third round 30 % full) could be filled with workgroups of the other.  MEASURED SLOWER on MI355X
    (5 110 vs 5 210 img/s, A/B in one process): the two GEMMs evict each other's panels from L2.
    Kept as an option (SFCVIT_SIDE_STREAM=1), off by default."""
    _streams = {}

    def __init__(self, device):
        self.main = torch.cuda.current_stream(device)
        key = (device.index, self.main.cuda_stream)
        if key not in _SideStream._streams:
            _SideStream._streams[key] = torch.cuda.Stream(device)
        self.side = _SideStream._streams[key]

    def run(self, fn, *tensors):
        """fn() on the side stream after everything issued so far on the main stream."""
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            out = fn()
        for t in tensors:                       # inputs allocated on the main stream, read on the side stream
            t.record_stream(self.side)
        return out

    def join(self, *outs):
        self.main.wait_stream(self.side)
        for t in outs:                          # allocated on the side stream, consumed on the main stream
            if t is not None:
                t.record_stream(self.main)


import os as _os
SIDE_STREAM_WGRAD = _os.environ.get("SFCVIT_SIDE_STREAM", "0") == "1"
USE_ACTMASK = _os.environ.get("SFCVIT_ACTMASK", "1") == "1"        # "0": linear2's dX reads the stored activation (A/B)


def _ln_slots(w, b):
    """grad_out for ops.layernorm_bwd: (dgamma slot, dbeta slot, None) when both parameters have one, else None."""
    sw, sb = _slot(w), _slot(b)
    return (sw, sb, None) if sw is not None and sb is not None else None


def _ln_grads(dg, db, go):
    return (dg, db) if go is not None else (dg.to(_BF16), db.to(_BF16))


def _bgrad(dy2, b=None):
    out = _slot(b)
    return ops.colsum(dy2, out=out) if out is not None else ops.colsum(dy2).to(_BF16)


# ----------------------------------------------------------------------------
PE_TWO_STAGE = _os.environ.get("SFCVIT_PE_FUSED", "0") != "1"   # "1": the fused gather-GEMM kernels (rounds 1-2) instead of gather + GEMM


class _PatchEmbed2(Function):
    """Gather, then project (round 3).  The fused kernels of rounds 1-2 make the gather the A loader of their own GEMM and run
    it at 280 TFLOP/s (192 us forward, 185 + 30 us backward at ViT-B / 256 images, the image read 2-3 times); materialising the
    token matrix once (154 MB of fp32 image in, 77 MB of bf16 tokens out) lets the projection and its weight gradient run on
    the persistent GEMMs at 950-1 150 TFLOP/s -- what the reference does (hilbert_embedding1D.py:36-43), minus its reshape copy."""

    @staticmethod
    def forward(ctx, x, pix, w, b, desc, order, mix=None):
        B, (N, P) = x.shape[0], pix.shape
        tokens = ops.gather_tokens(_c(x), pix, desc, order, mix)      # mix: MixUp / CutMix inside the gather; backward sees tokens only
        ctx.save_for_backward(tokens, w)
        ctx.small = (b,)
        return ops.gemm(tokens, w, bias=b).view(B, N, w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        tokens, w = ctx.saved_tensors
        dy2 = _c(dy).view(-1, dy.shape[-1])
        b = ctx.small[0]
        return None, None, _wgrad(dy2, tokens, w), (_bgrad(dy2, b) if b is not None else None), None, None, None


class _PatchEmbed(Function):
    @staticmethod
    def forward(ctx, x, pix, w, b, desc):
        tiled = ops.patch_embed_is_tiled(desc, pix.shape[1], w.shape[0])
        if tiled:
            # tiles / strips: the tiled kernel reads whole 16-pixel row segments of the image AS IT IS (fp32 from the
            # loader: one pass over 154 MB at ViT-B / 256 images; a bf16 copy first would cost that pass plus its own
            # write and re-read) and rounds to bf16 on the way into LDS -- the same rounding, the same tokens
            x = _c(x)
        else:
            # The generic kernels round the pixels to bf16 when they load them; doing that once up front gives the same
            # tokens bit for bit, halves the bytes both kernels pull through the texture path (they are bound by it: every
            # 128-column tile of D re-reads its token tile) and halves what is kept for backward (77 instead of 154 MB).
            x = _c(x if x.dtype == _BF16 else x.to(_BF16))
        ctx.save_for_backward(x, pix)
        ctx.D = w.shape[0]
        ctx.has_bias = b is not None
        ctx.desc = desc if tiled else None
        return ops.patch_embed_fwd(x, pix, w, b, ctx.desc)

    @staticmethod
    def backward(ctx, dy):
        x, pix = ctx.saved_tensors
        dw, db = ops.patch_embed_bwd(x, pix, _c(dy), ctx.D, want_bias=ctx.has_bias, desc=ctx.desc)
        return None, None, dw.to(_BF16), (db.to(_BF16) if db is not None else None), None


def _traced():
    """Under torch.compile the blocks run as `sfcvit::` custom ops (sfcvit/library.py): one graph, no breaks."""
    return torch.compiler.is_compiling()


def pe_two_stage(x, pix, D):
    """Gather + GEMM (default) or the fused kernels?  The GEMM wants 16-byte rows (P * C a multiple of 8), and the split only
    pays where the projection is big enough to be GPU-bound: two launches forward and four backward instead of one and two
    cost a launch-bound model more than the faster GEMM returns (CIFAR-size tokenizers: 0.3 GFLOP per pass)."""
    K = pix.shape[1] * x.shape[1]
    return PE_TWO_STAGE and K % 8 == 0 and 2.0 * x.shape[0] * pix.shape[0] * K * D >= 4e9


def mix_images(x, mix):
    """The MixUp / CutMix'd image batch (fp32, one pass: ops.mix_images), for the tokenizers that do not materialise
    tokens.  Images receive no gradient; mix = None returns x."""
    if mix is None:
        return x
    if _traced():
        from . import library
        return library.mix_images(x, mix)
    return ops.mix_images(x.detach(), mix)


def patch_embed(x, pix, weight, bias, desc=None, order=None, mix=None):
    """Curve gather + patchify + projection: x [B,C,H,W] (fp32 or bf16) -> [B,N,D] bf16.
    desc = ops.TileDesc of the pixel table (tokens are 16 x 16 tiles / 256-pixel strips) or None: picks the tile gather
    kernel (and the fused kernels of SFCVIT_PE_FUSED=1); order = ops.gather_order of the table on the device, or None.
    mix = a sfcvit.training.BatchMix or None: MixUp / CutMix of the batch, inside the gather where tokens are
    materialised (gather + GEMM), as one pass over the image in front of the fused kernels otherwise (they re-gather
    from the saved image in backward and so need the mixed one)."""
    if _traced():
        from . import library
        return library.patch_embed(mix_images(x, mix), pix, _bf(weight), _bf(bias), desc)
    if pe_two_stage(x, pix, weight.shape[0]):
        return _PatchEmbed2.apply(x, pix, _bf(weight), _bf(bias), desc, order, mix)
    return _PatchEmbed.apply(mix_images(x, mix), pix, _bf(weight), _bf(bias), desc)


class _ResampleConcat(Function):
    """Linear resampling of the coarser levels to the first level's token count + concatenation (multi_hilbert.py:33-38)."""

    @staticmethod
    def forward(ctx, *levels):
        levels = [_c(t) for t in levels]
        ctx.n_tokens, ctx.D = [t.shape[1] for t in levels], levels[0].shape[2]
        return ops.hier_resample_concat(levels)

    @staticmethod
    def backward(ctx, dout):
        return tuple(ops.hier_resample_concat_bwd(_c(dout), ctx.n_tokens, ctx.D))


def hier_resample_concat(levels):
    """levels: list of [B, N_l, D] -> [B, N_0, L * D] bf16 (sfcvit_hier_resample_concat)."""
    return _ResampleConcat.apply(*[_bf(t) for t in levels])


# SFCVIT_HIER_ONE_KERNEL=1: gather + levels + concatenation + fusion Linear in ONE kernel (csrc/hier_tokenizer.hip,
# FUSE = true).  Default: the same kernel without its last phase (gather + levels + concatenation) followed by the
# fusion Linear on the persistent 8-phase GEMM -- measured faster at the reference's shape.
HIER_ONE_KERNEL = _os.environ.get("SFCVIT_HIER_ONE_KERNEL", "0") == "1"


class _HierTokenizer(Function):
    """Fused hierarchical tokenizer (ops.hier_tokenizer_fwd).  Saved for backward: the image (bf16, what the kernel's
    gather rounds to anyway) and the concatenated level outputs h; backward is the chain rule on existing kernels:
    dh = dy Wf, dWf = dy^T h, then per level the tokenizer weight gradient from that level's columns of dh."""

    @staticmethod
    def forward(ctx, x, wf, bf, n_levels, one_kernel, *rest):
        pix = rest[:n_levels]
        w = rest[n_levels:2 * n_levels]
        b = rest[2 * n_levels:3 * n_levels]
        x = _c(x if x.dtype == _BF16 else x.to(_BF16))
        if one_kernel:
            y, h = ops.hier_tokenizer_fwd(x, pix, w, b, wf, bf)
        else:
            _, h = ops.hier_tokenizer_fwd(x, pix, w, b, None, None)
            y = ops.gemm(h.view(-1, h.shape[-1]), wf, bias=bf).view(h.shape)
        ctx.save_for_backward(x, h, wf, *pix)
        ctx.n_levels, ctx.params = n_levels, (w, b, bf)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, wf = ctx.saved_tensors[:3]
        pix = ctx.saved_tensors[3:]
        w, b, bf = ctx.params
        L = ctx.n_levels
        E = h.shape[-1]
        D = E // L
        dy2, h2 = _c(dy).view(-1, E), h.view(-1, E)
        dwf = _wgrad(dy2, h2, wf)
        dbf = _bgrad(dy2, bf) if bf is not None else None
        dh = ops.gemm_dx(dy2, wf).view(h.shape)
        dws, dbs = [], []
        for l in range(L):
            dwl, dbl = ops.patch_embed_bwd(x, pix[l], _c(dh[..., l * D:(l + 1) * D]), D, want_bias=b[l] is not None)
            dws.append(dwl.to(_BF16))
            dbs.append(dbl.to(_BF16) if dbl is not None else None)
        return (None, dwf, dbf, None, None) + (None,) * L + tuple(dws) + tuple(dbs)


def hier_tokenizer(x, pix_list, weights, biases, fusion_weight, fusion_bias, one_kernel=None):
    """y = fusion(concat_l(level_l(x))) for levels with one common token count (reference:
    multiscale/multi_hilbert.py:31-40).  x [B,C,H,W] -> [B, N, L*D] bf16.  one_kernel: True = everything in one kernel,
    False = fused gather + levels + concatenation, then the fusion Linear as a GEMM; None = HIER_ONE_KERNEL."""
    L = len(pix_list)
    one = HIER_ONE_KERNEL if one_kernel is None else bool(one_kernel)
    return _HierTokenizer.apply(x, _bf(fusion_weight), _bf(fusion_bias), L, one, *pix_list, *[_bf(w) for w in weights],
                                *[_bf(b) for b in biases])


# ----------------------------------------------------------------------------
class _Linear(Function):
    @staticmethod
    def forward(ctx, x, w, b, act):
        x2 = _c(x).view(-1, x.shape[-1])
        if act == ops.ACT_GELU:
            y, pre = ops.gemm(x2, w, bias=b, act=act, want_aux=True)
            ctx.save_for_backward(x2, w, pre)
        else:
            y = ops.gemm(x2, w, bias=b, act=act)
            ctx.save_for_backward(x2, w, y if act == ops.ACT_RELU else None)
        ctx.act, ctx.has_bias, ctx.shape = act, b is not None, x.shape
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, aux = ctx.saved_tensors
        dy2 = _c(dy).view(-1, dy.shape[-1])
        if ctx.act == ops.ACT_RELU:
            dy2 = torch.where(aux > 0, dy2, torch.zeros_like(dy2))
        elif ctx.act == ops.ACT_GELU:
            dy2 = ops.gelu_bwd(dy2, aux)
        dx = ops.gemm_dx(dy2, w).view(ctx.shape)
        return dx, _wgrad(dy2, x2, w), (_bgrad(dy2) if ctx.has_bias else None), None


def linear(x, weight, bias=None, act=ops.ACT_NONE):
    """y = act(x W^T + b).  Output widths that are not a multiple of 8 (a 10-class head) are computed on zero-padded
    rows of W (16-byte output rows) and sliced back; the padding is differentiable torch plumbing."""
    x, weight, bias = _bf(x), _bf(weight), _bf(bias)
    out = weight.shape[0]
    pad = (-out) % 8
    if pad:
        weight = torch.nn.functional.pad(weight, (0, 0, 0, pad))
        bias = torch.nn.functional.pad(bias, (0, pad)) if bias is not None else None
        return _Linear.apply(x, weight, bias, act)[..., :out]
    return _Linear.apply(x, weight, bias, act)


class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        x2 = _c(x).view(-1, x.shape[-1])
        y, mean, rstd = ops.layernorm_fwd(x2, w, b, eps)
        ctx.save_for_backward(x2, mean, rstd, w)
        ctx.small = (b,)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, w = ctx.saved_tensors
        go = _ln_slots(w, ctx.small[0])
        dx, dg, db = ops.layernorm_bwd(_c(dy).view(-1, dy.shape[-1]), x2, mean, rstd, w, grad_out=go)
        return (dx.view(dy.shape), *_ln_grads(dg, db, go), None)


def layer_norm(x, weight, bias, eps=1e-5):
    return _LayerNorm.apply(_bf(x), _bf(weight), _bf(bias), eps)


class _Gelu(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.save_for_backward(x)
        return ops.gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.gelu_bwd(_c(dy), x)


def gelu(x):
    return _Gelu.apply(_bf(x))


class _GeluDrop(Function):
    """dropout_p(gelu_erf(x)) in one pass, the mask regenerated in backward (nn.GELU followed by nn.Dropout:
    MultiLayerPredictor's hidden layers, src/models/vit.py:303-318)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = _c(x)
        ctx.save_for_backward(x)
        ctx.p, ctx.seed, ctx.shape = p, seed, x.shape
        return ops.gelu_drop_fwd(x.view(-1, x.shape[-1]), p, seed).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = ops.gelu_drop_bwd(_c(dy).view(-1, x.shape[-1]), x.view(-1, x.shape[-1]), ctx.p, ctx.seed)
        return dx.view(ctx.shape), None, None


def gelu_dropout(x, p):
    """Dropout(p)(GELU(x)), training mode (p > 0 draws a fresh mask per call; p = 0 is gelu)."""
    if p <= 0:
        return gelu(x)
    return _GeluDrop.apply(_bf(x), float(p), ops.next_seed())


def _attention_mask(mask, n_tokens, what):
    """ops.as_attention_mask for a layer call.  Under tracing a mask is refused: the torch.library ops have no masked form."""
    if mask is None:
        return None
    if _traced():
        raise NotImplementedError(f"{what}: an attention mask is not supported under torch.compile / tracing (the torch.library "
                                  "ops have no masked form); run the masked model eagerly")
    return ops.as_attention_mask(mask, n_tokens)


def _table_grad(dtable, table):
    """The fp32 table gradient of the bias kernels in the parameter's dtype: in its gradient slot when it has one."""
    slot = _slot(table)
    if slot is None:
        return _like(dtable, table)
    slot.copy_(dtable)
    return slot


def _fp32_bias(rel_table, rel_index):
    """The attention core's third form as the kernels take it: (the table parameter cast to fp32, once per call; the index)."""
    return None if rel_index is None else (_c(rel_table.detach().to(torch.float32)), rel_index)


def _attn_fwd(qkv3, n_heads, p, seed, scale, attn_mask, rel_bias):
    """The attention core of a layer and of `attention` on qkv3 [B, N, 3 * H * hd] -> (o, lse): the bias kernels with rel_bias =
    (fp32 table [H, T], ops.AttentionBiasIndex), the masked kernels with an ops.AttentionMask, and only then; the plain ones
    otherwise.  This and _attn_bwd are the only place that chooses."""
    if rel_bias is not None:
        return ops.attention_bias_fwd(qkv3, n_heads, *rel_bias, p, seed, scale=scale)
    if attn_mask is not None:
        return ops.attention_masked_fwd(qkv3, n_heads, *attn_mask.on(qkv3.device), p, seed, scale=scale)
    return ops.attention_fwd(qkv3, n_heads, p, seed, scale=scale, any_length=True)


def _attn_bwd(qkv3, o, lse, do3, n_heads, p, seed, scale, attn_mask, rel_bias, want_colsum, in_b, rel_table, want_table,
              fp32_sums=False):
    """-> (dqkv, dbi or None, dtable or None).  want_colsum: the in_proj bias gradient (column sums of dqkv) comes out of the
    attention backward itself, into in_b's gradient slot when it has one.  want_table = False (a frozen table) costs nothing;
    otherwise the table gradient comes back as _table_grad leaves it.  fp32_sums (_qk_norm_bwd): the column sums come back as a
    fresh fp32 tensor and no slot is touched."""
    col = None
    if want_colsum:
        bi_slot = None if fp32_sums else _slot(in_b)
        col = bi_slot if bi_slot is not None else True
    dtable = None
    if rel_bias is not None:
        dqkv, dtable, *dbi = ops.attention_bias_bwd(qkv3, o, lse, do3, n_heads, *rel_bias, p, seed, colsum=col, scale=scale,
                                                    table_grad=want_table)
        dtable = _table_grad(dtable, rel_table) if want_table else None
    else:
        if attn_mask is not None:
            got = ops.attention_masked_bwd(qkv3, o, lse, do3, n_heads, *attn_mask.on(qkv3.device), p, seed, colsum=col, scale=scale)
        else:
            got = ops.attention_bwd(qkv3, o, lse, do3, n_heads, p, seed, colsum=col, scale=scale, any_length=True)
        dqkv, *dbi = got if want_colsum else (got,)
    if not want_colsum:
        return dqkv, None, dtable
    return dqkv, (dbi[0].to(_BF16) if col is True and not fp32_sums else dbi[0]), dtable


def _qk_norm_fwd(qkv, qk, cfg):
    """QK-norm of a layer, between the projection GEMM and the attention core: with qk [4, hd] (q_weight, q_bias, k_weight,
    k_bias) the q and k thirds of qkv [M, 3 * H * hp] are normalised per head IN PLACE and the raw q | k, which the backward
    needs, is returned; with qk = None nothing is launched.  This and _qk_norm_bwd are the only place that decides."""
    if qk is None:
        return None
    return ops.qk_norm_fwd(qkv, qk, cfg.n_heads, qk.shape[1], cfg.qk_eps)


def _qk_norm_bwd(attn_bwd, raw, qk, qk_param, in_b, cfg):
    """The attention backward of a layer with the mirror of _qk_norm_fwd behind it -> (dqkv, dbi, dtable, dqk or None).
    attn_bwd(fp32_sums): _attn_bwd with the layer's arguments.  Without QK-norm that is all.  With it, the attention backward's
    column sums are the bias gradient for the v third alone: they come back as fp32, never into the slot, and ops.qk_norm_bwd
    -- which rewrites dq | dk in place -- writes its own q | k sums and carries the v sums over, into in_b's slot when it has
    one, so the slot holds one kernel's complete answer whatever reductions are queued.  dqk goes into qk_param's slot."""
    if raw is None:
        return attn_bwd(False) + (None,)
    dqkv, sums, dtable = attn_bwd(True)
    Da = raw.shape[1] // 2
    bi_slot, qk_slot = _slot(in_b), _slot(qk_param)
    dbi = bi_slot if bi_slot is not None else torch.empty(3 * Da, device=raw.device, dtype=_BF16)
    _, dqk, _ = ops.qk_norm_bwd(dqkv, raw, qk, cfg.n_heads, qk.shape[1], cfg.qk_eps, colsum=dbi, grad_out=qk_slot, vsum=sums[2 * Da:])
    return dqkv, dbi, dtable, (dqk if qk_slot is not None else dqk.to(_BF16))


def _qk_norm_arg(qk_norm, qk_norm_eps, hd, what):
    """A layer call's qk_norm = None or a [4, head_dim] tensor (rows q_weight, q_bias, k_weight, k_bias; the model's head dim,
    not the padded one) -> (bf16 tensor or None, eps).  A bf16 parameter passes as it is, so its gradient can be written into its
    slot.  Refused under tracing: the torch.library ops have no QK-norm form."""
    if qk_norm is None:
        return None, float(qk_norm_eps)
    if _traced():
        raise NotImplementedError(f"{what}: qk_norm is not supported under torch.compile / tracing (the torch.library ops have "
                                  "no QK-norm form); run the model eagerly")
    if not isinstance(qk_norm, torch.Tensor) or tuple(qk_norm.shape) != (4, hd):
        got = tuple(qk_norm.shape) if isinstance(qk_norm, torch.Tensor) else type(qk_norm).__name__
        raise ValueError(f"{what}: qk_norm must be a [4, head_dim] = [4, {hd}] tensor (q_weight, q_bias, k_weight, k_bias), got {got}")
    eps = float(qk_norm_eps)
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError(f"{what}: qk_norm_eps={qk_norm_eps} must be finite and >= 0")
    return _c(_bf(qk_norm)), eps


def _rope_fwd(qkv, cfg):
    """RoPE of a layer, after QK-norm and before the attention core: with cfg.rope (an ops.RopeTable) the channel pairs of the q
    and k thirds of qkv [M, 3 * H * hp] are rotated per token IN PLACE; nothing is kept for the backward.  With cfg.rope = None
    nothing is launched.  This and _rope_bwd are the only place that decides."""
    if cfg.rope is not None:
        ops.rope_fwd(qkv, cfg.rope, cfg.n_heads)


def _rope_bwd(attn_bwd, in_b, cfg):
    """attn_bwd(fp32_sums) -- _attn_bwd with the layer's arguments -- with the mirror of _rope_fwd behind it, in the same form, so
    that _qk_norm_bwd takes either.  Without RoPE it is attn_bwd itself.  With it, the attention backward's column sums are
    the bias gradient for the v third alone: they come back as fp32, never into the slot.  Asked for fp32 sums (QK-norm follows
    and owns the q | k sums) the transposed rotation runs in its no-sums form, one launch; otherwise ops.rope_bwd writes the
    column sums of the dq | dk it stores and carries the v sums over, into in_b's slot when it has one."""
    if cfg.rope is None:
        return attn_bwd

    def run(fp32_sums):
        dqkv, sums, dtable = attn_bwd(True)
        if fp32_sums:
            ops.rope_bwd(dqkv, cfg.rope, cfg.n_heads)
            return dqkv, sums, dtable
        Da = sums.numel() // 3
        bi_slot = _slot(in_b)
        dbi = bi_slot if bi_slot is not None else torch.empty(3 * Da, device=dqkv.device, dtype=_BF16)
        ops.rope_bwd(dqkv, cfg.rope, cfg.n_heads, colsum=dbi, vsum=sums[2 * Da:])
        return dqkv, dbi, dtable
    return run


def _rope_arg(rope, n_tokens, hd, what):
    """A layer call's rope = None, an ops.RopeTable or a CPU fp32 [N, head_dim / 2, 2] table (sfcvit.rope builds them; head_dim
    = the model's head dim, not the padded one) -> ops.RopeTable or None, matching n_tokens and hd where the caller knows them
    (None: not known here; ops checks the table against the buffer).  Refused under tracing: the torch.library ops have no RoPE
    form."""
    if rope is None:
        return None
    if _traced():
        raise NotImplementedError(f"{what}: rope is not supported under torch.compile / tracing (the torch.library ops have "
                                  "no RoPE form); run the model eagerly")
    if isinstance(rope, torch.Tensor):
        rope = ops.RopeTable(rope)
    if not isinstance(rope, ops.RopeTable):
        raise ValueError(f"{what}: rope must be an ops.RopeTable or a CPU fp32 [N, head_dim / 2, 2] table, got {type(rope).__name__}")
    if hd is not None and hd % 2:
        raise ValueError(f"{what}: rope needs an even head dim, got {hd}: channels rotate in pairs")
    if (n_tokens is not None and rope.n_tokens != n_tokens) or (hd is not None and rope.head_dim != hd):
        raise ValueError(f"{what}: rope table for {rope.n_tokens} tokens and head dim {rope.head_dim} on a sequence of {n_tokens} "
                         f"tokens with head dim {hd}")
    return rope


class _Rope(Function):
    """rope: the stand-alone differentiable form on a copy of the packed projection (the layers use the in-place kernels)."""

    @staticmethod
    def forward(ctx, qkv, table, n_heads):
        ctx.table, ctx.n_heads = table, n_heads
        return ops.rope_fwd(qkv.clone(memory_format=torch.contiguous_format), table, n_heads)

    @staticmethod
    def backward(ctx, dout):
        dqkv, _ = ops.rope_bwd(dout.clone(memory_format=torch.contiguous_format), ctx.table, ctx.n_heads)
        return dqkv, None, None


def rope(qkv, table, n_heads):
    """Rotary position embedding of a packed projection qkv [B, N, 3 * H * hp] (or [B * N, ..]; q | k | v thirds, head h at
    columns h * hp .. of each third): the channel pairs (2 p, 2 p + 1) of every query and key head row are rotated by the
    table's (cos, sin) of the row's token, v unchanged -> a new tensor.  table: an ops.RopeTable, or a CPU fp32
    [N, head_dim / 2, 2] table (sfcvit.rope.curve_table / image_table); head_dim <= hp, the columns above it come out +0; hp
    must be 64, 128, 192 or 256.  The table receives no gradient."""
    qkv = _bf(qkv)
    if n_heads <= 0 or qkv.shape[-1] % (3 * n_heads):
        raise ValueError(f"rope: packed width {qkv.shape[-1]} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    hp = qkv.shape[-1] // (3 * n_heads)
    if hp not in ops.SUPPORTED_HEAD_DIMS:
        raise ValueError(f"rope: packed head width {hp} must be one of {ops.SUPPORTED_HEAD_DIMS}")
    if table is None:
        raise ValueError("rope: table must be an ops.RopeTable or a CPU fp32 [N, head_dim / 2, 2] table")
    table = _rope_arg(table, qkv.shape[1] if qkv.dim() == 3 else None, None, "rope")
    return _Rope.apply(qkv, table, n_heads)


class _QkNorm(Function):
    """qk_norm: the stand-alone differentiable form on a copy of the packed projection (the layers use the in-place kernels)."""

    @staticmethod
    def forward(ctx, qkv, params, n_heads, eps):
        out = qkv.clone(memory_format=torch.contiguous_format)
        raw = ops.qk_norm_fwd(out, params, n_heads, params.shape[1], eps)
        ctx.save_for_backward(raw, params)
        ctx.n_heads, ctx.eps = n_heads, eps
        return out

    @staticmethod
    def backward(ctx, dout):
        raw, params = ctx.saved_tensors
        dqkv = dout.clone(memory_format=torch.contiguous_format)
        _, dP, _ = ops.qk_norm_bwd(dqkv, raw, params, ctx.n_heads, params.shape[1], ctx.eps)
        return dqkv, dP.to(_BF16), None, None


def qk_norm(qkv, n_heads, params, eps=1e-6, head_dim=None):
    """QK-norm (ViT-22B; timm's qk_norm=True) of a packed projection qkv [.., 3 * H * hp] (q | k | v thirds, head h at columns
    h * hp .. of each third): a LayerNorm over the head dim on every query and key head row, v unchanged -> a new tensor.
    params: [4, head_dim], rows q_weight, q_bias, k_weight, k_bias, shared by all heads.  head_dim: the model's head dim when hp
    is a zero-padded kernel head dim (the padded columns stay out of the statistics and come out +0); default hp, which must
    then be 64, 128, 192 or 256."""
    qkv = _bf(qkv)
    if n_heads <= 0 or qkv.shape[-1] % (3 * n_heads):
        raise ValueError(f"qk_norm: packed width {qkv.shape[-1]} is not 3 * n_heads * head_dim for n_heads = {n_heads}")
    hp = qkv.shape[-1] // (3 * n_heads)
    hd = hp if head_dim is None else int(head_dim)
    if hp not in ops.SUPPORTED_HEAD_DIMS or not 1 <= hd <= hp:
        raise ValueError(f"qk_norm: head dim {hd} on a packed head width of {hp}: the width must be one of {ops.SUPPORTED_HEAD_DIMS} "
                         "and 1 <= head_dim <= width")
    params, eps = _qk_norm_arg(params, eps, hd, "qk_norm")
    if params is None:
        raise ValueError("qk_norm: params must be a [4, head_dim] tensor")
    return _QkNorm.apply(qkv, params, n_heads, eps)


def _rel_bias(rel_bias, mask, n_tokens, n_heads, what):
    """A layer call's rel_bias = (table [H, T], ops.AttentionBiasIndex), checked; None stays None.  Not together with a mask
    (a window belongs in the index) and not under tracing (the torch.library ops have no biased form)."""
    if rel_bias is None:
        return None
    if mask is not None:
        raise ValueError(f"{what}: rel_bias and an attention mask cannot be combined: express the window in the bias index "
                         "(sfcvit.relpos.curve_offsets(window=) / image_offsets(radius=)), where hidden pairs are -1")
    if _traced():
        raise NotImplementedError(f"{what}: a relative position bias is not supported under torch.compile / tracing (the "
                                  "torch.library ops have no biased form); run the biased model eagerly")
    try:
        table, index = rel_bias
    except (TypeError, ValueError):
        raise ValueError(f"{what}: rel_bias must be (table [H, T], ops.AttentionBiasIndex)") from None
    if not isinstance(index, ops.AttentionBiasIndex) or not isinstance(table, torch.Tensor):
        raise ValueError(f"{what}: rel_bias must be (table [H, T], ops.AttentionBiasIndex)")
    if tuple(table.shape) != (n_heads, index.n_buckets):
        raise ValueError(f"{what}: rel_bias table must be [H, T] = {(n_heads, index.n_buckets)}, got {tuple(table.shape)}")
    if index.n_tokens != n_tokens:
        raise ValueError(f"{what}: rel_bias index for {index.n_tokens} tokens on a sequence of {n_tokens}")
    return table, index


class _Attention(Function):
    """softmax(q k^T / sqrt(hd)) v per head on a packed projection [B, N, 3 * H * hd] (q | k | v thirds, head h at
    columns h*hd.. of each third): the core of nn.MultiheadAttention and of altvit.Attention (altvit.py:131-142).  With an
    additive mask (ops.AttentionMask) softmax(q k^T / sqrt(hd) + M) v on the masked kernels; with a learned relative position
    bias per head (rel_table [H, T], rel_index) softmax(q k^T / sqrt(hd) + table[h, index]) v on the bias kernels."""

    @staticmethod
    def forward(ctx, qkv, n_heads, scale, mask, rel_table, rel_index):
        qkv = _c(qkv)
        rel_bias = _fp32_bias(rel_table, rel_index)
        out, lse = _attn_fwd(qkv, n_heads, 0.0, 0, scale, mask, rel_bias)
        ctx.save_for_backward(qkv, out, lse)
        ctx.n_heads, ctx.scale, ctx.mask, ctx.rel_bias, ctx.rel_table = n_heads, scale, mask, rel_bias, rel_table
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        want = ctx.rel_bias is not None and ctx.needs_input_grad[4]          # a frozen table costs nothing
        dqkv, _, dtable = _attn_bwd(qkv, out, lse, _c(dout), ctx.n_heads, 0.0, 0, ctx.scale, ctx.mask, ctx.rel_bias, False, None,
                                    ctx.rel_table, want)
        return dqkv, None, None, None, dtable, None


def _head_padding(D, n_heads):
    """(head dim, kernel head dim) of a model width / head count; equal when the kernels have that head dim."""
    if D % n_heads:
        raise ValueError(f"attention: width {D} is not a multiple of n_heads = {n_heads}")
    hd = D // n_heads
    hp = ops.padded_head_dim(hd)
    if hp is None:
        raise ValueError(f"attention: head dim {hd} (= {D} / {n_heads}) exceeds the largest supported one, "
                         f"{max(ops.SUPPORTED_HEAD_DIMS)}")
    return hd, hp


def attention(qkv, n_heads, mask=None, rel_bias=None):
    """Head dims the kernels do not have (32, 48, 96, ...) run zero-padded to the next one that exists: the padded
    q / k / v columns add nothing to q k^T or p v, the softmax scale stays 1 / sqrt(head dim).
    mask: None, or an additive attention mask [N, N] shared by all batches and heads (ops.AttentionMask, a float tensor,
    or a bool tensor with True = may not attend): scores q k^T / sqrt(hd) + mask on the masked kernels (kernel head dim
    64: head dims up to 64).  Without a mask nothing changes.
    rel_bias: None, or (table [H, T], ops.AttentionBiasIndex): a learned relative position bias per head, scores
    q k^T / sqrt(hd) + table[h, index[i, j]] on the bias kernels (kernel head dim 64); the table receives a gradient.  Not
    together with a mask: a window is part of the index (sfcvit.relpos)."""
    qkv = _bf(qkv)
    D = qkv.shape[-1] // 3
    hd, hp = _head_padding(D, n_heads)
    rel_bias = _rel_bias(rel_bias, mask, qkv.shape[-2], n_heads, "attention")
    mask = _attention_mask(mask, qkv.shape[-2], "attention")
    table, index = rel_bias if rel_bias is not None else (None, None)
    if hp == hd:
        return _Attention.apply(qkv, n_heads, None, mask, table, index)
    lead = qkv.shape[:-1]
    padded = torch.nn.functional.pad(qkv.reshape(*lead, 3, n_heads, hd), (0, hp - hd)).reshape(*lead, 3 * n_heads * hp)
    out = _Attention.apply(padded, n_heads, 1.0 / math.sqrt(hd), mask, table, index)
    return out.reshape(*lead, n_heads, hp)[..., :hd].reshape(*lead, D)


def _fast_gemm_shape(M, N, K):
    """Shapes the persistent 8-phase GEMM takes (csrc/dispatch.cpp: plan_p8)."""
    return M >= 192 and N % 256 == 0 and K % 128 == 0 and K >= 256


# ----------------------------------------------------------------------------
class _Mixer(Function):
    """x + W2 gelu(W1 LN(x) + b1) + b2"""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w1, b1, w2, b2, eps):
        x2 = _c(x).view(-1, x.shape[-1])
        z, mean, rstd = ops.layernorm_fwd(x2, ln_w, ln_b, eps)
        if _fast_gemm_shape(z.shape[0], w1.shape[0], z.shape[1]):
            # the persistent 8-phase GEMM has no erf-GELU / second-output epilogue: pre-activation from it (~1000 TFLOP/s)
            # + one elementwise pass beats the older kernel's fused epilogue (500 TFLOP/s): 174 vs 240 us at ViT-B / 256
            u = ops.gemm(z, w1, bias=b1)
            h = ops.gelu_fwd(u)
        else:
            h, u = ops.gemm(z, w1, bias=b1, act=ops.ACT_GELU, want_aux=True)
        y = ops.gemm(h, w2, bias=b2, residual=x2)
        ctx.save_for_backward(x2, mean, rstd, z, u, h, ln_w, w1, w2)
        ctx.small = (ln_b, b1, b2)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, z, u, h, ln_w, w1, w2 = ctx.saved_tensors
        ln_b, b1, b2 = ctx.small
        dy2 = _c(dy).view(-1, dy.shape[-1])
        dw2, db2 = _wgrad(dy2, h, w2), _bgrad(dy2, b2)
        if _fast_gemm_shape(dy2.shape[0], w2.shape[1], dy2.shape[1]):
            du = ops.gelu_bwd(ops.gemm_dx(dy2, w2), u)                     # as in forward: plain 8-phase GEMM + elementwise pass
        else:
            du = ops.gemm_dx(dy2, w2, aux_in=u, dact=ops.ACT_GELU)
        dw1, db1 = _wgrad(du, z, w1), _bgrad(du, b1)
        dz = ops.gemm_dx(du, w1)
        go = _ln_slots(ln_w, ln_b)
        dx, dg, dbeta = ops.layernorm_bwd(dz, x2, mean, rstd, ln_w, dx_add=dy2, grad_out=go)
        return (dx.view(dy.shape), *_ln_grads(dg, dbeta, go), dw1, db1, dw2, db2, None)


def _pair_slots(w, b):
    """out for ops.tokmix_wgrad: (dw slot, db slot) when both parameters have one, else None."""
    sw, sb = _slot(w), _slot(b)
    return (sw, sb) if sw is not None and sb is not None else None


class _TokenMix(Function):
    """x + (W2 gelu(W1 LN(x) + b1) + b2) with the Linears applied along the TOKEN axis: the token-mix branch of MixerBlock
    (src/models/vit.py:269-271) on [B, N, D] as it lies in memory.  W1 [hid, N] and W2 [N, hid] multiply every image's
    [N, D] / [hid, D] matrix from the left (ops.tokmix_left); the biases are row biases; neither the activation nor the
    hidden tensor [B, hid, D] is ever transposed.  Saved for backward: z = LN(x), the pre-activation U and H = gelu(U)."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w1, b1, w2, b2, eps):
        x = _c(x)
        B, N, D = x.shape
        x2 = x.view(B * N, D)
        z, mean, rstd = ops.layernorm_fwd(x2, ln_w, ln_b, eps)
        h, u = ops.tokmix_left(w1, z.view(B, N, D), bias=b1, act=ops.ACT_GELU, want_aux=True)
        y = ops.tokmix_left(w2, h, bias=b2, residual=x)
        ctx.save_for_backward(x2, mean, rstd, z, u, h, ln_w, w1, w2)
        ctx.small = (ln_b, b1, b2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, z, u, h, ln_w, w1, w2 = ctx.saved_tensors
        ln_b, b1, b2 = ctx.small
        dy = _c(dy)
        B, N, D = dy.shape
        s2 = _pair_slots(w2, b2)
        dw2, db2 = ops.tokmix_wgrad(dy, h, out=s2)                           # dW2 = sum_b dy_b H_b^T, db2 = row sums of dy
        du = ops.tokmix_left(w2, dy, transposed=True, aux_in=u)             # dU = (W2^T dy) * gelu'(U)
        s1 = _pair_slots(w1, b1)
        dw1, db1 = ops.tokmix_wgrad(du, z.view(B, N, D), out=s1)
        dz = ops.tokmix_left(w1, du, transposed=True)                       # dz = W1^T dU
        go = _ln_slots(ln_w, ln_b)
        dx, dg, dbeta = ops.layernorm_bwd(dz.view(B * N, D), x2, mean, rstd, ln_w, dx_add=dy.view(B * N, D), grad_out=go)
        if s1 is None:
            dw1, db1 = dw1.to(_BF16), db1.to(_BF16)
        if s2 is None:
            dw2, db2 = dw2.to(_BF16), db2.to(_BF16)
        return (dx.view(B, N, D), *_ln_grads(dg, dbeta, go), dw1, db1, dw2, db2, None)


def token_mix(x, ln_w, ln_b, w1, b1, w2, b2, eps=1e-5):
    """The token-mix branch of MixerBlock (src/models/vit.py:269-271) on x [B, N, D]:
    x + fc2(gelu(fc1(LN(x)^T)))^T with fc1 = Linear(N, hid) (w1 [hid, N]), fc2 = Linear(hid, N) (w2 [N, hid]) -> [B, N, D]
    bf16.  Any N; D and hid multiples of 8."""
    N, hid = x.shape[1], w1.shape[0]
    if x.dim() != 3 or tuple(w1.shape) != (hid, N) or tuple(w2.shape) != (N, hid):
        raise ValueError(f"token_mix: x {tuple(x.shape)} needs w1 [hid, {N}] and w2 [{N}, hid], got {tuple(w1.shape)} and "
                         f"{tuple(w2.shape)}: the token count is fixed by the weights")
    if hid % 8 or x.shape[2] % 8:
        raise ValueError(f"token_mix: hidden width {hid} and embedding width {x.shape[2]} must be multiples of 8")
    args = (_bf(x), _bf(ln_w), _bf(ln_b), _c(_bf(w1)), _bf(b1), _c(_bf(w2)), _bf(b2))
    if _traced():
        from . import library
        return library.token_mix(*args, float(eps))
    return _TokenMix.apply(*args, float(eps))


_token_mix = token_mix        # (mixer_block's keyword has the function's name)


def mixer_block(x, ln_w, ln_b, w1, b1, w2, b2, eps=1e-5, token_mix=None):
    """MixerBlock.forward (src/models/vit.py:268-273).  token_mix = None: the channel-mix branch alone (the reference as
    shipped); (ln_w, ln_b, w1, b1, w2, b2) of the token-mix branch: that branch first (vit.py:269-271), same eps."""
    if token_mix is not None:
        x = _token_mix(x, *token_mix, eps=eps)
    if _traced():
        from . import library
        return library.mixer_block(_bf(x), _bf(ln_w), _bf(ln_b), _bf(w1), _bf(b1), _bf(w2), _bf(b2), eps)
    return _Mixer.apply(_bf(x), _bf(ln_w), _bf(ln_b), _bf(w1), _bf(b1), _bf(w2), _bf(b2), eps)


# ----------------------------------------------------------------------------
def _dw_slots(w, b):
    """out for ops.dwconv1d_bwd: (dw slot, db slot) when both parameters have one, else None."""
    sw, sb = _slot(w), _slot(b)
    return (sw, sb) if sw is not None and sb is not None else None


def _dw_grads(dw, db, slots):
    return (dw, db) if slots is not None else (dw.to(_BF16), db.to(_BF16) if db is not None else None)


class _DwConv1d(Function):
    """Depth-wise nn.Conv1d(D, D, k, stride, padding=k // 2, groups=D) on [B, N, D], D contiguous: no transposes."""

    @staticmethod
    def forward(ctx, x, w, b, stride):
        x = _c(x)
        ctx.save_for_backward(x, w)
        ctx.small, ctx.stride = (b,), stride
        return ops.dwconv1d_fwd(x, w, b, stride)

    @staticmethod
    def backward(ctx, du):
        x, w = ctx.saved_tensors
        b = ctx.small[0]
        slots = _dw_slots(w, b) if b is not None else None
        dx, dw, db = ops.dwconv1d_bwd(_c(du), x, w, ctx.stride, want_dx=ctx.needs_input_grad[0], want_db=b is not None, out=slots)
        return (dx, *_dw_grads(dw, db, slots), None)


def dwconv1d(x, weight, bias=None, stride=1):
    """x [B, N, D] -> [B, Nout, D] bf16; weight is the Conv1d parameter [D, 1, k] (or [D, k]), bias [D] or None."""
    return _DwConv1d.apply(_bf(x), _c(_bf(weight)), _bf(bias), int(stride))


class _TokenAggregator(Function):
    """LN(gelu(pw(dw(x)))): TokenAggregator.forward (src/models/vit.py:37-42) without its two transposes -- the depth-wise
    conv kernel on [B, N, D], the point-wise Conv1d as a GEMM, GELU with the pre-activation kept (the fast-shape split of
    _Mixer), LayerNorm."""

    @staticmethod
    def forward(ctx, x, dw_w, dw_b, pw_w, pw_b, ln_w, ln_b, stride, eps):
        x = _c(x)
        B, _, D = x.shape
        u = ops.dwconv1d_fwd(x, dw_w, dw_b, stride)
        u2 = u.view(-1, D)
        pw2 = pw_w.view(D, D)
        if _fast_gemm_shape(u2.shape[0], D, D):
            v = ops.gemm(u2, pw2, bias=pw_b)
            g = ops.gelu_fwd(v)
        else:
            g, v = ops.gemm(u2, pw2, bias=pw_b, act=ops.ACT_GELU, want_aux=True)
        y, mean, rstd = ops.layernorm_fwd(g, ln_w, ln_b, eps)
        ctx.save_for_backward(x, u2, v, g, mean, rstd, dw_w, pw_w, ln_w)
        ctx.small, ctx.stride = (dw_b, pw_b, ln_b), stride
        return y.view(B, -1, D)

    @staticmethod
    def backward(ctx, dy):
        x, u2, v, g, mean, rstd, dw_w, pw_w, ln_w = ctx.saved_tensors
        dw_b, pw_b, ln_b = ctx.small
        B, _, D = x.shape
        dy2 = _c(dy).view(-1, D)
        go = _ln_slots(ln_w, ln_b)
        dgl, dgam, dbeta = ops.layernorm_bwd(dy2, g, mean, rstd, ln_w, grad_out=go)
        dv = ops.gelu_bwd(dgl, v)
        spw = _slot(pw_w)                                     # the Conv1d weight [D, D, 1]: its slot is the [D, D] matrix
        dpw = ops.gemm(dv, u2, a_kmajor=True, b_kmajor=True, out=None if spw is None else spw.view(D, D))
        dpw = spw if spw is not None else dpw.view(pw_w.shape)
        dpb = _bgrad(dv, pw_b)
        du = ops.gemm_dx(dv, pw_w.view(D, D)).view(B, -1, D)
        slots = _dw_slots(dw_w, dw_b)
        want_dx = getattr(ctx, "needs_input_grad", (True,))[0]
        dx, ddw, ddb = ops.dwconv1d_bwd(du, x, dw_w, ctx.stride, want_dx=want_dx, out=slots)
        return (dx, *_dw_grads(ddw, ddb, slots), dpw, dpb, *_ln_grads(dgam, dbeta, go), None, None)


def token_aggregator(x, dw_w, dw_b, pw_w, pw_b, ln_w, ln_b, stride=1, eps=1e-5):
    """TokenAggregator (src/models/vit.py:20-42) on x [B, N, D]: depth-wise Conv1d (dw_w [D, 1, k], padding k // 2, stride)
    -> point-wise Conv1d (pw_w [D, D, 1]) -> erf-GELU -> LayerNorm.  -> [B, Nout, D] bf16."""
    args = (_bf(x), _c(_bf(dw_w)), _bf(dw_b), _c(_bf(pw_w)), _bf(pw_b), _bf(ln_w), _bf(ln_b))
    if _traced():
        from . import library
        return library.token_aggregator(*args, int(stride), float(eps))
    return _TokenAggregator.apply(*args, int(stride), float(eps))


# ----------------------------------------------------------------------------
class _PosEmbed(Function):
    """x + pos over the batch (src/models/vit.py:382, commented out there).  dx is dy itself; the table's gradient is the
    batch sum of dy, computed only when the table asks for one (a fixed sin-cos buffer launches nothing in backward) and
    written into the parameter's gradient slot when it has one."""

    @staticmethod
    def forward(ctx, x, pos):
        ctx.small = (pos,)
        return ops.pos_embed_fwd(_c(x), pos)

    @staticmethod
    def backward(ctx, dy):
        pos = ctx.small[0]
        if not getattr(ctx, "needs_input_grad", (True, True))[1]:
            return dy, None
        slot = _slot(pos)
        dpos = ops.pos_embed_bwd(_c(dy), out=slot)
        return dy, (dpos if slot is not None else dpos.to(_BF16).view(pos.shape))


def _pos_table(x, pos):
    if x.dim() != 3 or pos.dim() not in (2, 3) or (pos.dim() == 3 and pos.shape[0] != 1) or pos.shape[-1] != x.shape[-1]:
        raise ValueError(f"pos_embed: x [B, N, D] and a table [N, D] or [1, N, D] expected, got {tuple(x.shape)} and {tuple(pos.shape)}")
    if pos.shape[-2] != x.shape[1]:
        raise ValueError(f"pos_embed: the activation has {x.shape[1]} tokens and the table {pos.shape[-2]}")


def pos_embed(x, pos):
    """x [B, N, D] + pos ([1, N, D] or [N, D]) -> [B, N, D] bf16: the positional table added to every image."""
    _pos_table(x, pos)
    if _traced():
        from . import library
        return library.pos_embed(_bf(x), _c(_bf(pos)))
    return _PosEmbed.apply(_bf(x), _c(_bf(pos)))


# ----------------------------------------------------------------------------
class _ClsPrepend(Function):
    """cat([cls, x], dim=1) (src/models/vit.py:237-238, commented out there).  dx is dy without its first row; the token's
    gradient is the batch sum of that row, written into the parameter's gradient slot when it has one."""

    @staticmethod
    def forward(ctx, x, cls):
        ctx.small = (cls,)
        return ops.cls_prepend_fwd(_c(x), cls)

    @staticmethod
    def backward(ctx, dy):
        cls = ctx.small[0]
        need = getattr(ctx, "needs_input_grad", (True, True))
        if not need[1]:
            return dy[:, 1:], None
        slot = _slot(cls)
        dx, dcls = ops.cls_prepend_bwd(_c(dy), want_dx=need[0], out=slot)
        return dx, (dcls if slot is not None else dcls.to(_BF16).view(cls.shape))


def cls_prepend(x, cls):
    """x [B, N, D], cls ([1, 1, D] or [D]) -> [B, N + 1, D] bf16 with the token in front of every image's sequence."""
    if x.dim() != 3 or cls.numel() != x.shape[-1] or tuple(cls.shape) not in ((x.shape[-1],), (1, 1, x.shape[-1])):
        raise ValueError(f"cls_prepend: x [B, N, D] and a token [D] or [1, 1, D] expected, got {tuple(x.shape)} and {tuple(cls.shape)}")
    if _traced():
        from . import library
        return library.cls_prepend(_bf(x), _c(_bf(cls)))
    return _ClsPrepend.apply(_bf(x), _c(_bf(cls)))


class _TokenPool(Function):
    """Mean over a token range (count = 1: the row itself).  Backward writes every element of dx: the gradient over the
    range, +0 outside it."""

    @staticmethod
    def forward(ctx, x, first, count):
        ctx.geom = (x.shape[1], first, count)
        return ops.token_pool_fwd(_c(x), first, count)

    @staticmethod
    def backward(ctx, dy):
        T, first, count = ctx.geom
        return ops.token_pool_bwd(_c(dy), T, first, count), None, None


def token_pool(x, first=0, count=None):
    """x [B, T, D] -> [B, D] bf16: the mean of tokens [first, first + count) (count = None: to the last token); count = 1
    reads one token, bit for bit -- token_pool(x, 0, 1) is the CLS read-out."""
    if x.dim() != 3:
        raise ValueError(f"token_pool: x [B, T, D] expected, got {tuple(x.shape)}")
    first, count = ops._pool_range(x.shape[1], first, count)
    if _traced():
        from . import library
        return library.token_pool(_bf(x), first, count)
    return _TokenPool.apply(_bf(x), first, count)


def pooled_head(x, ln_w, ln_b, w, b, eps=1e-5):
    """LayerNorm(D) + Linear(D, classes) on a pooled token x [B, D]: layer_norm and linear as they are; one traceable op
    under torch.compile."""
    if _traced():
        from . import library
        return library.pooled_head(_bf(x), _bf(ln_w), _bf(ln_b), _bf(w), _bf(b), eps)
    return linear(layer_norm(x, ln_w, ln_b, eps), w, b)


# ----------------------------------------------------------------------------
# The two encoder layers (post-norm _EncoderLayer, pre-norm _PreNormLayer) are "residual site + the LayerNorm after it", twice,
# around one attention core (_attn_fwd / _attn_bwd above) and one MLP: the pieces below, shared by both.
# ----------------------------------------------------------------------------
class _LayerCfg:
    """The non-tensor arguments of _EncoderLayer and _PreNormLayer, one object so that apply() has a fixed argument list.
    seeds: the four dropout seeds (attention, dropout1, the MLP's, dropout2); drop_path: None or (rate, (seed1, seed2))."""

    def __init__(self, n_heads, eps, p, seeds, scale, act, attn_mask=None, drop_path=None, rel_index=None, qk_eps=1e-6, rope=None):
        self.n_heads, self.eps, self.p, self.seeds, self.scale, self.act = n_heads, eps, p, seeds, scale, act
        self.attn_mask, self.drop_path, self.rel_index, self.qk_eps = attn_mask, drop_path, rel_index, qk_eps
        self.rope = rope                                        # None or an ops.RopeTable: not differentiable, like the mask


_PreNormCfg = _LayerCfg     # the name callers that build a _PreNormLayer by hand knew it by: same constructor


def _site_fwd(branch_in, w, b, res, lam_row, g_w, g_b, B, eps, p, seed, drop_path, site):
    """One residual site + the LayerNorm after it -> (branch or None, s, n, mean, rstd).  Which kernels it runs:
      no lam, no drop_path   the branch GEMM's residual= epilogue + ops.layernorm_fwd
      drop_path alone        the branch GEMM stores drop(a) without the residual; ops.add_layernorm_path_fwd adds, rounds once, normalises
      lam                    the same with ops.add_layernorm_scale_fwd; the branch is returned (the backward needs it for dlam)"""
    if lam_row is None and drop_path is None:
        s = ops.gemm(branch_in, w, bias=b, residual=res, dropout_p=p, dropout_seed=seed)
        return (None, s) + tuple(ops.layernorm_fwd(s, g_w, g_b, eps))
    a = ops.gemm(branch_in, w, bias=b, dropout_p=p, dropout_seed=seed)
    rate, pseed = (drop_path[0], drop_path[1][site]) if drop_path is not None else (0.0, 0)
    if lam_row is None:
        return (None,) + tuple(ops.add_layernorm_path_fwd(a, res, g_w, g_b, B, rate, pseed, eps))
    return (a,) + tuple(ops.add_layernorm_scale_fwd(a, res, lam_row, g_w, g_b, B, rate, pseed, eps))


def _site_bwd(dyv, sv, mean, rstd, g_w, g_b, prev_bias, N, p, seed, drop_path, site, add=None, branch=None, lam_row=None, lam_out=None):
    """The LayerNorm backward after a site -> (gradient of s, dgamma, dbeta, gradient entering the branch, column sums of that =
    the bias gradient of linear2 / out_proj, for free in the same pass; dlam or None).  It applies the site's dropout mask and
    DropPath flag (riding on the dropout multiplier) to the gradient it hands the branch and adds `add`, the gradient of s arriving
    on the residual path:  ops.layernorm_bwd / ops.layernorm_bwd_path / with lam_row ops.layernorm_bwd_scale (branch: the site's
    stored branch).  Gradients go straight into their slots when every parameter of the call has one (lam_out: the site's row of
    the LayerScale parameter's slot, or None)."""
    slots = (_slot(g_w), _slot(g_b), _slot(prev_bias))
    ok = all(t is not None for t in slots) and (lam_row is None or lam_out is not None)
    go = slots if ok else None
    dl = None
    if lam_row is not None:
        if ok:
            lam_out._sfcvit_deferrable = True
            go = slots + (lam_out,)
        rate, pseed = (drop_path[0], drop_path[1][site]) if drop_path is not None else (0.0, 0)
        dsv, dg, dbt, dsub, dl, dcol = ops.layernorm_bwd_scale(dyv, sv, mean, rstd, g_w, branch, lam_row, N, rate, pseed, dx_add=add,
                                                               drop_p=p, drop_seed=seed, want_colsum=True, grad_out=go)
    elif drop_path is not None:
        dsv, dg, dbt, dsub, dcol = ops.layernorm_bwd_path(dyv, sv, mean, rstd, g_w, N, drop_path[0], drop_path[1][site], dx_add=add,
                                                          drop_p=p, drop_seed=seed, want_colsum=True, grad_out=go)
    elif p > 0:
        dsv, dg, dbt, dsub, dcol = ops.layernorm_bwd(dyv, sv, mean, rstd, g_w, dx_add=add, drop_p=p, drop_seed=seed, want_colsum=True,
                                                     grad_out=go)
    else:
        dsv, dg, dbt, dcol = ops.layernorm_bwd(dyv, sv, mean, rstd, g_w, dx_add=add, want_colsum=True, grad_out=go)
        dsub = dsv
    if not ok:
        dg, dbt, dcol = dg.to(_BF16), dbt.to(_BF16), dcol.to(_BF16)
    return dsv, dg, dbt, dsub, dcol, dl


def _mlp_fwd(n1, w1, b1, act, p, seed):
    """h = drop(act(W1 n1 + b1)) -> (hbits, u, h).  relu: one GEMM; the dX GEMM through ReLU + dropout needs only the sign
    pattern of h, a bit matrix hbits written by linear1's epilogue (19 MB instead of 308 MB per ViT-B layer read back in
    backward; sfcvit_gemm_args.actmask).  gelu (erf): _Mixer's recipe, the pre-activation u from the GEMM and one element-wise
    pass with the dropout."""
    if act == "relu":
        hbits = (torch.empty((n1.shape[0], w1.shape[0] // 8), device=n1.device, dtype=torch.uint8)
                 if USE_ACTMASK and w1.shape[0] % 16 == 0 else None)
        return hbits, None, ops.gemm(n1, w1, bias=b1, act=ops.ACT_RELU, dropout_p=p, dropout_seed=seed, actmask=hbits)
    u = ops.gemm(n1, w1, bias=b1)
    return None, u, (ops.gelu_drop_fwd(u, p, seed) if p > 0 else ops.gelu_fwd(u))


def _mlp_bwd(df, h, u, hbits, w2, b1, act, p, seed):
    """df = the gradient of linear2's output -> (dh, the gradient of linear1's output; db1, in b1's slot when it has one)."""
    b1_slot = _slot(b1)
    if act == "relu":
        # h is stored after relu + dropout: (h > 0) is the joint mask, 1/(1-p) the dropout scale; b1's gradient is the column
        # sum of dh, fused into that GEMM's epilogue
        dh, db1 = ops.gemm_dx(df, w2, aux_in=h, dact=ops.ACT_RELU, dact_scale=1.0 / (1.0 - p),
                              colsum=b1_slot if b1_slot is not None else True, actmask=hbits)
        return dh, (db1 if b1_slot is not None else db1.to(_BF16))
    dh = ops.gemm_dx(df, w2)
    dh = ops.gelu_drop_bwd(dh, u, p, seed) if p > 0 else ops.gelu_bwd(dh, u)
    return dh, (ops.colsum(dh, out=b1_slot) if b1_slot is not None else ops.colsum(dh).to(_BF16))


def _wgrad_runner(device):
    """(wg, join): wg(dy2, x2, w) = _wgrad, on the side stream with SFCVIT_SIDE_STREAM=1; join(*dws) before they are returned."""
    if not SIDE_STREAM_WGRAD:
        return _wgrad, lambda *dws: None
    ss = _SideStream(device)
    return (lambda a_, b_, w_: ss.run(lambda: _wgrad(a_, b_, w_), a_, b_)), ss.join


class _EncoderLayer(Function):
    """Post-norm transformer encoder layer (torch:nn/modules/transformer.py:951-982):
         a  = out_proj(attention(in_proj(x)));  x1 = LN1(x + drop1(a))
         f  = W2 drop(relu(W1 x1 + b1)) + b2;   y  = LN2(x1 + drop2(f))
    with dropout p on the attention probabilities as well.  p = 0 (eval) makes every mask the
    identity.  Masks are functions of (seed, element index), regenerated in backward.
    cfg.drop_path = (rate, (seed1, seed2)), rate > 0: stochastic depth on the two residual sites,
         x1 = LN1(x + c1[b] drop1(a));  y = LN2(x1 + c2[b] drop2(f)),  c[b] = keep[b] / (1 - rate), one flag per image and site
    (functions of (seed, image index), regenerated in backward): _site_fwd's second form.  Arguments: the 13 tensors, the bias
    table parameter (None without cfg.rel_index), a _LayerCfg (act "relu")."""

    @staticmethod
    def launches(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, rel_bias, cfg, qk=None):
        """The forward's kernel launches, every intermediate returned (forward saves them; encoder_layer_probe reads the
        attention inputs out of the same sequence, so what it carries on is what forward computes)."""
        B, N, D = x.shape
        Da = in_w.shape[0] // 3                             # attention width: D, or n_heads * padded head dim (encoder_layer)
        p = cfg.p
        sa, s1_, sf, s2_ = cfg.seeds
        x2 = _c(x).view(B * N, D)
        qkv = ops.gemm(x2, in_w, bias=in_b)
        raw = _qk_norm_fwd(qkv, qk, cfg)
        _rope_fwd(qkv, cfg)
        o, lse = _attn_fwd(qkv.view(B, N, 3 * Da), cfg.n_heads, p, sa, cfg.scale, cfg.attn_mask, rel_bias)
        _, s1, x1, mean1, rstd1 = _site_fwd(o.view(B * N, Da), out_w, out_b, x2, None, n1_w, n1_b, B, cfg.eps, p, s1_, cfg.drop_path, 0)
        hbits, _, h = _mlp_fwd(x1, w1, b1, cfg.act, p, sf)
        _, s2, y, mean2, rstd2 = _site_fwd(h, w2, b2, x1, None, n2_w, n2_b, B, cfg.eps, p, s2_, cfg.drop_path, 1)
        return dict(x2=x2, qkv=qkv, raw=raw, o=o, lse=lse, s1=s1, mean1=mean1, rstd1=rstd1, x1=x1, hbits=hbits, h=h, s2=s2, y=y, mean2=mean2,
                    rstd2=rstd2)

    @staticmethod
    def forward(ctx, x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, rel_table, cfg, qk=None):
        rel_bias = _fp32_bias(rel_table, cfg.rel_index)
        t = _EncoderLayer.launches(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, rel_bias, cfg, qk)
        ctx.cfg, ctx.shape, ctx.rel_bias, ctx.rel_table, ctx.hbits = cfg, tuple(x.shape), rel_bias, rel_table, t["hbits"]
        ctx.small = (in_b, out_b, n1_b, b1, b2, n2_b)      # parameters only needed for their gradient slots
        ctx.qk_param = qk                                   # QK-norm: for its gradient slot; raw q | k and qk are saved last
        opt = [t["raw"], qk] if qk is not None else []
        ctx.save_for_backward(t["x2"], t["qkv"], t["o"], t["lse"], t["s1"], t["mean1"], t["rstd1"], t["x1"], t["h"], t["s2"],
                              t["mean2"], t["rstd2"], in_w, out_w, n1_w, w1, w2, n2_w, *opt)
        return t["y"].view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (x2, qkv, o, lse, s1, mean1, rstd1, x1, h, s2, mean2, rstd2,
         in_w, out_w, n1_w, w1, w2, n2_w, *opt) = ctx.saved_tensors
        raw, qk = opt if opt else (None, None)
        cfg = ctx.cfg
        B, N, D = ctx.shape
        p, drop_path = cfg.p, cfg.drop_path
        sa, s1_, sf, s2_ = cfg.seeds
        dy2 = _c(dy).view(B * N, D)
        in_b, out_b, n1_b, b1, b2, n2_b = ctx.small
        wg, join = _wgrad_runner(dy2.device)
        ds2, dg2, dbt2, df, db2, _ = _site_bwd(dy2, s2, mean2, rstd2, n2_w, n2_b, b2, N, p, s2_, drop_path, 1)
        dw2 = wg(df, h, w2)
        dh, db1 = _mlp_bwd(df, h, None, ctx.hbits, w2, b1, cfg.act, p, sf)
        dw1 = wg(dh, x1, w1)
        dx1 = ops.gemm_dx(dh, w1, residual=ds2)
        ds1, dg1, dbt1, da, dbo, _ = _site_bwd(dx1, s1, mean1, rstd1, n1_w, n1_b, out_b, N, p, s1_, drop_path, 0)
        Da = in_w.shape[0] // 3
        dwo = wg(da, o.view(B * N, Da), out_w)
        do = ops.gemm_dx(da, out_w)
        want = ctx.rel_bias is not None and ctx.needs_input_grad[13]        # a frozen table costs nothing
        dqkv, dbi, dtable, dqk = _qk_norm_bwd(_rope_bwd(
            lambda fp32: _attn_bwd(qkv.view(B, N, 3 * Da), o, lse, do.view(B, N, Da), cfg.n_heads, p, sa, cfg.scale, cfg.attn_mask,
                                   ctx.rel_bias, True, in_b, ctx.rel_table, want, fp32), in_b, cfg), raw, qk, getattr(ctx, "qk_param", None), in_b, cfg)
        dqkv = dqkv.view(B * N, 3 * Da)
        dwi = wg(dqkv, x2, in_w)
        dx = ops.gemm_dx(dqkv, in_w, residual=ds1)
        join(dw2, dw1, dwo, dwi)
        return dx.view(B, N, D), dwi, dbi, dwo, dbo, dg1, dbt1, dw1, db1, dw2, db2, dg2, dbt2, dtable, None, dqk


def _encoder_layer_args(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, n_heads):
    """bf16 arguments of _EncoderLayer and its softmax scale (None = 1 / sqrt(kernel head dim)), the per-head zero
    padding of encoder_layer applied."""
    args = [_bf(t) for t in (x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b)]
    D = args[0].shape[-1]
    hd, hp = _head_padding(D, n_heads)
    scale = None
    if hp != hd:
        pad = torch.nn.functional.pad
        args[1] = pad(args[1].reshape(3, n_heads, hd, D), (0, 0, 0, hp - hd)).reshape(3 * n_heads * hp, D)
        if args[2] is not None:
            args[2] = pad(args[2].reshape(3, n_heads, hd), (0, hp - hd)).reshape(3 * n_heads * hp)
        args[3] = pad(args[3].reshape(D, n_heads, hd), (0, hp - hd)).reshape(D, n_heads * hp)
        scale = 1.0 / math.sqrt(hd)
    return args, scale


def encoder_layer_probe(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, n_heads, eps=1e-5, qk_norm=None,
                        qk_norm_eps=1e-6, rope=None):
    """The eval-mode (dropout 0) encoder layer with its attention inputs exposed: (y, qkv [B, N, 3 * H * kernel head dim],
    lse [B, H, N], softmax scale or None).  Same launches as encoder_layer(dropout_p=0): y has its bits.  With qk_norm the
    qkv returned is the NORMALISED one, with rope the ROTATED one: what the attention kernels consumed.  For sfcvit.analysis; no
    autograd graph is built."""
    with torch.no_grad():
        args, scale = _encoder_layer_args(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, n_heads)
        B, N, D = args[0].shape
        qk, qk_eps = _qk_norm_arg(qk_norm, qk_norm_eps, D // n_heads, "encoder_layer_probe")
        rope = _rope_arg(rope, N, D // n_heads, "encoder_layer_probe")
        t = _EncoderLayer.launches(*args, None, _LayerCfg(n_heads, eps, 0.0, (0, 0, 0, 0), scale, "relu", qk_eps=qk_eps, rope=rope), qk)
        return t["y"].view(B, N, D), t["qkv"].view(B, N, -1), t["lse"], scale


def _path_rate(what, drop_path):
    """A layer call's drop_path as a float in [0, 1): checked first, before the tensors are looked at."""
    drop_path = float(drop_path)
    if not 0.0 <= drop_path < 1.0:
        raise ValueError(f"{what}: drop_path={drop_path} outside [0, 1)")
    return drop_path


def _layer_options(what, n_tokens, n_heads, attn_mask, rel_bias, no_traced_form=None):
    """The attention options both layers take, checked -> (ops.AttentionMask or None, (table, ops.AttentionBiasIndex) or None).
    no_traced_form: a layer without a traced form says so here: after the bias refusals, before the mask's."""
    rel_bias = _rel_bias(rel_bias, attn_mask, n_tokens, n_heads, what)
    if no_traced_form is not None and _traced():
        raise NotImplementedError(f"{what}: {no_traced_form}")
    return _attention_mask(attn_mask, n_tokens, what), rel_bias


def _layer_cfg(n_heads, eps, dropout_p, scale, act, attn_mask, drop_path, rel_bias, qk_eps=1e-6, rope=None):
    """An eager layer call's (_LayerCfg, bias table or None).  The seeds are drawn here, on the host, in this order: four dropout
    seeds when dropout_p > 0, then two path seeds when drop_path > 0.  (QK-norm and RoPE draw nothing.)"""
    seeds = tuple(ops.next_seed() for _ in range(4)) if dropout_p > 0 else (0, 0, 0, 0)
    path = (drop_path, (ops.next_seed(), ops.next_seed())) if drop_path > 0 else None
    table, index = rel_bias if rel_bias is not None else (None, None)
    return _LayerCfg(n_heads, eps, float(dropout_p), seeds, scale, act, attn_mask, path, index, qk_eps, rope), table


def encoder_layer(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, n_heads, eps=1e-5,
                  dropout_p=0.0, attn_mask=None, drop_path=0.0, rel_bias=None, qk_norm=None, qk_norm_eps=1e-6, rope=None):
    """dropout_p > 0 = training-mode nn.TransformerEncoderLayer (fresh masks every call).
    attn_mask = nn.TransformerEncoderLayer's src_mask: None, or an additive [N, N] mask as in `attention` (build an
    ops.AttentionMask once when the layer runs more than once).  With None the launches and the bits are those of a call
    without the argument; with a mask the attention core alone changes, to the masked kernels (not under tracing).
    A head dim the attention kernels do not have (embed_dim / n_heads = 32, 48, 96, ...) runs on the next one that
    exists: in_proj's rows and out_proj's columns are zero-padded per head (differentiable torch plumbing on the
    weights, 3 D^2 elements -- not on the activations), so q, k, v come out of the projection GEMM already padded, the
    padded columns add nothing to q k^T or p v, and out_proj ignores them; the softmax scale stays 1 / sqrt(head dim).
    drop_path = r in (0, 1): stochastic depth for a layer in TRAINING mode (the caller passes 0 in eval, as it passes
    dropout_p = 0): each of the two residual branches is dropped per image with probability r and scaled by 1 / (1 - r)
    otherwise, the two sites drawing independently (timm's drop_path1 / drop_path2, scale_by_keep=True).  0 runs the launches
    and gives the bits of a call without the argument.  Not under tracing.
    rel_bias = (table [H, T] -- a parameter in any float dtype --, ops.AttentionBiasIndex): a learned relative position bias
    per head on the attention scores, softmax(q k^T / sqrt(hd) + table[h, index[i, j]]), with dropout as without it; the
    attention core alone changes, to the bias kernels, and the table receives its gradient (in its dtype, in its gradient
    slot when it has one).  Not with attn_mask (a window is part of the index: sfcvit.relpos), not under tracing; None
    runs the call as it is without the argument.
    qk_norm = a [4, head_dim] tensor, rows q_weight, q_bias, k_weight, k_bias (timm's attn.q_norm / attn.k_norm, shared by all
    heads; head_dim = embed_dim / n_heads, not the padded one): QK-norm, a LayerNorm(head_dim, eps=qk_norm_eps) on the queries
    and keys of every head before q k^T, one in-place kernel between the projection GEMM and the attention core and its mirror
    in the backward; the softmax scale, mask, bias and dropout are untouched and the tensor receives its gradient (in its slot
    when it has one).  Combines with every other option; not under tracing.  None runs the call as it is without the argument.
    rope = an ops.RopeTable (or a CPU fp32 [N, head_dim / 2, 2] table; sfcvit.rope builds them): rotary position embedding, the
    channel pairs of the queries and keys of every head rotated by the table's (cos, sin) of their token, after QK-norm and
    before q k^T; one in-place kernel and its transposed mirror in the backward, nothing saved, no gradient to the table.
    Needs an even head_dim.  Combines with every other option; not under tracing.  None runs the call as it is without it."""
    drop_path = _path_rate("encoder_layer", drop_path)
    args, scale = _encoder_layer_args(x, in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b, n_heads)
    qk, qk_eps = _qk_norm_arg(qk_norm, qk_norm_eps, args[0].shape[-1] // n_heads, "encoder_layer")
    rope = _rope_arg(rope, args[0].shape[1], args[0].shape[-1] // n_heads, "encoder_layer")
    attn_mask, rel_bias = _layer_options("encoder_layer", args[0].shape[1], n_heads, attn_mask, rel_bias)
    if drop_path > 0 and _traced():
        raise NotImplementedError("encoder_layer: drop_path > 0 has no traced form (torch.compile); run the layer eagerly")
    if _traced():
        from . import library      # (dropout seeds are drawn inside the op: nothing data-dependent in the traced graph)
        return library.encoder_layer(args, n_heads, eps, float(dropout_p), scale)
    cfg, table = _layer_cfg(n_heads, eps, dropout_p, scale, "relu", attn_mask, drop_path, rel_bias, qk_eps, rope)
    return _EncoderLayer.apply(*args, table, cfg) if qk is None else _EncoderLayer.apply(*args, table, cfg, qk)


# ----------------------------------------------------------------------------
class _PreNormLayer(Function):
    """Pre-norm transformer encoder layer (torch:nn/modules/transformer.py, norm_first=True) as "residual site + the LayerNorm
    after it", twice.  In: the residual stream s and n = LN1(s).  Out: s' and n' = LN_next(s'), LN_next being the next layer's
    norm1 or the encoder's final norm:
         a  = drop1(out_proj(attention(in_proj(n))));    s1 = s  + c1[b] lam1 * a;   n1 = LN2(s1)
         f  = drop2(W2 drop(act(W1 n1 + b1)) + b2);      s' = s1 + c2[b] lam2 * f;   n' = LN_next(s')
    cfg.act is ReLU or erf-GELU (_mlp_fwd); lam = None is no LayerScale, cfg.drop_path = None no stochastic depth (_site_fwd /
    _site_bwd: which kernels a site runs).  Arguments: s, n, the 12 parameters, lam [2, D] or None, the bias table parameter or
    None, a _LayerCfg."""

    @staticmethod
    def launches(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, nf_w, nf_b, lam, rel_bias, cfg, qk=None):
        """The forward's kernel launches, every intermediate returned (forward saves them; pre_norm_layer_probe reads the attention
        inputs out of the same sequence)."""
        B, N, D = s.shape
        Da = in_w.shape[0] // 3
        p = cfg.p
        sa, s1_, sf, s2_ = cfg.seeds
        s0, n0 = _c(s).view(B * N, D), _c(n).view(B * N, D)
        qkv = ops.gemm(n0, in_w, bias=in_b)
        raw = _qk_norm_fwd(qkv, qk, cfg)
        _rope_fwd(qkv, cfg)
        o, lse = _attn_fwd(qkv.view(B, N, 3 * Da), cfg.n_heads, p, sa, cfg.scale, cfg.attn_mask, rel_bias)
        lam1, lam2 = (lam[0], lam[1]) if lam is not None else (None, None)
        a, s1, n1, mean1, rstd1 = _site_fwd(o.view(B * N, Da), out_w, out_b, s0, lam1, n2_w, n2_b, B, cfg.eps, p, s1_, cfg.drop_path, 0)
        hbits, u, h = _mlp_fwd(n1, w1, b1, cfg.act, p, sf)
        f, s2, n2, mean2, rstd2 = _site_fwd(h, w2, b2, s1, lam2, nf_w, nf_b, B, cfg.eps, p, s2_, cfg.drop_path, 1)
        return dict(n0=n0, qkv=qkv, raw=raw, o=o, lse=lse, a=a, s1=s1, n1=n1, mean1=mean1, rstd1=rstd1, hbits=hbits, u=u, h=h, f=f, s2=s2,
                    n2=n2, mean2=mean2, rstd2=rstd2)

    @staticmethod
    def forward(ctx, s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, nf_w, nf_b, lam, rel_table, cfg, qk=None):
        B, N, D = s.shape
        rel_bias = _fp32_bias(rel_table, cfg.rel_index)
        t = _PreNormLayer.launches(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, nf_w, nf_b, lam, rel_bias, cfg, qk)
        ctx.qk_param = qk                                       # QK-norm: for its gradient slot; raw q | k and qk are saved last
        ctx.cfg, ctx.shape, ctx.rel_bias, ctx.rel_table, ctx.hbits = cfg, (B, N, D), rel_bias, rel_table, t["hbits"]
        ctx.lam_param = lam                                     # for its gradient slot: both rows are written in one backward
        ctx.small = (in_b, out_b, n2_b, b1, b2, nf_b)          # parameters only needed for their gradient slots
        ctx.has = tuple(t[k] is not None for k in ("a", "u", "f"))
        ctx.has_lam = lam is not None
        opt = [t[k] for k in ("a", "u", "f") if t[k] is not None] + ([lam] if lam is not None else [])
        opt += [t["raw"], qk] if qk is not None else []
        ctx.save_for_backward(t["n0"], t["qkv"], t["o"], t["lse"], t["s1"], t["n1"], t["mean1"], t["rstd1"], t["h"], t["s2"],
                              t["mean2"], t["rstd2"], in_w, out_w, n2_w, w1, w2, nf_w, *opt)
        ctx.set_materialize_grads(False)
        return t["s2"].view(B, N, D), t["n2"].view(B, N, D)

    @staticmethod
    def backward(ctx, ds_out, dn_out):
        (n0, qkv, o, lse, s1, n1, mean1, rstd1, h, s2, mean2, rstd2, in_w, out_w, n2_w, w1, w2, nf_w, *opt) = ctx.saved_tensors
        opt = list(opt)
        a, u, f = (opt.pop(0) if has else None for has in ctx.has)
        lam = opt.pop(0) if ctx.has_lam else None
        raw, qk = opt if opt else (None, None)
        cfg = ctx.cfg
        B, N, D = ctx.shape
        p, drop_path = cfg.p, cfg.drop_path
        sa, s1_, sf, s2_ = cfg.seeds
        in_b, out_b, n2_b, b1, b2, nf_b = ctx.small
        ds_out = None if ds_out is None else _c(ds_out).view(B * N, D)
        dn_out = torch.zeros_like(s2) if dn_out is None else _c(dn_out).view(B * N, D)
        wg, join = _wgrad_runner(dn_out.device)
        lam_slot = _slot(ctx.lam_param) if lam is not None else None
        lam1, lam2 = (lam[0], lam[1]) if lam is not None else (None, None)
        out1, out2 = (lam_slot[0], lam_slot[1]) if lam_slot is not None else (None, None)
        ds2, dgf, dbtf, df, db2, dlam2 = _site_bwd(dn_out, s2, mean2, rstd2, nf_w, nf_b, b2, N, p, s2_, drop_path, 1, ds_out, f, lam2, out2)
        dw2 = wg(df, h, w2)
        dh, db1 = _mlp_bwd(df, h, u, ctx.hbits, w2, b1, cfg.act, p, sf)
        dw1 = wg(dh, n1, w1)
        dn1 = ops.gemm_dx(dh, w1)
        ds1, dg2, dbt2, da, dbo, dlam1 = _site_bwd(dn1, s1, mean1, rstd1, n2_w, n2_b, out_b, N, p, s1_, drop_path, 0, ds2, a, lam1, out1)
        Da = in_w.shape[0] // 3
        dwo = wg(da, o.view(B * N, Da), out_w)
        do = ops.gemm_dx(da, out_w)
        want = ctx.rel_bias is not None and ctx.needs_input_grad[15]        # a frozen table costs nothing
        dqkv, dbi, dtable, dqk = _qk_norm_bwd(_rope_bwd(
            lambda fp32: _attn_bwd(qkv.view(B, N, 3 * Da), o, lse, do.view(B, N, Da), cfg.n_heads, p, sa, cfg.scale, cfg.attn_mask,
                                   ctx.rel_bias, True, in_b, ctx.rel_table, want, fp32), in_b, cfg), raw, qk, getattr(ctx, "qk_param", None), in_b, cfg)
        dqkv = dqkv.view(B * N, 3 * Da)
        dwi = wg(dqkv, n0, in_w)
        dn_in = ops.gemm_dx(dqkv, in_w)
        join(dw2, dw1, dwo, dwi)
        if lam is None:
            dl = None
        elif lam_slot is not None and all(d.dtype == _BF16 and d.data_ptr() == r.data_ptr() for d, r in ((dlam1, out1), (dlam2, out2))):
            dl = lam_slot                                       # both rows were written in place
        else:
            if lam_slot is not None:                            # one row sits in the slot, its reduction perhaps still queued
                ops.flush_deferred(end=False)
            dl = torch.stack([dlam1.to(_BF16), dlam2.to(_BF16)])
        return (ds1.view(B, N, D), dn_in.view(B, N, D), dwi, dbi, dwo, dbo, dg2, dbt2, dw1, db1, dw2, db2, dgf, dbtf, dl, dtable, None, dqk)


def _layer_scale_arg(layer_scale, D, what):
    """layer_scale = None, (lam1, lam2) with [D] each, or one [2, D] tensor (row 0: the attention branch) -> bf16 [2, D] or None.
    A [2, D] bf16 parameter passes as it is, so its gradient can be written into its slot."""
    if layer_scale is None:
        return None
    if isinstance(layer_scale, (tuple, list)):
        if len(layer_scale) != 2 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != (D,) for t in layer_scale):
            raise ValueError(f"{what}: layer_scale must be (lam1, lam2) with [D] = [{D}] each, or one [2, D] tensor")
        layer_scale = torch.stack([_bf(layer_scale[0]), _bf(layer_scale[1])])
    if not isinstance(layer_scale, torch.Tensor) or tuple(layer_scale.shape) != (2, D):
        raise ValueError(f"{what}: layer_scale must be (lam1, lam2) with [D] = [{D}] each, or one [2, D] tensor")
    return _c(_bf(layer_scale))


def _check_pre_norm_width(D, what="pre_norm_layer"):
    if D % 8 or D > 2048:
        raise ValueError(f"{what}: width {D} is not supported by the pre-norm kernels (a multiple of 8, at most 2048)")


def _pre_norm_args(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, next_w, next_b, n_heads, activation, layer_scale, what):
    if activation not in ("relu", "gelu"):
        raise ValueError(f"{what}: activation={activation!r} (relu or gelu)")
    if tuple(n.shape) != tuple(s.shape) or s.dim() != 3:
        raise ValueError(f"{what}: s and n = LayerNorm(s) must be equal [B, N, D], got {tuple(s.shape)} and {tuple(n.shape)}")
    _check_pre_norm_width(s.shape[-1], what)
    args, scale = _encoder_layer_args(s, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, next_w, next_b, n_heads)
    return args, scale, _bf(n), _layer_scale_arg(layer_scale, s.shape[-1], what)


def pre_norm_layer(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, next_w, next_b, n_heads, eps=1e-5, dropout_p=0.0,
                   attn_mask=None, drop_path=0.0, rel_bias=None, activation="relu", layer_scale=None, qk_norm=None, qk_norm_eps=1e-6,
                   rope=None):
    """One pre-norm encoder layer (nn.TransformerEncoderLayer(norm_first=True)) on the HIP path, as "residual site + the
    LayerNorm after it": takes the residual stream s [B, N, D] and n = norm1(s), returns (s', n') with n' = LayerNorm(s') by
    the FOLLOWING norm (next_w, next_b): the next layer's norm1, or the encoder's final norm after the last layer.  The first
    layer's n comes from layer_norm(s, norm1).  n2_w / n2_b are the layer's own norm2.
    activation: "relu" or "gelu" (erf).  layer_scale: None, or (lam1, lam2) / a [2, D] tensor: the per-channel scales of the
    attention and MLP branches (CaiT / DeiT-III), s1 = s + c1[b] lam1 * a.  dropout_p, attn_mask, drop_path, rel_bias and the
    zero padding of head dims the kernels do not have: as in encoder_layer, with its masks, flags and seeds; qk_norm, qk_norm_eps
    (QK-norm) and rope (rotary position embedding) as there too.  Not under tracing."""
    what = "pre_norm_layer"
    drop_path = _path_rate(what, drop_path)
    args, scale, n, lam = _pre_norm_args(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, next_w, next_b, n_heads,
                                         activation, layer_scale, what)
    qk, qk_eps = _qk_norm_arg(qk_norm, qk_norm_eps, args[0].shape[-1] // n_heads, what)
    rope = _rope_arg(rope, args[0].shape[1], args[0].shape[-1] // n_heads, what)
    attn_mask, rel_bias = _layer_options(what, args[0].shape[1], n_heads, attn_mask, rel_bias,
                                         no_traced_form="the pre-norm layer has no traced form (torch.compile); run the model eagerly")
    cfg, table = _layer_cfg(n_heads, eps, dropout_p, scale, activation, attn_mask, drop_path, rel_bias, qk_eps, rope)
    if qk is None:
        return _PreNormLayer.apply(args[0], n, *args[1:], lam, table, cfg)
    return _PreNormLayer.apply(args[0], n, *args[1:], lam, table, cfg, qk)


def pre_norm_layer_probe(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, next_w, next_b, n_heads, eps=1e-5,
                         activation="relu", layer_scale=None, qk_norm=None, qk_norm_eps=1e-6, rope=None):
    """The eval-mode (dropout 0) pre-norm layer with its attention inputs exposed: (s', n', qkv [B, N, 3 * H * kernel head dim],
    lse [B, H, N], softmax scale or None).  Same launches as pre_norm_layer(dropout_p=0): s' and n' have its bits.  With qk_norm
    the qkv returned is the NORMALISED one, with rope the ROTATED one: what the attention kernels consumed.  For sfcvit.analysis;
    no autograd graph is built."""
    with torch.no_grad():
        args, scale, n, lam = _pre_norm_args(s, n, in_w, in_b, out_w, out_b, n2_w, n2_b, w1, b1, w2, b2, next_w, next_b, n_heads,
                                             activation, layer_scale, "pre_norm_layer_probe")
        B, N, D = args[0].shape
        qk, qk_eps = _qk_norm_arg(qk_norm, qk_norm_eps, D // n_heads, "pre_norm_layer_probe")
        rope = _rope_arg(rope, N, D // n_heads, "pre_norm_layer_probe")
        cfg = _LayerCfg(n_heads, eps, 0.0, (0, 0, 0, 0), scale, activation, qk_eps=qk_eps, rope=rope)
        t = _PreNormLayer.launches(args[0], n, *args[1:], lam, None, cfg, qk)
        return t["s2"].view(B, N, D), t["n2"].view(B, N, D), t["qkv"].view(B, N, -1), t["lse"], scale


# ----------------------------------------------------------------------------
def _pad_rows(t, rows):
    if t.shape[0] == rows:
        return t
    out = torch.zeros((rows,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    out[: t.shape[0]] = t
    return out


class _Head(Function):
    """LN -> h = z W_emb^T -> y = <h, W_seq> -> GELU -> Dropout(p) -> classifier.
    The classifier is computed on a class count padded to a multiple of 8 (16-byte rows)."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w_emb, w_seq, wc, bc, eps, p, seed):
        B, N, D = x.shape
        R, O, C = w_emb.shape[0], w_seq.shape[0], wc.shape[0]
        x2 = _c(x).view(B * N, D)
        z, mean, rstd = ops.layernorm_fwd(x2, ln_w, ln_b, eps)
        h = ops.gemm(z, w_emb)                                      # [B*N, R]
        y1 = ops.gemm(h.view(B, N * R), w_seq.view(O, N * R))      # [B, O]
        a = ops.gelu_drop_fwd(y1, p, seed) if p > 0 else ops.gelu_fwd(y1)
        cpad = (C + 7) // 8 * 8
        wc_p, bc_p = _pad_rows(wc, cpad), _pad_rows(bc, cpad)
        logits = ops.gemm(a, wc_p, bias=bc_p)                       # [B, cpad]
        ctx.save_for_backward(x2, mean, rstd, z, h, y1, a, ln_w, w_emb, w_seq, wc_p)
        ctx.small = (ln_b, bc)
        ctx.dims = (B, N, D, R, O, C, cpad)
        ctx.p, ctx.seed = p, seed
        return logits[:, :C] if cpad != C else logits

    @staticmethod
    def backward(ctx, dlogits):
        x2, mean, rstd, z, h, y1, a, ln_w, w_emb, w_seq, wc_p = ctx.saved_tensors
        B, N, D, R, O, C, cpad = ctx.dims
        ln_b, bc = ctx.small
        if cpad == C:                                   # (wc_p IS the classifier weight then: gradients straight into the slots)
            dl = _c(dlogits)
            dwc, dbc = _wgrad(dl, a, wc_p), _bgrad(dl, bc)
        else:
            dl = torch.zeros((B, cpad), device=dlogits.device, dtype=_BF16)
            dl[:, :C] = dlogits
            dwc = ops.gemm(dl, a, a_kmajor=True, b_kmajor=True)[:C]
            dbc = ops.colsum(dl)[:C].to(_BF16)
        da = ops.gemm_dx(dl, wc_p)                      # [B, O]
        dy1 = ops.gelu_drop_bwd(da, y1, ctx.p, ctx.seed) if ctx.p > 0 else ops.gelu_bwd(da, y1)
        h2 = h.view(B, N * R)
        sseq = _slot(w_seq)
        dwseq = ops.gemm(dy1, h2, a_kmajor=True, b_kmajor=True, out=None if sseq is None else sseq.view(O, N * R))
        dwseq = dwseq.view(O, N, R) if sseq is None else sseq
        dh = ops.gemm(dy1, w_seq.view(O, N * R), b_kmajor=True).view(B * N, R)
        dwemb = _wgrad(dh, z, w_emb)
        dz = ops.gemm_dx(dh, w_emb)
        go = _ln_slots(ln_w, ln_b)
        dx, dg, dbeta = ops.layernorm_bwd(dz, x2, mean, rstd, ln_w, grad_out=go)
        return (dx.view(B, N, D), *_ln_grads(dg, dbeta, go), dwemb, dwseq, dwc, dbc, None, None, None)


def predictor_head(x, ln_w, ln_b, w_emb, w_seq, wc, bc, eps=1e-5, dropout_p=0.0):
    if _traced():
        from . import library
        return library.predictor_head(_bf(x), _bf(ln_w), _bf(ln_b), _bf(w_emb), _c(_bf(w_seq)), _bf(wc), _bf(bc), eps, float(dropout_p))
    seed = ops.next_seed() if dropout_p > 0 else 0
    return _Head.apply(_bf(x), _bf(ln_w), _bf(ln_b), _bf(w_emb), _c(_bf(w_seq)), _bf(wc), _bf(bc), eps,
                       float(dropout_p), seed)


# ----------------------------------------------------------------------------
class _SoftCE(Function):
    @staticmethod
    def forward(ctx, logits, targets):
        B, C = logits.shape
        base = _c(logits)                   # [B, C], row stride C (2-byte loads: no alignment needed)
        rows, dl = ops.soft_ce(base, _c(targets.float()), C, 1.0 / B)
        ctx.save_for_backward(dl)
        ctx.C = C
        return rows.mean()

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl[:, : ctx.C] * g.to(dl.dtype)), None


def soft_target_cross_entropy(logits, targets):
    """-(targets * log_softmax(logits)).sum(-1).mean() with the gradient produced in the same pass."""
    if _traced():
        from . import library
        return library.soft_ce(_bf(logits), targets)
    return _SoftCE.apply(_bf(logits), targets)


class _PairCE(Function):
    @staticmethod
    def forward(ctx, logits, y_a, y_b, mix):
        B, C = logits.shape
        rows, dl, hits = ops.soft_ce_pair(_c(logits), _c(y_a), _c(y_b), mix, C, 1.0 / B)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(hits)
        return rows.mean(), hits

    @staticmethod
    def backward(ctx, g, _ghits):
        (dl,) = ctx.saved_tensors
        return dl * g.to(dl.dtype), None, None, None


def mixed_target_cross_entropy(logits, y_a, y_b, mix):
    """soft_target_cross_entropy on lam * onehot(y_a) + (1 - lam) * onehot(y_b) without building the targets: lam comes
    from the batch mix's device record, the labels are int64 [B] on the device.  -> (loss, hit_rows) with
    hit_rows[b] = lam * (argmax == y_a) + (1 - lam) * (argmax == y_b), the loop's accuracy bookkeeping (train.py:171)."""
    return _PairCE.apply(_bf(logits), y_a, y_b, mix)


# ----------------------------------------------------------------------------
# torch.compile (main.py:284 wraps the model in torch.compile(mode="reduce-overhead")).  The blocks a VisionTransformer{,1D}
# is made of -- patch_embed, token_aggregator, pos_embed, cls_prepend, token_pool, pooled_head, token_mix, mixer_block, encoder_layer, predictor_head, soft_target_cross_entropy -- are registered as
# `sfcvit::` custom ops with fake kernels and autograd formulas (sfcvit/library.py) and take that path whenever Dynamo is
# tracing: the model compiles into ONE graph and "reduce-overhead" replays it from a hipGraph.  The remaining pieces
# (used by the hierarchical tokenizers, altvit and MultiLayerPredictor(n_layers > 2)) stay opaque: Dynamo breaks the graph
# around each and runs it as written.
# ----------------------------------------------------------------------------
for _name in ("mixed_target_cross_entropy", "hier_tokenizer", "linear", "layer_norm", "gelu", "gelu_dropout", "attention", "dwconv1d"):
    globals()[_name] = torch.compiler.disable(globals()[_name], recursive=True)
del _name
