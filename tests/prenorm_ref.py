"""References for the pre-norm encoder layer with GELU and LayerScale: the layer and the encoder stack in plain torch at the dtype of
their inputs, with explicit dropout masks, per-image DropPath factors and the LayerScale vectors, their backward by autograd; and
the torch module tree the HIP model shares its state_dict keys with."""
import math

import torch

from drop_path_ref import keep_flags, layernorm_of  # noqa: F401  (re-exported: the tests take them from here)

ORDER = ["in_w", "in_b", "out_w", "out_b", "n2_w", "n2_b", "w1", "b1", "w2", "b2", "next_w", "next_b"]


def _ln(t, w, b, eps):
    return torch.nn.functional.layer_norm(t, (t.shape[-1],), w, b, eps)


def pre_norm_layer(s, n, P, H, masks=None, c1=None, c2=None, lam=None, act="relu", attn_mask=None, rel_bias=None, eps=1e-5,
                   keep=None):
    """One pre-norm layer as "residual site + the LayerNorm after it": s [B, N, D] the residual stream, n = norm1(s);
         a = drop1(out_proj(attention(in_proj(n))));   s1 = s  + c1[b] lam1 * a;   n1 = LN(s1; n2_w, n2_b)
         f = drop2(W2 drop(act(W1 n1 + b1)) + b2);     s2 = s1 + c2[b] lam2 * f;   n2 = LN(s2; next_w, next_b)
    -> (s2, n2).  masks = (ma [B, H, N, N], m1 [B, N, D], mf [B, N, F], m2 [B, N, D]), each {0, 1 / (1 - p)}, or None (all ones);
    c1, c2 [B] = keep / (1 - rate) or None (ones); lam = (lam1, lam2) [D] each or None (ones); act "relu" | "gelu" (erf);
    attn_mask additive [N, N]; rel_bias additive [H, N, N].  keep: a dict that receives the intermediates (a, s1, n1, u, h, f)."""
    B, N, D = s.shape
    hd = D // H
    one = s.new_ones(())
    ma, m1, mf, m2 = masks if masks is not None else (one, one, one, one)
    c1 = s.new_ones(B) if c1 is None else c1
    c2 = s.new_ones(B) if c2 is None else c2
    l1, l2 = lam if lam is not None else (one, one)
    qkv = n @ P["in_w"].t() + P["in_b"]
    q, k, v = qkv.split(D, dim=-1)
    sp = lambda t: t.reshape(B, N, H, hd).transpose(1, 2)      # noqa: E731
    sc = (sp(q) @ sp(k).transpose(-1, -2)) / math.sqrt(hd)
    if attn_mask is not None:
        sc = sc + attn_mask
    if rel_bias is not None:
        sc = sc + rel_bias
    o = ((torch.softmax(sc, -1) * ma) @ sp(v)).transpose(1, 2).reshape(B, N, D)
    a = (o @ P["out_w"].t() + P["out_b"]) * m1
    s1 = s + c1[:, None, None] * l1 * a
    n1 = _ln(s1, P["n2_w"], P["n2_b"], eps)
    u = n1 @ P["w1"].t() + P["b1"]
    h = (torch.relu(u) if act == "relu" else torch.nn.functional.gelu(u)) * mf
    f = (h @ P["w2"].t() + P["b2"]) * m2
    s2 = s1 + c2[:, None, None] * l2 * f
    n2 = _ln(s2, P["next_w"], P["next_b"], eps)
    if keep is not None:
        keep.update(a=a, s1=s1, n1=n1, u=u, h=h, f=f)
    return s2, n2


def encoder(x, layers, final, H, act="relu", lams=None, masks=None, cs=None, eps=1e-5):
    """The pre-norm stack: layers = a list of dicts with in_w, in_b, out_w, out_b, n1_w, n1_b, w1, b1, w2, b2, n2_w, n2_b (a
    layer's own two norms); final = (weight, bias) of the final norm; lams / masks / cs per layer or None.  -> LN_final(s_L)."""
    s = x
    n = _ln(s, layers[0]["n1_w"], layers[0]["n1_b"], eps)
    for l, L in enumerate(layers):
        nxt = (layers[l + 1]["n1_w"], layers[l + 1]["n1_b"]) if l + 1 < len(layers) else final
        P = dict(L, next_w=nxt[0], next_b=nxt[1])
        c1, c2 = cs[l] if cs is not None else (None, None)
        s, n = pre_norm_layer(s, n, P, H, masks[l] if masks is not None else None, c1, c2, lams[l] if lams is not None else None, act,
                              eps=eps)
    return n


def torch_encoder(D, H, Fd, depth, act, dropout=0.0):
    """nn.TransformerEncoder(nn.TransformerEncoderLayer(norm_first=True, activation=act, batch_first=True), norm=LayerNorm): the
    module tree whose state_dict keys a norm_first model's `encoder.transformer.*` are."""
    from torch import nn
    layer = nn.TransformerEncoderLayer(d_model=D, nhead=H, dim_feedforward=Fd, dropout=dropout, batch_first=True, norm_first=True,
                                       activation=act)
    return nn.TransformerEncoder(layer, num_layers=depth, norm=nn.LayerNorm(D), enable_nested_tensor=False)


def layers_of(enc):
    """The parameter dicts `encoder` takes, read from a torch nn.TransformerEncoder (or the HIP model's `encoder.transformer`)."""
    out = []
    for L in enc.layers:
        a = L.self_attn
        out.append(dict(in_w=a.in_proj_weight, in_b=a.in_proj_bias, out_w=a.out_proj.weight, out_b=a.out_proj.bias,
                        n1_w=L.norm1.weight, n1_b=L.norm1.bias, w1=L.linear1.weight, b1=L.linear1.bias, w2=L.linear2.weight,
                        b2=L.linear2.bias, n2_w=L.norm2.weight, n2_b=L.norm2.bias))
    return out, (enc.norm.weight, enc.norm.bias)
