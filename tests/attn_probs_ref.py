"""fp64 restatements of the attention WEIGHTS (plain helper module, no tests of its own): the softmax matrices of the reference's
CLIPAttention.forward (causal + padding, CLIP_ViP.py:266-330) and CLIPAttention.forward2 (video proxy, :332-381) on head-split
``[B, h, S, 64]`` q (already scaled) and k -- the matrices whose product with V the oracle's ``masked_attention_core`` /
``proxy_attention_core`` return -- and a layer-level wrapper that takes them from a state dict and a hidden state."""
import torch

from oracle import clipvip_oracle as O


def causal_probs(q, k, pad_mask=None):
    """[B,h,S,S]: softmax(q k^T + causal mask + padding mask), by the mask arithmetic of ``O.masked_attention_core``: -inf above the
    diagonal (:788-797), finfo.min ADDED at padded keys (_expand_mask, :50-61; it absorbs the score, so a row that sees only padded
    keys is uniform over its visible keys)"""
    S = q.shape[2]
    add = torch.full((S, S), float("-inf"), dtype=q.dtype, device=q.device).triu(1)
    if pad_mask is not None:
        inv = 1.0 - pad_mask.to(q.dtype)[:, None, None, :]
        add = add + inv.masked_fill(inv.bool(), torch.finfo(q.dtype).min)
    return torch.softmax(q @ k.transpose(-1, -2) + add, dim=-1)


def proxy_probs(q, k, size):
    """``(proxy [B,h,M,S], frame [B,h,N,L,M+L])``: forward2's second (:365-370) and first (:350-358) attn_weights, with the slicing
    of ``O.proxy_attention_core``: frame-n queries over [M proxy keys | the L keys of frame n], proxy queries over every key"""
    M, N, L = size
    B, h, S, dh = q.shape
    qf = q[:, :, M:].reshape(B, h, N, L, dh)
    kf = k[:, :, M:].reshape(B, h, N, L, dh)
    kk = torch.cat([k[:, :, :M].unsqueeze(2).expand(B, h, N, M, dh), kf], dim=3)
    frame = torch.softmax(qf @ kk.transpose(-1, -2), dim=-1)
    proxy = torch.softmax(q[:, :, :M] @ k.transpose(-1, -2), dim=-1)
    return proxy, frame


def causal_pv(p, v):
    """[B,h,S,dh]: the weights times V, what ``O.masked_attention_core`` returns"""
    return p @ v


def proxy_pv(proxy, frame, v, size):
    """[B,h,S,dh] in [proxies, frames] order: what ``O.proxy_attention_core`` returns"""
    M, N, L = size
    B, h, S, dh = v.shape
    vf = v[:, :, M:].reshape(B, h, N, L, dh)
    vv = torch.cat([v[:, :, :M].unsqueeze(2).expand(B, h, N, M, dh), vf], dim=3)
    return torch.cat([proxy @ v, (frame @ vv).reshape(B, h, N * L, dh)], dim=2)


def layer_qk(hidden, sd, pfx, heads, dtype=torch.float64):
    """LayerNorm 1 -> q * dh^-0.5, k (head-split [B,h,S,dh]) of encoder layer ``pfx`` ("text_model.encoder.layers.0.") on the layer
    input ``hidden`` [B,S,D], from the state dict ``sd`` (keys without the "clipmodel." prefix), as ``O.encoder_layer`` /
    ``O.attention_block`` compute them"""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(pfx)}
    x = hidden.to(dtype)
    h1 = O.layer_norm(x, sd[pfx + "layer_norm1.weight"], sd[pfx + "layer_norm1.bias"])
    dh = x.shape[-1] // heads
    q = O._heads(O.linear(h1, sd, pfx + "self_attn.q_proj") * dh ** -0.5, heads)
    k = O._heads(O.linear(h1, sd, pfx + "self_attn.k_proj"), heads)
    return q, k


def layer_probs(hidden, sd, pfx, heads, size=None, pad_mask=None):
    """the attention weights of encoder layer ``pfx`` on its input ``hidden``, in fp64: ``causal_probs`` (text) or
    ``proxy_probs`` (video, ``size=(M,N,L)``)"""
    q, k = layer_qk(hidden, sd, pfx, heads)
    return proxy_probs(q, k, size) if size is not None else causal_probs(q, k, pad_mask)
