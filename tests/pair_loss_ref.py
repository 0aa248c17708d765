"""The four fixed-temperature pair losses restated with plain torch ops (a helper, not a test).

Dtype-generic: run it in fp64 under autograd and it is the yardstick for the fused kernels (tests/test_pair_loss_gpu.py);
tests/test_pair_loss_cpu.py pins it to the reference's own outputs (tests/golden/pair_losses.pt).  Written from the maths in
include/xpretrain_hip.h (xp_pair_loss).  Three of the losses select (top-k, hardest negative, hinge), so they are only
piecewise smooth: `decision_margin` says how far an input is from the nearest switch, and every gradient comparison asserts
MIN_MARGIN on its inputs first.
"""
import math

import torch

# kind name -> module class name; the order is XpPairLossKind's
KINDS = {
    "nce": "NCEContrastiveLoss",
    "triplet": "TripletContrastiveLoss",
    "hardneg": "HardNegLoss",
    "milnce": "MILNCEContrastiveLoss",
}
KIND_IDS = {k: i for i, k in enumerate(KINDS)}
KIND_NAMES = list(KINDS)                  # the fixtures store a kind as its number
DEFAULTS = dict(temp=1.0, margin=0.0, max_violation=0, order_measure=0, hard_negative_num=1, bag=1)
# An fp32 dot product of unit vectors of length d <= 128 is off by up to d 2^-24 <= 7.7e-6 whatever the summation order, so two
# compared similarities can swap when they are closer than 1.6e-5; a swap moves the gradient by a whole feature row.
MIN_MARGIN = 2e-5


def configs(n):
    """every (kind, params) of the fixtures and the GPU tests at n pairs"""
    out = [("triplet", dict(margin=0.2, max_violation=mv, order_measure=om)) for mv in (0, 1) for om in (0, 1)]
    out += [("nce", dict(temp=t)) for t in (0.05, 1.0)]
    out += [("hardneg", dict(hard_negative_num=k)) for k in sorted({1, min(3, n), min(15, n), n})]
    out += [("milnce", dict(temp=0.05, bag=b)) for b in (1, 3)]
    return out


def grad_scale(kind, params):
    """c of dV = c G T: 1 / temp for the two losses that have a temperature, otherwise 1"""
    return 1.0 / params["temp"] if kind in ("nce", "milnce") else 1.0


def grad_scale_floor(c):
    """Below this max-norm a feature-gradient tensor is fp32 rounding residue (tests/loss_family_ref.py::grad_scale_floor, with
    the fixed scale c in the place of exp(log_scale))."""
    return 4.0 * 2.0 ** -24 * c


def order_sim(vis, txt):
    """S_ij = -|max(0, t_j - v_i)|_2"""
    return -(txt[None, :, :] - vis[:, None, :]).clamp(min=0).pow(2).sum(2).sqrt()


def _triplet_costs(vis, txt, p):
    S = order_sim(vis, txt) if p["order_measure"] else vis @ txt.t()
    dg = torch.diagonal(S)
    off = ~torch.eye(S.shape[0], dtype=torch.bool, device=S.device)
    cs = (p["margin"] + S - dg[:, None]).clamp(min=0) * off
    ci = (p["margin"] + S - dg[None, :]).clamp(min=0) * off
    return S, cs, ci


def _lowered(S):
    """the similarity matrix with its diagonal lowered by 10000, as the top-k sees it"""
    return S - 10000 * torch.eye(S.shape[0], dtype=S.dtype, device=S.device)


def loss(kind, vis, txt, **params):
    p = dict(DEFAULTS, **params)
    n = vis.shape[0]
    if kind == "nce":
        S = vis @ txt.t() / p["temp"]
        dg = torch.diagonal(S)
        return (torch.logsumexp(S, 1) - dg).mean() + (torch.logsumexp(S, 0) - dg).mean()
    if kind == "triplet":
        _, cs, ci = _triplet_costs(vis, txt, p)
        if p["max_violation"]:
            return cs.max(1)[0].sum() + ci.max(0)[0].sum()
        return cs.sum() + ci.sum()
    if kind == "hardneg":
        S = txt @ vis.t()
        dg = torch.diagonal(S)
        out = 0.0
        for M in (S, S.t()):
            top = torch.topk(_lowered(M), p["hard_negative_num"], dim=1)[0]
            out = out + (torch.logsumexp(torch.cat([dg[:, None], top], 1), 1) - dg).mean()
        return out
    if kind == "milnce":
        x = (vis @ txt.t() / p["temp"]).view(n, n, -1)
        eye = torch.eye(n, dtype=torch.bool, device=x.device)
        nom = torch.logsumexp(x[eye], 1)                                         # x[i, i, :]
        rows = x.masked_fill(eye[:, :, None], float("-inf")).reshape(n, -1)      # x[i, j != i, :]
        cols = x.permute(1, 0, 2).reshape(n, -1)                                 # x[j, i, :], every j
        return (torch.logsumexp(torch.cat([rows, cols], 1), 1) - nom).mean()
    raise KeyError(kind)


def loss_and_grads(kind, feats, dtype=torch.float64, **params):
    """loss, [d vis, d txt] in `dtype` on the CPU"""
    fs = [f.detach().cpu().to(dtype).requires_grad_() for f in feats]
    out = loss(kind, fs[0], fs[1], **params)
    return out.detach(), list(torch.autograd.grad(out, fs))


def decision_margin(kind, params, feats):
    """In fp64: how far the input is from the nearest point where a selection of the loss switches -- the smallest of
      * hardneg: the gap between the k-th and the (k+1)-th largest lowered entry of any row, in either direction;
      * triplet with max_violation: the gap between the largest and the second-largest positive cost of any row / column;
      * triplet: |margin + S_ij - S_ii| and |margin + S_ij - S_jj| over all off-diagonal pairs (the hinges).
    +inf for nce and milnce, and wherever a row has no second candidate."""
    p = dict(DEFAULTS, **params)
    vis, txt = (f.detach().cpu().double() for f in feats)
    n = vis.shape[0]
    m = math.inf
    if kind == "hardneg":
        k = p["hard_negative_num"]
        if k < n:
            S = txt @ vis.t()
            for M in (S, S.t()):
                srt = torch.sort(_lowered(M), dim=1, descending=True)[0]
                m = min(m, (srt[:, k - 1] - srt[:, k]).min().item())
    elif kind == "triplet" and n > 1:
        S, cs, ci = _triplet_costs(vis, txt, p)
        dg = torch.diagonal(S)
        off = ~torch.eye(n, dtype=torch.bool)
        m = min((p["margin"] + S - dg[:, None]).abs()[off].min().item(), (p["margin"] + S - dg[None, :]).abs()[off].min().item())
        if p["max_violation"] and n > 2:
            for C in (cs, ci.t()):
                top = torch.topk(C, 2, dim=1)[0]
                two = top[:, 1] > 0                                              # lines with a second positive cost
                if two.any():
                    m = min(m, (top[two, 0] - top[two, 1]).min().item())
    return m


def unit_feats(n, d, seed, bag=1, dtype=torch.float64):
    """seeded unit-norm [vis [n, d], txt [n * bag, d]]: the draw of tests/loss_family_ref.py::unit_feats (same generator, vis then
    txt); a bag above 1 draws its [n * bag, d] text rows after those two"""
    g = torch.Generator().manual_seed(seed)
    vis, txt = (torch.randn(n, d, generator=g, dtype=dtype) for _ in range(2))
    if bag > 1:
        txt = torch.randn(n * bag, d, generator=g, dtype=dtype)
    return [torch.nn.functional.normalize(x, dim=-1) for x in (vis, txt)]


def joint_margin(n, d, seed):
    """the smallest decision margin over every configuration of `configs(n)` on the fp32-rounded draw of `seed`"""
    feats = [f.float() for f in unit_feats(n, d, seed)]
    return min(decision_margin(k, p, feats) for k, p in configs(n) if k in ("triplet", "hardneg"))
