"""The eight learnable-temperature contrastive losses restated with plain torch ops (a helper, not a test).

Dtype-generic: run it in fp64 under autograd and it is the yardstick for the fused kernels (tests/test_loss_family_gpu.py);
tests/test_loss_family_cpu.py pins it to the reference's own outputs (tests/golden/loss_family.pt).  Written from the maths in
include/xpretrain_hip.h (xp_contrastive_loss), with s = exp(log_scale), S1 = s V T^T, S2 = s V C^T, S3 = s I C^T.
"""
import math

import torch

# kind name -> (module class name, reads img, reads cap); the order is XpLossKind's
KINDS = {
    "nce": ("NCELearnableTempLoss", False, False),
    "vsc_fc": ("NCELearnableTempLoss_vsc_fc", True, True),
    "dsl": ("NCELearnableTempDSLLoss", False, False),
    "vs_vc": ("NCELearnableTempLoss_vs_vc", False, True),
    "vs_vc_fc": ("NCELearnableTempLoss_vs_vc_fc", True, True),
    "vsc": ("NCELearnableTempLoss_vsc", False, True),
    "vidimg": ("VidImgNCELearnableTempLoss", True, True),
    "vidimg_divide": ("VidImgDivideNCELearnableTempLoss", True, True),
}
KIND_IDS = {k: i for i, k in enumerate(KINDS)}
NEW_KINDS = [k for k in KINDS if k not in ("nce", "vsc_fc")]


def grad_scale_floor(log_scale):
    """Below this max-norm a feature-gradient tensor is fp32 rounding residue and has no relative accuracy, in the reference's
    own fp32 run as anywhere: d feature = s G F with |F| <= 1 and G a difference of up to four softmax probabilities and the
    identity, each carried to no better than 2^-24 next to 1, so its absolute resolution is at least 4 s 2^-24 (the rounding
    of the logits themselves makes it coarser; this is the smallest defensible floor).  Errors are measured relative to
    max(max|ref|, this); it only matters where every softmax saturates (n + m = 2 at s = 200: reference gradients of 1e-13)."""
    return 4.0 * 2.0 ** -24 * math.exp(float(log_scale))


def _rows(S):
    """mean over rows of (logsumexp of the row - its diagonal entry)"""
    return (torch.logsumexp(S, dim=1) - torch.diagonal(S)).mean()


def _cols(S):
    return _rows(S.t())


def _merged_rows(Sa, Sb):
    """mean_i [ lse(Sa[i, :] U Sb[i, j != i]) - Sa[i, i] ]: the other matrix's off-diagonal entries join the negatives"""
    n = Sa.shape[0]
    off = ~torch.eye(n, dtype=torch.bool, device=Sa.device)
    joint = torch.cat([Sa, Sb.masked_fill(~off, float("-inf"))], dim=1)
    return (torch.logsumexp(joint, dim=1) - torch.diagonal(Sa)).mean()


def loss(kind, vis, txt, img=None, cap=None, log_scale=None):
    s = log_scale.exp()
    S1 = vis @ txt.t() * s
    if kind == "nce":
        return _rows(S1) + _cols(S1)
    if kind == "dsl":
        B1 = S1 * torch.softmax(S1, dim=0)
        B2 = S1 * torch.softmax(S1, dim=1)
        return _rows(B1) + _cols(B2)
    if kind == "vidimg":
        S = torch.cat([vis, img]) @ torch.cat([txt, cap]).t() * s
        return _rows(S) + _cols(S)
    S3 = None if img is None else img @ cap.t() * s
    if kind == "vidimg_divide":
        return _rows(S1) + _cols(S1) + _rows(S3) + _cols(S3)
    S2 = vis @ cap.t() * s
    if kind in ("vs_vc", "vs_vc_fc"):
        out = _rows(S1) + _cols(S1) + _rows(S2) + _cols(S2)
    elif kind in ("vsc", "vsc_fc"):
        out = _cols(S1) + _cols(S2) + _merged_rows(S1, S2) + _merged_rows(S2, S1)
    else:
        raise KeyError(kind)
    if kind.endswith("_fc"):
        out = out + _rows(S3) + _cols(S3)
    return out


def operands(kind, feats):
    """(vis, txt, img | None, cap | None) of [vis, txt, img, cap] for what the kind reads"""
    _, use_img, use_cap = KINDS[kind]
    return feats[0], feats[1], feats[2] if use_img else None, feats[3] if use_cap else None


def loss_and_grads(kind, feats, log_scale, dtype=torch.float64):
    """loss and d loss / d(vis, txt, img, cap, log_scale) in `dtype` on the CPU; None for an operand the kind does not read"""
    fs = [f.detach().cpu().to(dtype).requires_grad_() for f in feats]
    ls = torch.as_tensor(log_scale).detach().cpu().to(dtype).reshape(()).requires_grad_()
    v, t, i, c = operands(kind, fs)
    out = loss(kind, v, t, i, c, ls)
    used = [x for x in (v, t, i, c) if x is not None]
    g = list(torch.autograd.grad(out, used + [ls]))
    grads = [g.pop(0) if x is not None else None for x in (v, t, i, c)]
    return out.detach(), grads, g[0]


def unit_feats(n, m, d, seed, dtype=torch.float64):
    """seeded unit-norm [vis, txt, img, cap]: vis/txt [n, d], img/cap [m, d]"""
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.functional.normalize(torch.randn(r, d, generator=g, dtype=dtype), dim=-1) for r in (n, n, m, m)]
