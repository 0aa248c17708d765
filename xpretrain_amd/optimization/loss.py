"""Contrastive loss surface (reference: src/optimization/loss.py).

``NCELearnableTempLoss`` (loss.py:126-141) is the hot-path loss: fused HIP kernels computing
exp(temp) * vis @ text^T, both cross-entropies and all gradients in one call
(csrc/loss_family.hip).  It and the other learnable-temperature losses the reference drivers name (run_pretrain.py:355-363,
run_video_retrieval.py:333) run through one library path, one ``XP_LOSS_*`` kind each (xp_contrastive_loss).
The four two-argument, fixed-temperature losses (loss.py:22-124, reached through the drivers' ``else: loss_func(vis_feat, text_feat)``
branch) run through xp_pair_loss, one ``XP_PAIR_*`` kind each.
``build_loss_func(cfg)`` keeps the reference's factory signature (loss.py:326-328).
"""
from __future__ import annotations

from torch import nn

from .. import _lib as L
from .. import functional as XF


class _FamilyLoss(nn.Module):
    """a loss of the family by its kind; `temp` is the LOG-scale parameter"""
    kind = None

    def __init__(self, cfg=None):
        super().__init__()

    def forward(self, vis_feat, text_feat, img_feat, cap_feat, temp):
        return XF.ContrastiveLossFn.apply(self.kind, vis_feat, text_feat, img_feat, cap_feat, temp)


class NCELearnableTempLoss(_FamilyLoss):
    """loss = CE(exp(temp) * V T^T, diag) + CE(exp(temp) * T V^T, diag) (loss.py:126-141)."""
    kind = L.XP_LOSS_NCE

    def forward(self, vis_feat, text_feat, temp):
        return XF.ContrastiveLossFn.apply(self.kind, vis_feat, text_feat, None, None, temp)


class NCELearnableTempLoss_vsc_fc(_FamilyLoss):
    """Pre-training default (loss.py:288-324, pretrain_vip_base_16.json:75): video-(subtitle, caption) and
    frame-caption contrast, six cross-entropy terms; same call signature as the reference."""
    kind = L.XP_LOSS_VSC_FC

    def forward(self, vis_feat, text_feat, img_feat, cap_feat, temp):
        assert text_feat.shape[0] == cap_feat.shape[0]                       # loss.py:297
        return super().forward(vis_feat, text_feat, img_feat, cap_feat, temp)


class VidImgNCELearnableTempLoss(_FamilyLoss):
    """loss.py:143-160: NCELearnableTempLoss over the concatenations [vis; img] and [text; cap] (img/cap may have another
    row count than vis/text)."""
    kind = L.XP_LOSS_VIDIMG


class VidImgDivideNCELearnableTempLoss(_FamilyLoss):
    """loss.py:162-183: NCELearnableTempLoss(vis, text) + NCELearnableTempLoss(img, cap), each with its own mean."""
    kind = L.XP_LOSS_VIDIMG_DIVIDE


class NCELearnableTempDSLLoss(NCELearnableTempLoss):
    """loss.py:185-202, the retrieval finetuning loss with the dual-softmax prior: each direction's logits are multiplied by
    their softmax over the OTHER axis before the cross-entropy; the prior is not detached (its Jacobian is in the gradient).
    Two operands, as NCELearnableTempLoss."""
    kind = L.XP_LOSS_DSL


class NCELearnableTempLoss_vs_vc(_FamilyLoss):
    """loss.py:204-225: video-subtitle + video-caption, four cross-entropy terms.  `img_feat` is accepted and not read."""
    kind = L.XP_LOSS_VS_VC


class NCELearnableTempLoss_vs_vc_fc(_FamilyLoss):
    """loss.py:227-254: vs_vc + frame-caption, six cross-entropy terms."""
    kind = L.XP_LOSS_VS_VC_FC


class NCELearnableTempLoss_vsc(_FamilyLoss):
    """loss.py:256-286: video-(subtitle, caption) with the off-diagonal negatives of both merged behind either positive.
    `img_feat` is accepted and not read."""
    kind = L.XP_LOSS_VSC

    def forward(self, vis_feat, text_feat, img_feat, cap_feat, temp):
        assert text_feat.shape[0] == cap_feat.shape[0]                       # loss.py:265
        return super().forward(vis_feat, text_feat, img_feat, cap_feat, temp)


def _cfg(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


class _PairLoss(nn.Module):
    """a fixed-temperature loss by its kind; ``self.params``: what its constructor read from `cfg`"""
    kind = None

    def forward(self, vis_feat, text_feat):
        return XF.PairLossFn.apply(self.kind, vis_feat, text_feat, self.params)


class TripletContrastiveLoss(_PairLoss):
    """loss.py:22-64: hinge costs of every negative against the positive of its row and of its column, summed, or with
    `cfg.max_violation` the hardest negative of each row and column only; `cfg.measure` 'order' takes order_sim (:13-19) for the
    cosine.  A pair at order distance exactly 0 contributes no gradient (torch gives NaN there)."""
    kind = L.XP_PAIR_TRIPLET

    def __init__(self, cfg):
        super().__init__()
        self.params = dict(margin=float(_cfg(cfg, "margin")), order_measure=_cfg(cfg, "measure") == "order",
                           max_violation=bool(_cfg(cfg, "max_violation")))

    def forward(self, im, s):
        return super().forward(im, s)


class NCEContrastiveLoss(_PairLoss):
    """loss.py:67-83: both cross-entropies of vis text^T / cfg.temp."""
    kind = L.XP_PAIR_NCE

    def __init__(self, cfg):
        super().__init__()
        self.params = dict(temp=float(_cfg(cfg, "temp")))


class HardNegLoss(_PairLoss):
    """loss.py:86-105: cross-entropy of the positive against the `cfg.hard_negative_num` hardest negatives of its row, both
    directions; no temperature."""
    kind = L.XP_PAIR_HARDNEG

    def __init__(self, cfg):
        super().__init__()
        self.params = dict(hard_negative_num=int(_cfg(cfg, "hard_negative_num")))


class MILNCEContrastiveLoss(_PairLoss):
    """loss.py:109-124: MIL-NCE over bags of text rows; `text_embd` has n * k rows for n videos (row j * k + b is text b of
    video j)."""
    kind = L.XP_PAIR_MILNCE

    def __init__(self, cfg):
        super().__init__()
        self.params = dict(temp=float(_cfg(cfg, "temp")))

    def forward(self, video_embd, text_embd):
        n = video_embd.shape[0]
        if text_embd.shape[0] % n:
            raise ValueError(f"MILNCEContrastiveLoss: {text_embd.shape[0]} text rows are no multiple of {n} videos")
        return XF.PairLossFn.apply(self.kind, video_embd, text_embd, dict(self.params, bag=text_embd.shape[0] // n))


_LOSSES = {c.__name__: c for c in (
    TripletContrastiveLoss, NCEContrastiveLoss, HardNegLoss, MILNCEContrastiveLoss,
    NCELearnableTempLoss, VidImgNCELearnableTempLoss, VidImgDivideNCELearnableTempLoss, NCELearnableTempDSLLoss,
    NCELearnableTempLoss_vs_vc, NCELearnableTempLoss_vs_vc_fc, NCELearnableTempLoss_vsc, NCELearnableTempLoss_vsc_fc)}


def build_loss_func(cfg):
    name = cfg["loss_name"] if isinstance(cfg, dict) else cfg.loss_name
    if name not in _LOSSES:
        raise NotImplementedError(f"loss {name!r} is not on the CLIP-ViP path; available on the HIP path: {sorted(_LOSSES)}")
    return _LOSSES[name](cfg)
