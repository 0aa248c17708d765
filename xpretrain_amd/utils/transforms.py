"""The reference's frame transforms on the device (``src/datasets/dataloader.py:209-233``, ``init_transform_dict_simple``: the one both
dataset classes use): ``Resize(input_res, BICUBIC)``, ``CenterCrop(input_res)``, ``Normalize(mean, std)`` applied to
``frames.permute(0, 3, 1, 2).float() / 255.`` (``dataset_video_retrieval.py:102-105``) -- here one HIP launch per batch on the raw decoded
uint8 frames, whatever their resolution (``hip_ops.frames_resize_norm``).  Same function name, signature and defaults, so the
dataset classes keep their line; what changes is WHERE the transform runs ("Decoded frames").

The geometry follows torchvision's rules and is resolved on the host by a pure function (``resize_crop_geometry``).  The deliberate
reading of the reference: the float path (no clamp of the bicubic overshoot, no re-quantisation), no antialias filter (the reference's
pinned torch has none), and a pair ``input_res`` -- the shipped ``[224, 224]`` -- squashes the aspect, as ``Resize((h, w))`` does.
The other ``init_transform_dict`` (two-stage bilinear val/test, RandomResizedCrop, ColorJitter) is used by neither dataset class and
is not provided."""
import torch

from .. import hip_ops as H


def _pair(size, what):
    if isinstance(size, int):
        return None, (size, size)
    size = tuple(int(s) for s in size)
    if len(size) == 1:
        return None, (size[0], size[0])
    if len(size) != 2:
        raise ValueError(f"{what} must be an int, a 1-sequence or an (h, w) pair, got {size}")
    return size, size


def resize_crop_geometry(H_src: int, W_src: int, input_res):
    """(rh, rw, oh, ow, top, left) of ``Resize(input_res)`` followed by ``CenterCrop(input_res)`` on an H_src x W_src image, by
    torchvision's rules: a pair resizes to exactly (h, w); an int or a 1-sequence puts the shorter side at ``size`` and the longer
    at ``int(size * long / short)``; the crop window sits at ``int(round((rh - oh) / 2.0))`` (Python's round: halves go to even)."""
    exact, (oh, ow) = _pair(input_res, "input_res")
    if H_src <= 0 or W_src <= 0 or oh <= 0 or ow <= 0:
        raise ValueError(f"non-positive size: source {H_src} x {W_src}, input_res {input_res}")
    if exact is not None:
        rh, rw = exact
    elif W_src <= H_src:
        rh, rw = int(oh * H_src / W_src), oh
    else:
        rh, rw = oh, int(oh * W_src / H_src)
    if rh < oh or rw < ow:          # (CenterCrop would pad: cannot happen behind its own Resize)
        raise ValueError(f"crop {oh} x {ow} exceeds the resized image {rh} x {rw}")
    return rh, rw, oh, ow, int(round((rh - oh) / 2.0)), int(round((rw - ow) / 2.0))


class FrameTransform:
    """Decoded uint8 frames on the GPU -> the fp32 ``pixel_values`` of ``VidCLIP.forward``.

    ``transform(frames)``: ``frames`` is one video ``[T, H, W, 3]`` (-> ``[T, 3, h, w]``), a stacked batch ``[B, T, H, W, 3]`` or a list
    of per-video tensors of differing resolution and equal T (-> ``[B, T, 3, h, w]``).  ``layout="TCHW"`` takes ``[T, 3, H, W]``
    (and ``[B, T, 3, H, W]``) instead; any strides are accepted, nothing is copied."""

    def __init__(self, input_res=(224, 224), norm_mean=H.CLIP_MEAN, norm_std=H.CLIP_STD, layout="THWC"):
        _pair(input_res, "input_res")
        if layout not in ("THWC", "TCHW"):
            raise ValueError(f"layout must be 'THWC' or 'TCHW', got {layout!r}")
        self.input_res, self.layout = input_res, layout
        self.mean, self.std = tuple(float(m) for m in norm_mean), tuple(float(s) for s in norm_std)

    def geometry(self, H_src, W_src):
        rh, rw, oh, ow, top, left = resize_crop_geometry(H_src, W_src, self.input_res)
        return H.FrameGeometry(0, 0, H_src, W_src, rh, rw, top, left, 0), oh, ow

    def __call__(self, frames, layout=None):
        layout = layout or self.layout
        if layout not in ("THWC", "TCHW"):
            raise ValueError(f"layout must be 'THWC' or 'TCHW', got {layout!r}")
        single = isinstance(frames, torch.Tensor) and frames.dim() == 4
        videos = [frames] if single else list(frames)          # (a [B, ...] tensor iterates over its videos: views)
        if not videos:
            raise ValueError("FrameTransform: no frames")
        for v in videos:
            if not isinstance(v, torch.Tensor) or v.dtype != torch.uint8 or not v.is_cuda:
                raise TypeError("FrameTransform: frames must be decoded uint8 tensors on the GPU (no CPU path, no float input: "
                                "fp32 pixel_values go to the model as they are)")
            if v.dim() != 4 or v.shape[3 if layout == "THWC" else 1] != 3:
                raise ValueError(f"FrameTransform: a video must be [T, H, W, 3] (layout 'TCHW': [T, 3, H, W]), got {tuple(v.shape)}")
        if layout == "TCHW":
            videos = [v.permute(0, 2, 3, 1) for v in videos]
        if any(v.shape[0] != videos[0].shape[0] for v in videos):
            raise ValueError("FrameTransform: the videos of one batch must have the same number of frames")
        geo = [self.geometry(v.shape[1], v.shape[2]) for v in videos]
        oh, ow = geo[0][1:]
        out = H.frames_resize_norm(videos, [g for g, _, _ in geo], oh, ow, self.mean, self.std)
        return out if single else out.view(len(videos), videos[0].shape[0], 3, oh, ow)


def init_transform_dict_simple(video_res=(240, 320),
                               input_res=(224, 224),
                               randcrop_scale=(0.8, 1.0),
                               color_jitter=(0, 0, 0),
                               norm_mean=(0.48145466, 0.4578275, 0.40821073),
                               norm_std=(0.26862954, 0.26130258, 0.27577711)):
    """dataloader.py:209-233: the three modes are the same transform (video_res, randcrop_scale and color_jitter are unused there too)"""
    return {mode: FrameTransform(input_res, norm_mean, norm_std) for mode in ("train", "val", "test")}
