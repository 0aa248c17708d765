"""The reference's frame transforms on the device: the three factories of ``src/datasets/dataloader.py:180-260`` with their names,
signatures and defaults, so the dataset classes keep their line; what changes is WHERE the transform runs ("Decoded
frames").  Each transform takes the raw decoded uint8 frames, whatever their resolution, and is one HIP launch per batch
(``hip_ops.frames_resize_norm`` / ``hip_ops.frames_transform``) instead of ``frames.permute(0, 3, 1, 2).float() / 255.``
(``dataset_video_retrieval.py:102-105``) followed by a torchvision ``Compose`` on a CPU worker.

``init_transform_dict_simple`` (:209-233, the one both dataset classes use): ``Resize(input_res, BICUBIC)``, ``CenterCrop(input_res)``,
``Normalize`` in all three modes -- ``FrameTransform``.
``init_transform_dict_image`` (:235-260): that stack for val / test; train is ``RandomResizedCrop(input_res, scale, BICUBIC)``,
``RandomHorizontalFlip``, ``ColorJitter(brightness, saturation, hue)``, ``Normalize`` -- ``AugmentTransform``.
``init_transform_dict`` (:180-207): the same train; val / test are ``Resize(video_res)``, ``CenterCrop(0.9 video_res)``,
``Resize(input_res)``, ``Normalize``, bilinear -- ``TwoStageTransform``.

The geometry follows torchvision's rules and is resolved on the host by pure functions.  The deliberate reading of the reference: the
float path (no clamp of the bicubic overshoot before the colour ops or Normalize, no re-quantisation), and a pair ``input_res`` -- the
shipped ``[224, 224]`` -- squashes the aspect, as ``Resize((h, w))`` does.  ``antialias=False``, the default, is the reference's pinned
torch 1.8, whose ``interpolate`` has no antialias filter (and torchvision < 0.17 on a tensor).  The reference pins no torchvision, and
every torchvision since 0.17 runs ``Resize`` and ``RandomResizedCrop`` on a float tensor with ``antialias=True``: each transform and
each factory takes ``antialias=True`` for that second definition (``hip_ops.frames_transform(..., antialias=True)``: Keys A = -0.5, a
support that widens with the scale, weights normalised per output coordinate; two launches a batch: a small table kernel, then the
resample).  One deviation: the hue op clamps its input to [0, 1] first.  torchvision documents float images as lying in [0, 1]; a bicubic
overshoot pixel with max(r, g, b) <= 0 is outside its ``_rgb2hsv``'s domain (at exactly 0 it divides by zero: a non-finite pixel).  On in-range input the clamp
is the identity.

The random parameters are drawn on the host from torch's CPU generator (the global one unless ``generator=`` is given), one set per
video shared by all of its frames -- the reference applies its transform to one video tensor --, with torchvision's calls in
torchvision's order (``draw_augment``).  torchvision is not installed where this was written: that the random STREAM matches
torchvision's holds by construction from its published ``get_params`` functions and was not tested against it."""
import functools
import math
import numbers
from typing import NamedTuple, Optional, Tuple

import torch

from .. import hip_ops as H

RATIO = (3.0 / 4.0, 4.0 / 3.0)          # RandomResizedCrop's default, which the reference keeps
# ColorJitter's op indices, as torch.randperm(4) orders them (1, contrast, is never set by the reference: skipped)
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)


def _pair(size, what):
    if isinstance(size, int):
        return None, (size, size)
    size = tuple(int(s) for s in size)
    if len(size) == 1:
        return None, (size[0], size[0])
    if len(size) != 2:
        raise ValueError(f"{what} must be an int, a 1-sequence or an (h, w) pair, got {size}")
    return size, size


def _resize_size(H_src, W_src, exact, size):
    """torchvision's Resize output size: a pair is taken as it is; an int puts the shorter side at ``size`` and the longer at
    ``int(size * long / short)``"""
    if exact is not None:
        return exact
    if W_src <= H_src:
        return int(size * H_src / W_src), size
    return size, int(size * W_src / H_src)


def resize_crop_geometry(H_src: int, W_src: int, input_res):
    """(rh, rw, oh, ow, top, left) of ``Resize(input_res)`` followed by ``CenterCrop(input_res)`` on an H_src x W_src image, by
    torchvision's rules: a pair resizes to exactly (h, w); an int or a 1-sequence puts the shorter side at ``size`` and the longer
    at ``int(size * long / short)``; the crop window sits at ``int(round((rh - oh) / 2.0))`` (Python's round: halves go to even)."""
    exact, (oh, ow) = _pair(input_res, "input_res")
    if H_src <= 0 or W_src <= 0 or oh <= 0 or ow <= 0:
        raise ValueError(f"non-positive size: source {H_src} x {W_src}, input_res {input_res}")
    rh, rw = _resize_size(H_src, W_src, exact, oh)
    if rh < oh or rw < ow:          # (CenterCrop would pad: cannot happen behind its own Resize)
        raise ValueError(f"crop {oh} x {ow} exceeds the resized image {rh} x {rw}")
    return rh, rw, oh, ow, int(round((rh - oh) / 2.0)), int(round((rw - ow) / 2.0))


def two_stage_geometry(H_src: int, W_src: int, video_res, input_res):
    """(mid_h, mid_w, crop_y, crop_x, crop_h, crop_w, rh, rw) of ``Resize(video_res)``, ``CenterCrop([int(vh * 0.9), int(vw * 0.9)])``,
    ``Resize(input_res)`` on an H_src x W_src image (dataloader.py:194-199).  The crop size comes from ``video_res`` as the reference
    writes it, so ``video_res`` is an (h, w) pair; the crop sits at ``int(round((mid - crop) / 2.0))``; a pair ``input_res`` squashes,
    an int puts the shorter side of the CROPPED image at that size (no further crop follows)."""
    exact_v, (vh, vw) = _pair(video_res, "video_res")
    exact_i, (ih, iw) = _pair(input_res, "input_res")
    if exact_v is None:
        raise ValueError(f"video_res must be an (h, w) pair (the reference indexes it), got {video_res}")
    ch, cw = int(vh * 0.9), int(vw * 0.9)
    if H_src <= 0 or W_src <= 0 or ch <= 0 or cw <= 0 or ih <= 0 or iw <= 0:
        raise ValueError(f"non-positive size: source {H_src} x {W_src}, video_res {video_res}, input_res {input_res}")
    rh, rw = _resize_size(ch, cw, exact_i, ih)
    return vh, vw, int(round((vh - ch) / 2.0)), int(round((vw - cw) / 2.0)), ch, cw, rh, rw


def _videos(name, frames, layout):
    """FrameTransform's input rules: (single, list of [T, H, W, 3]-indexed uint8 GPU views)"""
    if layout not in ("THWC", "TCHW"):
        raise ValueError(f"layout must be 'THWC' or 'TCHW', got {layout!r}")
    single = isinstance(frames, torch.Tensor) and frames.dim() == 4
    videos = [frames] if single else list(frames)          # (a [B, ...] tensor iterates over its videos: views)
    if not videos:
        raise ValueError(f"{name}: no frames")
    for v in videos:
        if not isinstance(v, torch.Tensor) or v.dtype != torch.uint8 or not v.is_cuda:
            raise TypeError(f"{name}: frames must be decoded uint8 tensors on the GPU (no CPU path, no float input: "
                            "fp32 pixel_values go to the model as they are)")
        if v.dim() != 4 or v.shape[3 if layout == "THWC" else 1] != 3:
            raise ValueError(f"{name}: a video must be [T, H, W, 3] (layout 'TCHW': [T, 3, H, W]), got {tuple(v.shape)}")
    if layout == "TCHW":
        videos = [v.permute(0, 2, 3, 1) for v in videos]
    if any(v.shape[0] != videos[0].shape[0] for v in videos):
        raise ValueError(f"{name}: the videos of one batch must have the same number of frames")
    return single, videos


class FrameTransform:
    """Decoded uint8 frames on the GPU -> the fp32 ``pixel_values`` of ``VidCLIP.forward``.

    ``transform(frames)``: ``frames`` is one video ``[T, H, W, 3]`` (-> ``[T, 3, h, w]``), a stacked batch ``[B, T, H, W, 3]`` or a list
    of per-video tensors of differing resolution and equal T (-> ``[B, T, 3, h, w]``).  ``layout="TCHW"`` takes ``[T, 3, H, W]``
    (and ``[B, T, 3, H, W]``) instead; any strides are accepted, nothing is copied."""

    def __init__(self, input_res=(224, 224), norm_mean=H.CLIP_MEAN, norm_std=H.CLIP_STD, layout="THWC", antialias=False):
        _pair(input_res, "input_res")
        if layout not in ("THWC", "TCHW"):
            raise ValueError(f"layout must be 'THWC' or 'TCHW', got {layout!r}")
        self.input_res, self.layout, self.antialias = input_res, layout, bool(antialias)
        self.mean, self.std = tuple(float(m) for m in norm_mean), tuple(float(s) for s in norm_std)

    def geometry(self, H_src, W_src):
        rh, rw, oh, ow, top, left = resize_crop_geometry(H_src, W_src, self.input_res)
        return H.FrameGeometry(0, 0, H_src, W_src, rh, rw, top, left, 0), oh, ow

    def __call__(self, frames, layout=None):
        single, videos = _videos("FrameTransform", frames, layout or self.layout)
        geo = [self.geometry(v.shape[1], v.shape[2]) for v in videos]
        oh, ow = geo[0][1:]
        if self.antialias:
            out = H.frames_transform(videos, [g for g, _, _ in geo], oh, ow, self.mean, self.std, antialias=True)
        else:
            out = H.frames_resize_norm(videos, [g for g, _, _ in geo], oh, ow, self.mean, self.std)
        return out if single else out.view(len(videos), videos[0].shape[0], 3, oh, ow)


class TwoStageTransform(FrameTransform):
    """``init_transform_dict``'s val / test: ``Resize(video_res)``, ``CenterCrop(0.9 video_res)``, ``Resize(input_res)``, ``Normalize``,
    bilinear (``F.interpolate(mode="bilinear", align_corners=False)``), without an intermediate image: one launch whose four taps per
    axis carry the product weights of the two stages (``antialias=True``: whose table rows are the product of the two stages'
    antialiased rows).  FrameTransform's calling convention."""

    def __init__(self, video_res=(240, 320), input_res=(224, 224), norm_mean=H.CLIP_MEAN, norm_std=H.CLIP_STD, layout="THWC",
                 antialias=False):
        super().__init__(input_res, norm_mean, norm_std, layout, antialias)
        self.video_res = video_res
        two_stage_geometry(1, 1, video_res, input_res)

    def geometry(self, H_src, W_src):
        """(FrameGeometry, FrameTwoStage, oh, ow): the output is the whole stage-2 image"""
        mh, mw, cy, cx, ch, cw, rh, rw = two_stage_geometry(H_src, W_src, self.video_res, self.input_res)
        return H.FrameGeometry(0, 0, H_src, W_src, rh, rw, 0, 0, 0), H.FrameTwoStage(mh, mw, cy, cx, ch, cw), rh, rw

    def __call__(self, frames, layout=None):
        single, videos = _videos("TwoStageTransform", frames, layout or self.layout)
        geo = [self.geometry(v.shape[1], v.shape[2]) for v in videos]
        oh, ow = geo[0][2:]
        out = H.frames_transform(videos, [g[0] for g in geo], oh, ow, self.mean, self.std, two_stage=[g[1] for g in geo],
                                 antialias=self.antialias)
        return out if single else out.view(len(videos), videos[0].shape[0], 3, oh, ow)


# ------------------------------------------------------------------------------------------------------ the random parameters
class AugmentParams(NamedTuple):
    """one video's drawn parameters: the crop box (torchvision's i, j, h, w: top, left, height, width in the source), the flip, the
    order of ColorJitter's four ops (a permutation of 0 .. 3; 1 = contrast is skipped) and the three factors (None: op not applied)"""
    i: int
    j: int
    h: int
    w: int
    flip: bool
    order: Tuple[int, int, int, int] = (0, 1, 2, 3)
    brightness: Optional[float] = None
    saturation: Optional[float] = None
    hue: Optional[float] = None

    def color_ops(self):
        """the ``(op name, factor)`` pairs to apply, in order"""
        f = {BRIGHTNESS: ("brightness", self.brightness), SATURATION: ("saturation", self.saturation), HUE: ("hue", self.hue)}
        return tuple(f[k] for k in self.order if k in f and f[k][1] is not None)


def jitter_range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
    """torchvision's ``ColorJitter._check_input``: a number v gives [center - v, center + v] (the lower end clipped at 0 for
    brightness / saturation); a (min, max) pair is taken as it is; both must lie inside ``bound``; a range that collapses onto the
    neutral value is None (no op, and no draw)."""
    if isinstance(value, numbers.Number):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        value = [float(value[0]), float(value[1])]
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise ValueError(f"{name} values should be between {bound}, but got {value}.")
    return None if value[0] == value[1] == center else (value[0], value[1])


def _uniform(lo, hi, generator):
    return torch.empty(1).uniform_(lo, hi, generator=generator).item()


def draw_crop(H_src, W_src, scale, ratio=RATIO, generator=None):
    """torchvision's ``RandomResizedCrop.get_params`` on an H_src x W_src image: (i, j, h, w)"""
    area = H_src * W_src
    log_ratio = torch.log(torch.tensor(ratio))
    lo, hi = float(log_ratio[0]), float(log_ratio[1])
    for _ in range(10):
        target_area = area * _uniform(scale[0], scale[1], generator)
        aspect_ratio = math.exp(_uniform(lo, hi, generator))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W_src and 0 < h <= H_src:
            i = torch.randint(0, H_src - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, W_src - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    in_ratio = float(W_src) / float(H_src)          # fallback: the central crop, clamped to the ratio range
    if in_ratio < min(ratio):
        w = W_src
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H_src
        w = int(round(h * max(ratio)))
    else:
        w, h = W_src, H_src
    return (H_src - h) // 2, (W_src - w) // 2, h, w


def draw_augment(H_src, W_src, scale, ratio, brightness, saturation, hue, generator=None) -> AugmentParams:
    """One video's parameters, by the calls and in the order of ``Compose([RandomResizedCrop, RandomHorizontalFlip, ColorJitter])``:
    the crop's tries, ``torch.rand(1) < 0.5``, then ``torch.randperm(4)`` (always) and one ``uniform_`` for each of brightness,
    saturation, hue whose range is not None."""
    i, j, h, w = draw_crop(H_src, W_src, scale, ratio, generator)
    flip = bool(torch.rand(1, generator=generator) < 0.5)
    order = tuple(int(k) for k in torch.randperm(4, generator=generator))
    b = None if brightness is None else _uniform(brightness[0], brightness[1], generator)
    s = None if saturation is None else _uniform(saturation[0], saturation[1], generator)
    f = None if hue is None else _uniform(hue[0], hue[1], generator)
    return AugmentParams(i, j, h, w, flip, order, b, s, f)


class AugmentTransform(FrameTransform):
    """The train transform of ``init_transform_dict`` and ``init_transform_dict_image``: ``RandomResizedCrop(input_res, scale,
    ratio=(3/4, 4/3), BICUBIC)``, ``RandomHorizontalFlip(0.5)``, ``ColorJitter(brightness, saturation, hue)``, ``Normalize`` -- one
    launch: the drawn box is the kernel's source box, the colour ops run on the resized float pixel in the drawn order.
    FrameTransform's calling convention, plus:

    ``draw(sizes_or_videos, generator=None)``: the per-video ``AugmentParams`` for a list of ``(H, W)`` pairs or of videos, in batch
    order, from ``generator`` (else the transform's, else torch's global CPU generator).
    ``transform(frames, params=records)`` applies the given records and draws nothing: how a test, a log or a replay pins an
    augmentation.  Without ``params`` the call draws (``generator=`` as for ``draw``)."""

    def __init__(self, input_res=(224, 224), randcrop_scale=(0.8, 1.0), color_jitter=(0, 0, 0), norm_mean=H.CLIP_MEAN,
                 norm_std=H.CLIP_STD, layout="THWC", generator=None, antialias=False):
        super().__init__(input_res, norm_mean, norm_std, layout, antialias)
        self.size = _pair(input_res, "input_res")[1]
        if not isinstance(randcrop_scale, (tuple, list)) or len(randcrop_scale) != 2 or \
                not 0 < randcrop_scale[0] <= randcrop_scale[1]:
            raise ValueError(f"randcrop_scale must be a (min, max) pair with 0 < min <= max, got {randcrop_scale}")
        if not isinstance(color_jitter, (tuple, list)) or len(color_jitter) != 3:
            raise ValueError(f"color_jitter must be (brightness, saturation, hue), got {color_jitter}")
        self.scale, self.ratio = (float(randcrop_scale[0]), float(randcrop_scale[1])), RATIO
        self.brightness = jitter_range(color_jitter[0], "brightness")
        self.saturation = jitter_range(color_jitter[1], "saturation")
        self.hue = jitter_range(color_jitter[2], "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        self.generator = generator

    def draw(self, sizes_or_videos, generator=None, layout=None):
        generator = generator if generator is not None else self.generator
        ih, iw = (1, 2) if (layout or self.layout) == "THWC" else (2, 3)
        sizes = [(s.shape[ih], s.shape[iw]) if isinstance(s, torch.Tensor) else (int(s[0]), int(s[1])) for s in sizes_or_videos]
        return [draw_augment(h, w, self.scale, self.ratio, self.brightness, self.saturation, self.hue, generator) for h, w in sizes]

    def geometry(self, H_src, W_src, p=None):
        """the drawn box resized to exactly the output size; without a record, the whole image unflipped"""
        oh, ow = self.size
        p = p if p is not None else AugmentParams(0, 0, H_src, W_src, False)
        return H.FrameGeometry(p.i, p.j, p.h, p.w, oh, ow, 0, 0, int(p.flip)), oh, ow

    def __call__(self, frames, layout=None, params=None, generator=None):
        single, videos = _videos("AugmentTransform", frames, layout or self.layout)
        if params is None:
            params = self.draw([(v.shape[1], v.shape[2]) for v in videos], generator)
        else:
            params = [params] if isinstance(params, AugmentParams) else list(params)
            if len(params) != len(videos):
                raise ValueError(f"AugmentTransform: {len(videos)} videos with {len(params)} parameter records")
        oh, ow = self.size
        geo = [self.geometry(v.shape[1], v.shape[2], p)[0] for v, p in zip(videos, params)]
        color = [p.color_ops() for p in params]
        out = H.frames_transform(videos, geo, oh, ow, self.mean, self.std, color=color if any(color) else None,
                                 antialias=self.antialias)
        return out if single else out.view(len(videos), videos[0].shape[0], 3, oh, ow)


def _with_antialias(factory):
    """``factory`` with a trailing ``antialias=False`` (the seventh positional argument, or the keyword) that goes to all three modes.
    The introspected signature stays the reference's six parameters (``inspect.signature`` follows ``__wrapped__``): code written
    against the reference's factory sees the reference's factory; the keyword is this package's addition."""
    @functools.wraps(factory)
    def with_antialias(*args, antialias=False, **kwargs):
        if len(args) == 7:
            *args, antialias = args
        modes = factory(*args, **kwargs)
        for transform in modes.values():
            transform.antialias = bool(antialias)
        return modes
    return with_antialias


@_with_antialias
def init_transform_dict(video_res=(240, 320),
                        input_res=(224, 224),
                        randcrop_scale=(0.8, 1.0),
                        color_jitter=(0, 0, 0),
                        norm_mean=(0.48145466, 0.4578275, 0.40821073),
                        norm_std=(0.26862954, 0.26130258, 0.27577711)):
    """dataloader.py:180-207: random crop, flip and colour jitter for train; the two-stage bilinear geometry for val and test"""
    return {"train": AugmentTransform(input_res, randcrop_scale, color_jitter, norm_mean, norm_std),
            "val": TwoStageTransform(video_res, input_res, norm_mean, norm_std),
            "test": TwoStageTransform(video_res, input_res, norm_mean, norm_std)}


@_with_antialias
def init_transform_dict_simple(video_res=(240, 320),
                               input_res=(224, 224),
                               randcrop_scale=(0.8, 1.0),
                               color_jitter=(0, 0, 0),
                               norm_mean=(0.48145466, 0.4578275, 0.40821073),
                               norm_std=(0.26862954, 0.26130258, 0.27577711)):
    """dataloader.py:209-233: the three modes are the same transform (video_res, randcrop_scale and color_jitter are unused there too)"""
    return {mode: FrameTransform(input_res, norm_mean, norm_std) for mode in ("train", "val", "test")}


@_with_antialias
def init_transform_dict_image(video_res=(240, 320),
                              input_res=(224, 224),
                              randcrop_scale=(0.8, 1.0),
                              color_jitter=(0, 0, 0),
                              norm_mean=(0.48145466, 0.4578275, 0.40821073),
                              norm_std=(0.26862954, 0.26130258, 0.27577711)):
    """dataloader.py:235-260: init_transform_dict's train; init_transform_dict_simple's val and test (video_res is unused there too)"""
    return {"train": AugmentTransform(input_res, randcrop_scale, color_jitter, norm_mean, norm_std),
            "val": FrameTransform(input_res, norm_mean, norm_std), "test": FrameTransform(input_res, norm_mean, norm_std)}
