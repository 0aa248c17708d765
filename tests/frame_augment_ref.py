"""The definition of ``xp_frames_transform`` (plain helper module, no tests of its own), stated twice as tests/frame_transform_ref.py
states ``xp_frames_resize_norm`` -- and importing from it what already exists (the cubic axis table, G, MEAN, STD):

``reference``: numpy, independent of torch.  The two-stage bilinear taps and weights come coordinate by coordinate from the EXACT
rational source coordinates (integer floor division, the fraction as one division of two integers), four taps per axis with the
product weights; the 4 x 4 taps are accumulated rows first; the colour ops are restated in array form.
``reference_torch``: the reference's transform stacks on a float tensor, line by line -- torchvision is not installed, and on a tensor
its transforms ARE these torch calls:
    dataloader.py:189  RandomResizedCrop(input_res, BICUBIC)  -> img[..., i:i + h, j:j + w], F.interpolate(size, mode="bicubic")
    dataloader.py:190  RandomHorizontalFlip                   -> img.flip(-1)
    dataloader.py:191  ColorJitter                            -> adjust_brightness / adjust_saturation / adjust_hue of torchvision's
                                                                 tensor backend (_blend, rgb_to_grayscale, _rgb2hsv, _hsv2rgb), restated
    dataloader.py:195  Resize([vh, vw])                       -> F.interpolate(size=(vh, vw), mode="bilinear", align_corners=False)
    dataloader.py:196  CenterCrop([int(vh*0.9), int(vw*0.9)]) -> img[..., top:top + ch, left:left + cw]
    dataloader.py:197  Resize(input_res)                      -> F.interpolate(size=(rh, rw), mode="bilinear", align_corners=False)
    Normalize                                                 -> (img - mean[:, None, None]) / std[:, None, None]
with the one documented deviation: the hue op clamps its input to [0, 1] first.

Both take a ``dtype``: float64 is the definition; float32 is the same definition at the kernel's precision, from which the GPU test's
colour-stage gate is derived (``float32_error``).  (In the numpy float32 run the cubic weights are the float64 table's, rounded.)

``CASES``: the case table both test files share (sources are generated from a fixed seed, once)."""
from collections import namedtuple

import numpy as np

from tests.frame_transform_ref import G, MEAN, STD, axis_table

# the two-stage fields of XpFrameTransform, in hip_ops.FrameTwoStage's order
Two = namedtuple("Two", "mid_h mid_w crop_y crop_x crop_h crop_w")
# utils.transforms.AugmentParams's fields, in its order
P = namedtuple("P", "i j h w flip order brightness saturation hue")
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)


def color_ops(p):
    """the (name, factor) pairs a record applies, in its order (contrast, index 1, is skipped)"""
    f = {BRIGHTNESS: ("brightness", p.brightness), SATURATION: ("saturation", p.saturation), HUE: ("hue", p.hue)}
    return tuple(f[k] for k in p.order if k in f and f[k][1] is not None)


# --------------------------------------------------------------------------------------------------------------- numpy
def linear_stage(r, n_in, n_out, dtype):
    """(i0, i1, l, 1 - l) of max(0, (r + 0.5) * n_in / n_out - 0.5), from the exact rational ((2 r + 1) n_in - n_out) / (2 n_out)"""
    num, den = max((2 * r + 1) * n_in - n_out, 0), 2 * n_out
    i0 = num // den
    rem = num - i0 * den
    return i0, min(i0 + 1, n_in - 1), dtype(rem) / dtype(den), dtype(den - rem) / dtype(den)


def axis_table2(r0, n, box, mid, crop0, crop, out, box0, dtype=np.float64):
    """taps [n, 4] (source indices) and weights [n, 4] of stage-2 coordinates r0 .. r0 + n - 1: two stage-1 coordinates, two source
    taps each"""
    taps, w = np.zeros((n, 4), np.int64), np.zeros((n, 4), dtype)
    for k in range(n):
        m0, m1, l2, s2 = linear_stage(r0 + k, crop, out, dtype)
        for a, (m, w2) in enumerate(((m0, s2), (m1, l2))):
            j0, j1, l1, s1 = linear_stage(crop0 + m, box, mid, dtype)
            taps[k, 2 * a], taps[k, 2 * a + 1] = box0 + j0, box0 + j1
            w[k, 2 * a], w[k, 2 * a + 1] = w2 * s1, w2 * l1
    return taps, w


def resized(src, g, oh, ow, two=None, dtype=np.float64):
    """the float image [T, oh, ow, 3] (source / 255 resized, windowed, flipped; overshoot kept)"""
    src = np.asarray(src).astype(dtype)
    if two is None:
        ty, wy = axis_table(g.top, oh, g.box_h, g.rh, g.box_y)
        tx, wx = axis_table(g.left, ow, g.box_w, g.rw, g.box_x)
        wy, wx = wy.astype(dtype), wx.astype(dtype)
    else:
        ty, wy = axis_table2(g.top, oh, g.box_h, two.mid_h, two.crop_y, two.crop_h, g.rh, g.box_y, dtype)
        tx, wx = axis_table2(g.left, ow, g.box_w, two.mid_w, two.crop_x, two.crop_w, g.rw, g.box_x, dtype)
    if g.flip:
        tx, wx = tx[::-1], wx[::-1]
    acc = np.zeros((src.shape[0], oh, ow, 3), dtype)
    for j in range(4):
        row = np.zeros_like(acc)
        for i in range(4):
            row += wx[None, None, :, i, None] * src[:, ty[:, j]][:, :, tx[:, i]]
        acc += wy[None, :, j, None, None] * row
    return acc / dtype(255.0)


def brightness(x, f):
    return np.clip(x.dtype.type(f) * x, 0, 1)


def saturation(x, f):
    t = x.dtype.type
    gray = t(0.2989) * x[..., 0] + t(0.587) * x[..., 1] + t(0.114) * x[..., 2]
    return np.clip(t(f) * x + (t(1) - t(f)) * gray[..., None], 0, 1)


def rgb2hsv(x):
    t = x.dtype.type
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(-1), x.min(-1)
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, t(1), maxc)
    div = np.where(eqc, t(1), cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (t(2) + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (t(4) + gc - rc)
    h = np.fmod((hr + hg + hb) / t(6) + t(1), t(1))
    return h, s, maxc


def hsv2rgb(h, s, v):
    t = h.dtype.type
    i = np.floor(h * t(6))
    f = h * t(6) - i
    i = i.astype(np.int32) % 6
    p = np.clip(v * (t(1) - s), 0, 1)
    q = np.clip(v * (t(1) - s * f), 0, 1)
    k = np.clip(v * (t(1) - s * (t(1) - f)), 0, 1)
    tables = ((v, q, p, p, k, v), (k, v, v, q, p, p), (p, p, k, v, v, q))
    return np.stack([np.choose(i, tab) for tab in tables], -1)


def hue(x, f, clamp=True):
    """(clamp=False: torchvision's own arithmetic, for the test that shows the clamp is the identity on in-range input)"""
    if clamp:
        x = np.clip(x, 0, 1)
    h, s, v = rgb2hsv(x)
    h = h + x.dtype.type(f)
    h = h - np.floor(h)                              # Python's % 1
    return hsv2rgb(h, s, v)


COLOR = {"brightness": brightness, "saturation": saturation, "hue": hue}


def reference(src, g, oh, ow, two=None, ops=(), mean=MEAN, std=STD, dtype=np.float64):
    """src: uint8 ndarray [T, H, W, 3]; returns ``dtype`` [T, 3, oh, ow]"""
    x = resized(src, g, oh, ow, two, dtype)
    for name, f in ops:
        x = COLOR[name](x, f)
    out = (x - np.asarray(mean, dtype)) / np.asarray(std, dtype)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


# --------------------------------------------------------------------------------------------------------------- torch
def _blend(img1, img2, ratio):
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 1.0)


def _rgb2hsv_torch(img):
    import torch
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb_torch(img):
    import torch
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def _color_torch(img, name, f):
    import torch
    if name == "brightness":
        return _blend(img, torch.zeros_like(img), f)
    if name == "saturation":
        r, g, b = img.unbind(dim=-3)
        gray = (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)
        return _blend(img, gray, f)
    img = _rgb2hsv_torch(img.clamp(0.0, 1.0))                 # (the clamp: this project's deviation)
    h, s, v = img.unbind(dim=-3)
    h = (h + f) % 1.0
    return _hsv2rgb_torch(torch.stack((h, s, v), dim=-3))


def reference_torch(src, g, oh, ow, two=None, ops=(), mean=MEAN, std=STD, dtype=np.float64):
    import torch
    import torch.nn.functional as F
    td = torch.float64 if dtype is np.float64 else torch.float32
    img = torch.from_numpy(np.ascontiguousarray(src)).permute(0, 3, 1, 2).to(td) / 255.
    img = img[:, :, g.box_y:g.box_y + g.box_h, g.box_x:g.box_x + g.box_w]
    if two is None:
        img = F.interpolate(img, size=(g.rh, g.rw), mode="bicubic", align_corners=False)
    else:
        img = F.interpolate(img, size=(two.mid_h, two.mid_w), mode="bilinear", align_corners=False)
        img = img[:, :, two.crop_y:two.crop_y + two.crop_h, two.crop_x:two.crop_x + two.crop_w]
        img = F.interpolate(img, size=(g.rh, g.rw), mode="bilinear", align_corners=False)
    img = img[:, :, g.top:g.top + oh, g.left:g.left + ow]
    if g.flip:
        img = img.flip(-1)
    for name, f in ops:
        img = _color_torch(img, name, f)
    m, s = torch.tensor(mean, dtype=td), torch.tensor(std, dtype=td)
    return ((img - m[:, None, None]) / s[:, None, None]).numpy()


# ----------------------------------------------------------------------------------------------------------- the case table
# A case is one video.  kind "val": TwoStageTransform(video_res, input_res) must resolve (geometry, two) from the source size;
# kind "train": AugmentTransform(input_res)(video, params=record) -- the geometry is the record's box resized to input_res;
# kind "raw": hip_ops.frames_transform directly (the two-stage filter WITH colour ops, which no factory combines).
Spec = namedtuple("Spec", "kind T H W source video_res input_res oh ow geometry two params ops")


def _val(T, Hs, Ws, video_res, input_res, oh, ow, two, source="random"):
    return Spec("val", T, Hs, Ws, source, video_res, input_res, oh, ow, G(0, 0, Hs, Ws, oh, ow, 0, 0, 0), Two(*two), None, ())


def _train(T, Hs, Ws, size, p, source="random"):
    p = P(*p)
    return Spec("train", T, Hs, Ws, source, None, size, size[0], size[1], G(p.i, p.j, p.h, p.w, size[0], size[1], 0, 0, int(p.flip)),
                None, p, color_ops(p))


_BOX = (7, 9, 21, 30)          # a box inside a 40 x 50 source, as frame_transform_ref's "box" case
ORDERS = {"bsh": (0, 1, 2, 3), "bhs": (0, 3, 1, 2), "sbh": (2, 0, 3, 1), "shb": (1, 2, 3, 0), "hbs": (3, 0, 2, 1), "hsb": (3, 2, 1, 0)}
_SPECS = {
    # Resize(20, 30): CenterCrop(18, 27) at top round(2 / 2) = 1, left round(3 / 2 = 1.5) = 2; Resize(16, 16)
    "two_stage_37x53": _val(2, 37, 53, (20, 30), (16, 16), 16, 16, (20, 30, 1, 2, 18, 27)),
    # the first stage up-scales: its first coordinates are negative and clamp to 0, the last ones reach the last row twice
    "two_stage_up_9x4": _val(1, 9, 4, (20, 30), (16, 16), 16, 16, (20, 30, 1, 2, 18, 27)),
    # input_res an int: the shorter side of the 18 x 27 crop to 16, the longer to int(16 * 27 / 18) = 24, no further crop
    "two_stage_int": _val(1, 37, 53, (20, 30), 16, 16, 24, (20, 30, 1, 2, 18, 27)),
    # the second stage up-scales too, 70 output columns: two column tiles
    "two_stage_wide": _val(1, 11, 23, (10, 40), (9, 70), 9, 70, (10, 40, 0, 2, 9, 36)),
    "crop_flip_no_color": _train(2, 40, 50, (16, 20), _BOX + (True, (0, 1, 2, 3), None, None, None)),
    "brightness": _train(1, 40, 50, (16, 20), _BOX + (False, (0, 1, 2, 3), 1.3, None, None)),
    "brightness_dim": _train(1, 40, 50, (16, 20), _BOX + (False, (2, 1, 0, 3), 0.4, None, None)),
    "saturation": _train(1, 40, 50, (16, 20), _BOX + (True, (0, 1, 2, 3), None, 0.6, None)),
    "saturation_up": _train(1, 40, 50, (16, 20), _BOX + (False, (3, 2, 1, 0), None, 1.7, None)),
    "hue": _train(1, 40, 50, (16, 20), _BOX + (False, (0, 1, 2, 3), None, None, 0.1)),
    "hue_plus_half": _train(1, 40, 50, (16, 20), _BOX + (False, (0, 1, 2, 3), None, None, 0.5)),
    "hue_minus_half": _train(1, 40, 50, (16, 20), _BOX + (True, (0, 1, 2, 3), None, None, -0.5)),
    **{f"order_{n}": _train(1, 40, 50, (16, 20), _BOX + (False, o, 1.2, 0.7, -0.2)) for n, o in ORDERS.items()},
    # identity geometry on grey (r = g = b) pixels, a black and a white one: maxc == minc, s = 0, the hue is that of "no colour"
    "greys": _train(1, 6, 8, (6, 8), (0, 0, 6, 8, False, (3, 2, 1, 0), 1.1, 1.4, 0.3), source="greys"),
    # a 0 / 255 checkerboard up-scaled: the bicubic overshoot leaves [0, 1] on both sides and meets every clamp, the hue's first
    "checker_hue_first": _train(1, 8, 8, (20, 20), (0, 0, 8, 8, False, (3, 0, 2, 1), 1.2, 0.7, 0.25), source="checker"),
    "checker_hue_last": _train(1, 8, 8, (20, 20), (0, 0, 8, 8, True, (0, 2, 1, 3), 0.9, 1.5, -0.4), source="checker"),
    "checker_hue_only": _train(1, 8, 8, (20, 20), (0, 0, 8, 8, False, (0, 1, 2, 3), None, None, 0.5), source="checker"),
    "two_stage_color": Spec("raw", 1, 37, 53, "random", None, None, 16, 16, G(0, 0, 37, 53, 16, 16, 0, 0, 1),
                            Two(20, 30, 1, 2, 18, 27), None, (("saturation", 0.5), ("hue", -0.3), ("brightness", 1.25))),
}

CASES = tuple(_SPECS)
COLOR_CASES = tuple(n for n in CASES if _SPECS[n].ops)
_sources, _refs, _f32 = {}, {}, {}


def spec(name):
    return _SPECS[name]


def source(name):
    """the case's uint8 [T, H, W, 3] ndarray (seeded by the name); built once"""
    if name not in _sources:
        s = _SPECS[name]
        rng = np.random.RandomState(sum(name.encode()))
        if s.source == "random":
            a = rng.randint(0, 256, (s.T, s.H, s.W, 3))
        elif s.source == "greys":
            a = np.repeat(rng.randint(0, 256, (s.T, s.H, s.W, 1)), 3, axis=3)
            a[0, 0, 0], a[0, 0, 1] = 0, 255
        else:                                   # checker: single-pixel squares, the three channels out of phase
            y, x = np.mgrid[:s.H, :s.W]
            a = np.stack([((y + x) % 2) * 255, ((y // 2 + x) % 2) * 255, ((y + x // 2) % 2) * 255], -1)[None].repeat(s.T, 0)
        _sources[name] = a.astype(np.uint8)
    return _sources[name]


def case_reference(name):
    """float64 [T, 3, oh, ow] of the case; computed once and shared (treat as read-only)"""
    if name not in _refs:
        s = _SPECS[name]
        _refs[name] = reference(source(name), s.geometry, s.oh, s.ow, s.two, s.ops)
        _refs[name].setflags(write=False)
    return _refs[name]


def float32_error(name):
    """max |float32 - float64| of the case under BOTH restatements of the definition run in float32 on the CPU (the larger)"""
    if name not in _f32:
        s = _SPECS[name]
        a = reference(source(name), s.geometry, s.oh, s.ow, s.two, s.ops, dtype=np.float32)
        b = reference_torch(source(name), s.geometry, s.oh, s.ow, s.two, s.ops, dtype=np.float32)
        assert a.dtype == np.float32 and b.dtype == np.float32
        want = case_reference(name)
        _f32[name] = max(float(np.abs(a.astype(np.float64) - want).max()), float(np.abs(b.astype(np.float64) - want).max()))
    return _f32[name]


def color_gate():
    """the GPU bound of the paths WITH a colour stage: four times the largest float32_error over the colour cases (the margin covers
    a different but valid fp32 operation order and fused multiply-adds)"""
    return 4.0 * max(float32_error(n) for n in COLOR_CASES)
