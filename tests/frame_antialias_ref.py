"""The definition of ``xp_frames_transform_aa`` -- the frame transforms with ``antialias=True`` -- (plain helper module, no tests of its
own), stated twice as tests/frame_transform_ref.py and tests/frame_augment_ref.py state the two existing entry points, and importing
from them what already exists (G, Two, P, MEAN, STD, the colour ops, the case geometries):

``reference``: scalar numpy, independent of torch.  Per axis, ``box`` source pixels resized to ``out``:
    scale = box / out;  support = (k / 2) max(scale, 1), k = 4 (bicubic) or 2 (bilinear);  inv = 1 / max(scale, 1)
    for resized coordinate r:  c = scale (r + 0.5);  x0 = max(int(c - support + 0.5), 0);  n = min(int(c + support + 0.5), box) - x0
    w_j = f((j + x0 - c + 0.5) inv) / sum_j f(...),  j = 0 .. n - 1;  f: Keys' cubic with A = -0.5, or the triangle
and the resized pixel is sum_j w_j src[box0 + x0 + j]: the horizontal pass first, then the vertical, taps in ascending order.  The
window, the flip, the colour ops and Normalize follow as xp_frames_transform defines them.  Two-stage: stage 1 to ``mid``, the crop,
stage 2, each bilinear by the rule above, with a real intermediate image.
``reference_torch``: the reference's transform stacks on a float tensor (torchvision >= 0.17 runs its tensor ``Resize`` with
``antialias=True``), line by line: tests/frame_augment_ref.py's calls with ``F.interpolate(..., align_corners=False, antialias=True)``.

Both take a ``dtype``: float64 is the definition; float32 is the same stack at the kernel's precision, from which the GPU test's gates
are derived (``float32_error``: torch's own float32 stack; ``color_float32_error``: both restatements, the larger, as
frame_augment_ref.float32_error).  (In the numpy float32 run the weights are the float64 table's, rounded.)

``CASES``: the case table both test files share (sources are generated from a fixed seed, once)."""
from collections import namedtuple

import numpy as np

from tests import frame_transform_ref as R
from tests.frame_augment_ref import COLOR, P, Two, _color_torch, color_ops
from tests.frame_transform_ref import G, MEAN, STD

KEYS_A = -0.5


def _keys(x):
    """Keys' cubic convolution kernel, A = -0.5"""
    x = abs(x)
    if x < 1.0:
        return ((KEYS_A + 2.0) * x - (KEYS_A + 3.0)) * x * x + 1.0
    if x < 2.0:
        return ((KEYS_A * x - 5.0 * KEYS_A) * x + 8.0 * KEYS_A) * x - 4.0 * KEYS_A
    return 0.0


def _triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"bicubic": (_keys, 4), "bilinear": (_triangle, 2)}


def axis_rows(box, out, mode):
    """[(x0, weights fp64 [n])] for every resized coordinate 0 .. out - 1 of ``box`` source pixels resized to ``out``"""
    f, k = FILTERS[mode]
    scale = box / out
    support = (k / 2) * max(scale, 1.0)
    inv = 1.0 / max(scale, 1.0)
    rows = []
    for r in range(out):
        c = scale * (r + 0.5)
        x0 = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), box) - x0
        w = [f((j + x0 - c + 0.5) * inv) for j in range(n)]
        total = 0.0
        for v in w:
            total += v
        rows.append((x0, np.array([v / total for v in w], np.float64)))
    return rows


def resize(img, rh, rw, mode, dtype=np.float64):
    """img [T, H, W, 3] (``dtype``) -> [T, rh, rw, 3]: the horizontal pass, then the vertical, taps accumulated in ascending order"""
    T, H, W, _ = img.shape
    hor = np.zeros((T, H, rw, 3), dtype)
    for x, (x0, w) in enumerate(axis_rows(W, rw, mode)):
        for j, wj in enumerate(w.astype(dtype)):
            hor[:, :, x] += wj * img[:, :, x0 + j]
    out = np.zeros((T, rh, rw, 3), dtype)
    for y, (y0, w) in enumerate(axis_rows(H, rh, mode)):
        for j, wj in enumerate(w.astype(dtype)):
            out[:, y] += wj * hor[:, y0 + j]
    return out


def resized(src, g, oh, ow, two=None, dtype=np.float64):
    """the float image [T, oh, ow, 3] (source / 255 resized, windowed, flipped; overshoot kept)"""
    img = np.asarray(src).astype(dtype)[:, g.box_y:g.box_y + g.box_h, g.box_x:g.box_x + g.box_w]
    if two is None:
        img = resize(img, g.rh, g.rw, "bicubic", dtype)
    else:
        img = resize(img, two.mid_h, two.mid_w, "bilinear", dtype)
        img = img[:, two.crop_y:two.crop_y + two.crop_h, two.crop_x:two.crop_x + two.crop_w]
        img = resize(img, g.rh, g.rw, "bilinear", dtype)
    img = img[:, g.top:g.top + oh, g.left:g.left + ow]
    if g.flip:
        img = img[:, :, ::-1]
    return img / dtype(255.0)


def reference(src, g, oh, ow, two=None, ops=(), mean=MEAN, std=STD, dtype=np.float64):
    """src: uint8 ndarray [T, H, W, 3]; returns ``dtype`` [T, 3, oh, ow]"""
    x = resized(src, g, oh, ow, two, dtype)
    for name, f in ops:
        x = COLOR[name](x, f)
    out = (x - np.asarray(mean, dtype)) / np.asarray(std, dtype)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def reference_torch(src, g, oh, ow, two=None, ops=(), mean=MEAN, std=STD, dtype=np.float64):
    import torch
    import torch.nn.functional as F
    td = torch.float64 if dtype is np.float64 else torch.float32
    img = torch.from_numpy(np.ascontiguousarray(src)).permute(0, 3, 1, 2).to(td) / 255.
    img = img[:, :, g.box_y:g.box_y + g.box_h, g.box_x:g.box_x + g.box_w]
    if two is None:
        img = F.interpolate(img, size=(g.rh, g.rw), mode="bicubic", align_corners=False, antialias=True)
    else:
        img = F.interpolate(img, size=(two.mid_h, two.mid_w), mode="bilinear", align_corners=False, antialias=True)
        img = img[:, :, two.crop_y:two.crop_y + two.crop_h, two.crop_x:two.crop_x + two.crop_w]
        img = F.interpolate(img, size=(g.rh, g.rw), mode="bilinear", align_corners=False, antialias=True)
    img = img[:, :, g.top:g.top + oh, g.left:g.left + ow]
    if g.flip:
        img = img.flip(-1)
    for name, f in ops:
        img = _color_torch(img, name, f)
    m, s = torch.tensor(mean, dtype=td), torch.tensor(std, dtype=td)
    return ((img - m[:, None, None]) / s[:, None, None]).numpy()


# ----------------------------------------------------------------------------------------------------------- the case table
# name -> (oh, ow, [(T, H, W, geometry, two, ops), ...]); the first ten are frame_transform_ref's geometries (frame_224 is left to
# the probe: its 224 x 224 output adds no path the smaller cases lack), every size the smallest that still takes the path it names
Video = namedtuple("Video", "T H W geometry two ops")


def _one(T, H, W, g, two=None, ops=()):
    return Video(T, H, W, g, two, tuple(ops))


_SHARED = ("down_odd", "up_9x4", "one_pixel", "two_by_three", "squash_pair", "identity", "wide_1280", "box", "box_flip", "four_videos")
# RandomResizedCrop's box of a 40 x 50 source, flipped, with the three colour ops in a drawn order (hue first)
_TRAIN = P(7, 9, 21, 30, True, (3, 0, 2, 1), 1.2, 0.7, -0.2)
_SPECS = {
    **{n: (R._SPECS[n][0], R._SPECS[n][1], [_one(T, H, W, g) for T, H, W, g in R._SPECS[n][2]]) for n in _SHARED},
    # 3.27 x / 5.82 x down: 2 ceil(2 scale) + 1 = 15 / 25 table columns, 14 / 24 taps; the 22 output columns read 128 source
    # columns, the 22 rows 72 source rows: a footprint wider and taller than one staged chunk has to be
    "taps_72x128": (22, 22, [_one(1, 72, 128, R.full(72, 128, 22, 22))]),
    # down on one axis (40 -> 39), up on the other (50 -> 51)
    "down_up_40x50": (39, 51, [_one(2, 40, 50, R.full(40, 50, 39, 51))]),
    # two-stage with a 3 x stage-1 reduction: Resize(24, 32), CenterCrop(21, 28) at top round(3 / 2) = 2, left 2, Resize(20, 20)
    "two_stage_3x": (20, 20, [_one(2, 72, 96, G(0, 0, 72, 96, 20, 20, 0, 0, 0), Two(24, 32, 2, 2, 21, 28))]),
    "train_color": (16, 20, [_one(2, 40, 50, G(_TRAIN.i, _TRAIN.j, _TRAIN.h, _TRAIN.w, 16, 20, 0, 0, 1), None, color_ops(_TRAIN))]),
}
TRAIN_PARAMS = _TRAIN

Case = namedtuple("Case", "name oh ow sources videos")
CASES = tuple(_SPECS)
_cases, _refs, _f32 = {}, {}, {}


def case(name):
    """the case's sources (uint8 [T, H, W, 3] ndarrays, seeded by the name) and per-video records; built once"""
    if name not in _cases:
        oh, ow, vids = _SPECS[name]
        rng = np.random.RandomState(sum(name.encode()))
        _cases[name] = Case(name, oh, ow, [rng.randint(0, 256, (v.T, v.H, v.W, 3)).astype(np.uint8) for v in vids], vids)
    return _cases[name]


def _stack(name, fn, dtype):
    c = case(name)
    return np.concatenate([fn(s, v.geometry, c.oh, c.ow, v.two, v.ops, dtype=dtype) for s, v in zip(c.sources, c.videos)])


def case_reference(name):
    """float64 [sum of T, 3, oh, ow] of the case, in video order; computed once and shared (treat as read-only)"""
    if name not in _refs:
        _refs[name] = _stack(name, reference, np.float64)
        _refs[name].setflags(write=False)
    return _refs[name]


def float32_error(name):
    """max |float32 - float64|: torch's own float32 stack (``reference_torch`` in float32 on the CPU) against the definition"""
    if ("torch", name) not in _f32:
        got = _stack(name, reference_torch, np.float32)
        assert got.dtype == np.float32
        _f32["torch", name] = float(np.abs(got.astype(np.float64) - case_reference(name)).max())
    return _f32["torch", name]


def color_float32_error(name):
    """as frame_augment_ref.float32_error: the larger float32 deviation of BOTH restatements (the gate of a case with colour ops)"""
    if ("both", name) not in _f32:
        got = _stack(name, reference, np.float32)
        assert got.dtype == np.float32
        _f32["both", name] = max(float32_error(name), float(np.abs(got.astype(np.float64) - case_reference(name)).max()))
    return _f32["both", name]
