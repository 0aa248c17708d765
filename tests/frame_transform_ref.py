"""The fp64 definition of ``xp_frames_resize_norm`` (plain helper module, no tests of its own), twice:

``reference``: a restatement of the header's arithmetic in numpy, independent of torch.  The per-axis tap indices and weights are
formed coordinate by coordinate in scalar Python from the EXACT rational source coordinate (integer floor division; t = rem / den
is one fp64 rounding of an exact fraction), then the 4 x 4 taps are accumulated in a loop, rows first.

``reference_torch``: the reference's transform stack on a float tensor, line by line -- torchvision is not installed, and on a tensor
its transforms ARE these torch calls:
    dataset_video_retrieval.py:104   img_array.permute(0, 3, 1, 2).float() / 255.            (here .double())
    dataloader.py:218  Resize(input_res, BICUBIC)   -> F.interpolate(img, size=(rh, rw), mode="bicubic", align_corners=False)
                                                       (no antialias argument: the reference's torch 1.8 has none; no clamp)
    dataloader.py:219  CenterCrop(input_res)        -> img[..., top:top + oh, left:left + ow]
    dataloader.py:220  Normalize(mean, std)         -> (img - mean[:, None, None]) / std[:, None, None]
plus the two things only the kernel tests use: the resize applies to a source box, and a horizontal flip of the window.

``CASES``: the case table both test files share (sources are generated from a fixed seed, once)."""
from collections import namedtuple

import numpy as np

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
KEYS_A = -0.75

# the geometry fields of XpFrameSrc, in hip_ops.FrameGeometry's order
G = namedtuple("G", "box_y box_x box_h box_w rh rw top left flip")


def full(H, W, rh, rw, top=0, left=0, flip=0):
    return G(0, 0, H, W, rh, rw, top, left, flip)


def _keys(x):
    """Keys' cubic convolution kernel, A = -0.75"""
    x = abs(x)
    if x <= 1.0:
        return ((KEYS_A + 2.0) * x - (KEYS_A + 3.0)) * x * x + 1.0
    if x < 2.0:
        return ((KEYS_A * x - 5.0 * KEYS_A) * x + 8.0 * KEYS_A) * x - 4.0 * KEYS_A
    return 0.0


def axis_table(r0, n, box, out, box0):
    """taps [n, 4] (source indices) and weights [n, 4] (fp64) of resized coordinates r0 .. r0 + n - 1"""
    taps, w = np.zeros((n, 4), np.int64), np.zeros((n, 4), np.float64)
    for k in range(n):
        num, den = (2 * (r0 + k) + 1) * box - out, 2 * out          # s = num / den = (r + 0.5) * box / out - 0.5, exactly
        i = num // den                                              # Python: a true floor
        t = (num - i * den) / den
        for j in range(4):
            taps[k, j] = box0 + min(max(i - 1 + j, 0), box - 1)
            w[k, j] = _keys(t + 1 - j)
    return taps, w


def reference(src, g, oh, ow, mean=MEAN, std=STD):
    """src: uint8 ndarray [T, H, W, 3]; returns float64 [T, 3, oh, ow]"""
    src = np.asarray(src).astype(np.float64)
    ty, wy = axis_table(g.top, oh, g.box_h, g.rh, g.box_y)
    tx, wx = axis_table(g.left, ow, g.box_w, g.rw, g.box_x)
    if g.flip:                                  # output column x shows resized column left + ow - 1 - x
        tx, wx = tx[::-1], wx[::-1]
    acc = np.zeros((src.shape[0], oh, ow, 3), np.float64)
    for j in range(4):
        row = np.zeros_like(acc)
        for i in range(4):
            row += wx[None, None, :, i, None] * src[:, ty[:, j]][:, :, tx[:, i]]
        acc += wy[None, :, j, None, None] * row
    out = (acc / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def reference_torch(src, g, oh, ow, mean=MEAN, std=STD):
    import torch
    import torch.nn.functional as F
    img = torch.from_numpy(np.ascontiguousarray(src)).permute(0, 3, 1, 2).double() / 255.
    img = img[:, :, g.box_y:g.box_y + g.box_h, g.box_x:g.box_x + g.box_w]
    img = F.interpolate(img, size=(g.rh, g.rw), mode="bicubic", align_corners=False)
    img = img[:, :, g.top:g.top + oh, g.left:g.left + ow]
    if g.flip:
        img = img.flip(-1)
    m, s = torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64)
    return ((img - m[:, None, None]) / s[:, None, None]).numpy()


# ----------------------------------------------------------------------------------------------------------- the case table
# name -> (oh, ow, [(T, H, W, geometry), ...]); every size is the smallest that still takes the path the name describes
_SPECS = {
    # 37 x 53, shorter side to 16: resized (16, int(16 * 53 / 37) = 22), centre crop 16 x 16 at left = round(6 / 2) = 3
    "down_odd": (16, 16, [(2, 37, 53, full(37, 53, 16, 22, 0, 3))]),
    # up-scale: the first source coordinates are negative (0.5 * 9 / 16 - 0.5), taps clamp at both ends of both axes
    "up_9x4": (16, 16, [(1, 9, 4, full(9, 4, 16, 16))]),
    "one_pixel": (8, 8, [(1, 1, 1, full(1, 1, 8, 8))]),
    "two_by_three": (8, 8, [(2, 2, 3, full(2, 3, 8, 8))]),
    "squash_pair": (24, 40, [(1, 64, 48, full(64, 48, 24, 40))]),
    "identity": (12, 20, [(2, 12, 20, full(12, 20, 12, 20))]),
    # 3.5 column tiles of 64 and 56 row tiles per plane: many workgroups, a half-empty last wave
    "frame_224": (224, 224, [(1, 60, 80, full(60, 80, 224, 224))]),
    # source coordinates up to 1280: where scale * (r + 0.5) - 0.5 in fp32 loses 1e-4 of t
    "wide_1280": (4, 450, [(1, 4, 1280, full(4, 1280, 4, 450))]),
    "box": (16, 20, [(2, 40, 50, G(7, 9, 21, 30, 18, 26, 1, 3, 0))]),
    "box_flip": (16, 20, [(2, 40, 50, G(7, 9, 21, 30, 18, 26, 1, 3, 1))]),
    # four resolutions, shorter side to 16 and centre crop: (16, 22) left 3; (16, int(16 * 31 / 24) = 20) left 2;
    # (int(16 * 50 / 40) = 20, 16) top 2; identity
    "four_videos": (16, 16, [(2, 37, 53, full(37, 53, 16, 22, 0, 3)), (1, 24, 31, full(24, 31, 16, 20, 0, 2)),
                             (3, 50, 40, full(50, 40, 20, 16, 2, 0)), (2, 16, 16, full(16, 16, 16, 16))]),
}

Case = namedtuple("Case", "name oh ow sources geometry")
_cases = {}


def case(name):
    """the case's sources (uint8 [T, H, W, 3] ndarrays, seeded by the name) and geometry; built once"""
    if name not in _cases:
        oh, ow, vids = _SPECS[name]
        rng = np.random.RandomState(sum(name.encode()))
        _cases[name] = Case(name, oh, ow, [rng.randint(0, 256, (T, H, W, 3)).astype(np.uint8) for T, H, W, _ in vids],
                            [g for _, _, _, g in vids])
    return _cases[name]


CASES = tuple(_SPECS)
_refs = {}


def case_reference(name):
    """float64 [sum of T, 3, oh, ow] of the case, in video order; computed once and shared (treat as read-only)"""
    if name not in _refs:
        c = case(name)
        _refs[name] = np.concatenate([reference(s, g, c.oh, c.ow) for s, g in zip(c.sources, c.geometry)])
        _refs[name].setflags(write=False)
    return _refs[name]
