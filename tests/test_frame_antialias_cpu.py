"""CPU: the definition of the antialiased frame transforms (xp_frames_transform_aa, ``antialias=True``) and the Python surface around it.

The two fp64 restatements of tests/frame_antialias_ref.py -- scalar numpy from the stated formula, and the reference's torch calls in
float64 with ``antialias=True`` -- agree to 1e-12 over the case table, which pins the support, the truncated and renormalised window
at the border, Keys A = -0.5 and the two-stage path with its real intermediate image: what the GPU tests hold the kernel to.  The
surface: the factories and the transforms accept ``antialias`` and default to False, an ``antialias=False`` object resolves the
geometry it resolved before, CPU and float inputs still raise TypeError, and header, binding and library agree on the new symbols."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import frame_antialias_ref as A
from tests import frame_augment_ref as J
from tests import frame_transform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", A.CASES)
def test_the_two_restatements_agree(name):
    want = A.case_reference(name)
    got = A._stack(name, A.reference_torch, np.float64)
    assert got.shape == want.shape and got.dtype == np.float64
    d = float(np.abs(got - want).max())
    print(f"{name}: max |numpy - torch| in float64 = {d:.2e}")
    assert d <= 1e-12, d


def test_identity_is_exact():
    """box = out: the window is r - 1 .. r + 2 with f(-1), f(0), f(1), f(2) = 0, 1, 0, 0 exactly for A = -0.5, so the resized pixel is
    the source pixel and the result is fp64 (u / 255 - mean) / std to the bit"""
    c = A.case("identity")
    u = c.sources[0].astype(np.float64).transpose(0, 3, 1, 2)
    want = (u / 255.0 - np.asarray(R.MEAN)[:, None, None]) / np.asarray(R.STD)[:, None, None]
    assert np.array_equal(A.case_reference("identity"), want)
    for x0, w in A.axis_rows(12, 12, "bicubic")[2:-2]:
        assert list(w) == [0.0, 1.0, 0.0, 0.0]


def test_an_upscale_differs_from_the_point_sampled_definition():
    """no filter widens on an up-scale, but A (-0.5 against -0.75) and the border rule (a truncated, renormalised window against
    clamped taps) differ: 0.07 of the [0, 1] range on 9 x 4 -> 16 x 16 (torch's float64 interpolate, both ways).  The two definitions
    cannot be confused: the widest gate of the GPU tests (2.9e-4, the 1280-wide case) is more than two orders of magnitude below"""
    d = float(np.abs(A.case_reference("up_9x4") - R.case_reference("up_9x4")).max())
    print(f"up_9x4: max |antialias - point-sampled| = {d:.3f} (normalised units)")
    assert d > 0.05 / max(R.STD)                  # 0.05 of the [0, 1] range, in normalised units
    assert 4.0 * max(A.float32_error(n) for n in A.CASES) < 1e-2 * d


def test_a_downscale_differs_by_much_more():
    d = float(np.abs(A.case_reference("down_odd") - R.case_reference("down_odd")).max())
    assert d > 0.3 / max(R.STD)                   # 0.3 of the [0, 1] range


def test_two_stage_differs_from_the_point_sampled_two_stage():
    c = A.case("two_stage_3x")
    v = c.videos[0]
    old = J.reference(c.sources[0], v.geometry, c.oh, c.ow, v.two)
    assert float(np.abs(A.case_reference("two_stage_3x") - old).max()) > 0.1 / max(R.STD)


def test_table_rows_are_normalised_and_inside_the_box():
    for box, out, mode in ((1280, 224, "bicubic"), (720, 224, "bicubic"), (3840, 224, "bicubic"), (72, 24, "bilinear"), (9, 16, "bicubic")):
        rows = A.axis_rows(box, out, mode)
        assert all(x0 >= 0 and x0 + len(w) <= box and abs(w.sum() - 1.0) < 1e-14 for x0, w in rows)
    assert max(len(w) for _, w in A.axis_rows(3840, 224, "bicubic")) <= 70          # the widest geometry the header promises
    assert max(len(w) for _, w in A.axis_rows(128, 22, "bicubic")) == 24 and max(len(w) for _, w in A.axis_rows(72, 22, "bicubic")) == 14


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_factories_accept_antialias_and_default_to_false():
    from xpretrain_amd.utils import transforms as T
    for f in (T.init_transform_dict, T.init_transform_dict_simple, T.init_transform_dict_image):
        assert all(t.antialias is False for t in f().values())
        assert all(t.antialias is True for t in f(antialias=True).values())
        assert all(t.antialias is True for t in f((240, 320), (224, 224), (0.8, 1.0), (0, 0, 0), R.MEAN, R.STD, True).values())
        assert all(t.antialias is False for t in f(input_res=16, antialias=False).values())
        d = f(input_res=16, antialias=True)
        assert sorted(d) == ["test", "train", "val"] and len({id(t) for t in d.values()}) == 3
        # the reference's six parameters stay the introspected signature
        assert list(inspect.signature(f).parameters) == ["video_res", "input_res", "randcrop_scale", "color_jitter", "norm_mean", "norm_std"]
        with pytest.raises(TypeError):
            f(antialiased=True)
    for cls in (T.FrameTransform, T.TwoStageTransform, T.AugmentTransform):
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == "antialias" and p["antialias"].default is False
        assert cls().antialias is False and cls(antialias=True).antialias is True
    assert inspect.signature(__import__("xpretrain_amd.hip_ops", fromlist=["x"]).frames_transform).parameters["antialias"].default is False


def test_antialias_does_not_change_the_geometry():
    from xpretrain_amd.utils import transforms as T
    for aa in (False, True):
        d = T.init_transform_dict(video_res=(20, 30), input_res=16, antialias=aa)
        g, two, oh, ow = d["val"].geometry(37, 53)
        assert tuple(g) == (0, 0, 37, 53, 16, 24, 0, 0, 0) and tuple(two) == (20, 30, 1, 2, 18, 27) and (oh, ow) == (16, 24)
        p = T.AugmentParams(7, 9, 21, 30, True)
        assert tuple(d["train"].geometry(40, 50, p)[0]) == (7, 9, 21, 30, 16, 16, 0, 0, 1)
        g, oh, ow = T.init_transform_dict_simple(input_res=16, antialias=aa)["train"].geometry(37, 53)
        assert tuple(g) == (0, 0, 37, 53, 16, 22, 0, 3, 0) and (oh, ow) == (16, 16)
        recs = d["train"].draw([(37, 53), (24, 31)], generator=torch.Generator().manual_seed(3))
        assert recs == T.init_transform_dict(input_res=16)["train"].draw([(37, 53), (24, 31)], generator=torch.Generator().manual_seed(3))


def test_cpu_and_float_inputs_are_still_refused():
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.utils import transforms as T
    for f in (T.init_transform_dict, T.init_transform_dict_simple, T.init_transform_dict_image):
        for t in f(input_res=16, antialias=True).values():
            with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
                t(torch.zeros(2, 20, 30, 3, dtype=torch.uint8))
            with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
                t([torch.zeros(2, 20, 30, 3)])
            with pytest.raises(ValueError, match="layout"):
                t(torch.zeros(2, 20, 30, 3, dtype=torch.uint8), layout="HWC")
    with pytest.raises(TypeError, match="uint8 tensor on the GPU"):
        H.frames_transform([torch.zeros(2, 20, 30, 3, dtype=torch.uint8)], H.FrameGeometry(0, 0, 20, 30, 16, 24), 16, 16, antialias=True)


def test_header_and_binding_agree_on_the_new_symbols():
    from xpretrain_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "xpretrain_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("xp_frames_transform_aa", "xp_frames_transform_aa_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in L.SIGNATURES
    assert int(re.search(r"#define XP_FRAMES_AA_MAX_TAPS (\d+)", src).group(1)) == L.XP_FRAMES_AA_MAX_TAPS == 128
    res, args = L.SIGNATURES["xp_frames_transform_aa_workspace_bytes"]
    assert res is C.c_size_t and len(args) == 4
    res, args = L.SIGNATURES["xp_frames_transform_aa"]
    assert res is C.c_int32 and len(args) == 10 and args[8] is C.c_size_t
    assert args[:8] == L.SIGNATURES["xp_frames_transform"][1][:7] + [C.c_void_p]


# ------------------------------------------------------------------------------------------------ the sizing function (host only)
def _desc(H_src, W_src, g, two=None):
    from xpretrain_amd import _lib as L
    f = dict(src=0x10000, src_bytes=2 * H_src * W_src * 3, stride_t=H_src * W_src * 3, stride_y=W_src * 3, stride_x=3, stride_c=1, T=2,
             H=H_src, W=W_src, **g._asdict())
    e = L.XpFrameTransform(src=L.XpFrameSrc(**f), filter=0 if two is None else 1)
    if two is not None:
        e.mid_h, e.mid_w, e.crop_y, e.crop_x, e.crop_h, e.crop_w = two
    return e


def _bytes(descs, oh, ow):
    from xpretrain_amd import _lib as L
    tab = (L.XpFrameTransform * len(descs))(*descs)
    n = L.lib().xp_frames_transform_aa_workspace_bytes(tab, len(descs), oh, ow)
    return n, L.lib().xp_last_error().decode()


def test_workspace_size_is_the_tables():
    """per video and axis (2 + taps) words per output coordinate, taps = 2 ceil(support) + 1: 72 x 128 -> 22 x 22 has support 6.55 and
    11.64, 15 and 25 table columns; the two-stage 72 x 96 -> (24, 32) -> 21 x 28 -> 20 x 20 has stage-2 taps 2 ceil(1.05) + 1 = 5
    (1.4: 5) and stage-1 taps 7, a composite of ceil(3 * 4) + 7 = 19 on both axes"""
    n, _ = _bytes([_desc(72, 128, R.full(72, 128, 22, 22))], 22, 22)
    assert n == 4 * 22 * ((2 + 15) + (2 + 25))
    n, _ = _bytes([_desc(72, 96, R.G(0, 0, 72, 96, 20, 20, 0, 0, 0), J.Two(24, 32, 2, 2, 21, 28))], 20, 20)
    assert n == 4 * 20 * ((2 + 19) + (2 + 19))
    one, _ = _bytes([_desc(12, 20, R.full(12, 20, 12, 20))], 12, 20)
    assert one == 4 * (12 + 20) * (2 + 5)
    assert _bytes([_desc(72, 128, R.full(72, 128, 22, 22)), _desc(12, 20, R.full(12, 20, 22, 22))], 22, 22)[0] == \
        4 * 22 * (17 + 27) + 4 * 22 * 2 * (2 + 5)


def test_tap_limit():
    """3840 -> 224 bicubic passes (71 table columns); a support beyond XP_FRAMES_AA_MAX_TAPS is refused by both entry points' planning,
    naming the axis"""
    n, _ = _bytes([_desc(224, 3840, R.full(224, 3840, 224, 224))], 224, 224)
    assert n == 4 * 224 * ((2 + 5) + (2 + 71))
    n, msg = _bytes([_desc(8, 4000, R.full(8, 4000, 8, 100))], 8, 100)          # support 80: 161 columns
    assert n == 0 and "XP_FRAMES_AA_MAX_TAPS" in msg and "box_w" in msg and "videos_host[0]" in msg, msg
    n, msg = _bytes([_desc(2100, 8, R.full(2100, 8, 64, 8))], 64, 8)            # vertical: support 65.6, 133 columns
    assert n == 0 and "box_h" in msg, msg


@pytest.mark.parametrize("box, out", [(37, 16), (53, 22), (9, 16), (1, 8), (72, 22), (128, 22), (720, 224), (1280, 224), (3840, 224),
                                      (40, 39), (50, 51), (1000, 333), (500, 17)])
def test_table_width_covers_the_definitions_taps(box, out):
    """the library's table width of an axis, read back from the sizing function (the other axis is 1 -> 1: 5 columns), is
    2 ceil(support) + 1 and no row of the definition has more taps: the bound its LDS and workspace sizes rest on"""
    import math
    n, msg = _bytes([_desc(box, 1, R.full(box, 1, out, 1))], out, 1)
    assert n > 0, msg
    K = (n // 4 - (2 + 5)) // out - 2
    assert n == 4 * (out * (2 + K) + (2 + 5)) and K == 2 * math.ceil(2.0 * max(box / out, 1.0)) + 1
    assert max(len(w) for _, w in A.axis_rows(box, out, "bicubic")) <= K
