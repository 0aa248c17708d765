"""CPU: the definition, the random draws, the geometry and the refusals of the augmenting and two-stage frame transforms
(xp_frames_transform, xpretrain_amd.utils.transforms.init_transform_dict / init_transform_dict_image).

The two fp64 restatements of tests/frame_augment_ref.py -- numpy from the exact rational coordinates, and the reference's torch calls in
float64 with torchvision's tensor-backend colour functions restated -- agree to 1e-12 over the case table, which pins the two-stage
coordinates, the clamping, and every branch of the colour ops the GPU tests hold the kernel to.  The draws are checked for what can be
checked without torchvision: determinism, boxes inside the image, the fallback branch on sizes where no try can succeed (computed by
hand from the algorithm), and that a None range takes no draw.  Every refusal of the C entry point is exercised through the loaded
library (it answers before it touches a device)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import frame_augment_ref as A
from tests import frame_transform_ref as R


@pytest.mark.parametrize("name", A.CASES)
def test_the_two_fp64_restatements_agree(name):
    s = A.spec(name)
    want = A.case_reference(name)
    got = A.reference_torch(A.source(name), s.geometry, s.oh, s.ow, s.two, s.ops)
    assert got.shape == want.shape == (s.T, 3, s.oh, s.ow)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    d = np.abs(got - want).max()
    print(f"{name}: max |numpy fp64 - torch fp64| = {d:.2e}")
    assert d <= 1e-12


def test_float32_definition_error_and_the_gate_it_sets():
    """(printed for DESIGN.md 7e: the figure the GPU gate of the colour paths is four times of)"""
    for name in A.CASES:
        print(f"{name}: max |fp32 definition - fp64 definition| = {A.float32_error(name):.2e}")
    worst = max(A.float32_error(n) for n in A.COLOR_CASES)
    print(f"colour cases: worst {worst:.2e}, gate {A.color_gate():.2e}")
    assert 0 < worst < 2e-5 and A.color_gate() == 4 * worst          # (a colour stage that loses more than the resize's bound is a bug)
    assert max(A.float32_error(n) for n in A.CASES if n not in A.COLOR_CASES) <= 2e-5


def test_case_table_covers_what_it_names():
    raw = A.resized(A.source("checker_hue_first"), A.spec("checker_hue_first").geometry, 20, 20)
    assert raw.min() < -0.05 and raw.max() > 1.05                    # the overshoot reaches the clamps from both sides
    assert (raw.max(-1) <= 0).any()                                  # ... with pixels whose maxc <= 0: outside torchvision's domain
    with np.errstate(all="ignore"):                                  # (the reason for the clamp in front of the hue op: at maxc == 0
        assert not np.isfinite(A.hue(np.array([[-0.1, -0.2, 0.0]]), 0.25, clamp=False)).all()          # _rgb2hsv divides by zero)
    assert np.isfinite(A.hue(raw, 0.25)).all() and np.isfinite(A.hue(np.array([[-0.1, -0.2, 0.0]]), 0.25)).all()
    g = A.source("greys")
    assert (g[..., 0] == g[..., 1]).all() and tuple(g[0, 0, 0]) == (0, 0, 0) and tuple(g[0, 0, 1]) == (255, 255, 255)
    orders = {tuple(n for n, _ in A.spec(f"order_{k}").ops) for k in ("bsh", "bhs", "sbh", "shb", "hbs", "hsb")}
    assert len(orders) == 6
    up = A.axis_table2(0, 16, 9, 20, 1, 18, 16, 0)[0]
    assert up.min() == 0 and up.max() == 8                           # the up-scaling first stage reaches both ends of the source


def test_two_stage_matches_the_issue_example():
    """37 x 53, video_res (20, 30), to 16 x 16: crop 18 x 27 at top 1, left 2"""
    from xpretrain_amd.utils.transforms import two_stage_geometry
    assert two_stage_geometry(37, 53, (20, 30), (16, 16)) == (20, 30, 1, 2, 18, 27, 16, 16)
    assert two_stage_geometry(37, 53, (20, 30), 16) == (20, 30, 1, 2, 18, 27, 16, 24)
    assert two_stage_geometry(360, 640, (240, 320), (224, 224)) == (240, 320, 12, 16, 216, 288, 224, 224)
    assert two_stage_geometry(37, 53, (30, 20), [16]) == (30, 20, 2, 1, 27, 18, 24, 16)          # portrait crop: the width is the shorter side
    with pytest.raises(ValueError):
        two_stage_geometry(37, 53, 20, 16)
    with pytest.raises(ValueError):
        two_stage_geometry(0, 53, (20, 30), 16)


@pytest.mark.parametrize("name", [n for n in A.CASES if A.spec(n).kind == "val"])
def test_val_transform_resolves_the_table_geometry(name):
    from xpretrain_amd.utils.transforms import init_transform_dict
    s = A.spec(name)
    d = init_transform_dict(video_res=s.video_res, input_res=s.input_res)
    for mode in ("val", "test"):
        g, two, oh, ow = d[mode].geometry(s.H, s.W)
        assert tuple(g) == tuple(s.geometry) and tuple(two) == tuple(s.two) and (oh, ow) == (s.oh, s.ow)


# ------------------------------------------------------------------------------------------------------------------ draws
def _train(**kw):
    from xpretrain_amd.utils.transforms import init_transform_dict
    return init_transform_dict(**kw)["train"]


def test_factories_have_the_reference_signature():
    import inspect
    from xpretrain_amd.utils import transforms as T
    for f in (T.init_transform_dict, T.init_transform_dict_image):
        sig = inspect.signature(f)
        assert list(sig.parameters) == ["video_res", "input_res", "randcrop_scale", "color_jitter", "norm_mean", "norm_std"]
        assert sig.parameters["video_res"].default == (240, 320) and sig.parameters["input_res"].default == (224, 224)
        assert sig.parameters["randcrop_scale"].default == (0.8, 1.0) and sig.parameters["color_jitter"].default == (0, 0, 0)
        assert sig.parameters["norm_mean"].default == R.MEAN and sig.parameters["norm_std"].default == R.STD
        d = f()
        assert sorted(d) == ["test", "train", "val"] and isinstance(d["train"], T.AugmentTransform)
    assert all(isinstance(T.init_transform_dict()[m], T.TwoStageTransform) for m in ("val", "test"))


def test_image_val_is_the_simple_stack():
    from xpretrain_amd.utils import transforms as T
    for res in ((224, 224), 224, [16]):
        a, b = T.init_transform_dict_image(input_res=res), T.init_transform_dict_simple(input_res=res)
        for mode in ("val", "test"):
            assert type(a[mode]) is T.FrameTransform
            for hw in ((240, 320), (360, 640), (320, 240)):
                assert a[mode].geometry(*hw) == b[mode].geometry(*hw)


def test_draws_are_deterministic_and_inside_the_image():
    t = _train(input_res=16, randcrop_scale=(0.08, 1.0), color_jitter=(0.4, 0.4, 0.1))
    sizes = [(37, 53), (24, 31), (50, 40), (16, 16), (5, 200), (1, 1)] * 6
    a = t.draw(sizes, generator=torch.Generator().manual_seed(3))
    b = t.draw(sizes, generator=torch.Generator().manual_seed(3))
    c = t.draw(sizes, generator=torch.Generator().manual_seed(4))
    assert a == b and a != c and len(a) == len(sizes)
    for (Hs, Ws), p in zip(sizes, a):
        assert 0 < p.h <= Hs and 0 < p.w <= Ws and 0 <= p.i <= Hs - p.h and 0 <= p.j <= Ws - p.w, (Hs, Ws, p)
        assert sorted(p.order) == [0, 1, 2, 3] and isinstance(p.flip, bool)
        assert 0.6 <= p.brightness <= 1.4 and 0.6 <= p.saturation <= 1.4 and -0.1 - 1e-7 <= p.hue <= 0.1 + 1e-7          # (fp32 ends)
        assert len(p.color_ops()) == 3
    assert {p.flip for p in a} == {False, True}
    torch.manual_seed(9)                                             # without a generator: torch's global one
    d = t.draw(sizes)
    torch.manual_seed(9)
    assert t.draw(sizes) == d


@pytest.mark.parametrize("hw, want", [((10, 200), (0, 93, 10, 13)), ((200, 10), (93, 0, 13, 10))])
def test_fallback_branch(hw, want):
    """scale (0.8, 1): the target area is at least 1600, so at 10 x 200 every try has h >= sqrt(1600 * 3 / 4) > 10 -- all ten fail;
    in_ratio 20 > 4/3: h = 10, w = int(round(10 * 4 / 3)) = 13, j = (200 - 13) // 2 = 93 (and transposed)"""
    t = _train()
    for seed in range(3):
        p = t.draw([hw], generator=torch.Generator().manual_seed(seed))[0]
        assert (p.i, p.j, p.h, p.w) == want
    from xpretrain_amd.utils.transforms import draw_crop
    assert draw_crop(30, 40, (4.0, 5.0)) == (0, 0, 30, 40)          # no try can succeed and the ratio is in range: the whole image


def test_no_jitter_means_no_colour_ops():
    t = _train()
    assert t.brightness is None and t.saturation is None and t.hue is None
    for p in t.draw([(37, 53)] * 5, generator=torch.Generator().manual_seed(1)):
        assert p.color_ops() == () and (p.brightness, p.saturation, p.hue) == (None, None, None)


def test_a_none_range_takes_no_draw():
    """the generator's state after a draw equals that of the hand-written call sequence: crop tries, torch.rand(1), torch.randperm(4)
    (always), then one uniform_ per range that is not None -- here saturation only"""
    t = _train(randcrop_scale=(0.2, 0.5), color_jitter=(0, 0.5, 0))          # (at most half the area: every try fits 240 x 320)
    assert t.brightness is None and t.saturation == (0.5, 1.5) and t.hue is None
    g, h = torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)
    p = t.draw([(10, 200)], generator=g)[0]                          # (h >= sqrt(400 * 3 / 4) > 10: exactly ten failed tries)
    for _ in range(10):
        torch.empty(1).uniform_(0.2, 0.5, generator=h)
        torch.empty(1).uniform_(math.log(3 / 4), math.log(4 / 3), generator=h)
    flip = bool(torch.rand(1, generator=h) < 0.5)
    order = tuple(int(k) for k in torch.randperm(4, generator=h))
    sat = torch.empty(1).uniform_(0.5, 1.5, generator=h).item()
    assert torch.equal(g.get_state(), h.get_state())
    assert (p.flip, p.order, p.brightness, p.saturation, p.hue) == (flip, order, None, sat, None)
    # a successful first try: two uniforms, two randints, then the same tail
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    p = t.draw([(240, 320)], generator=g)[0]
    area = 240 * 320 * torch.empty(1).uniform_(0.2, 0.5, generator=h).item()
    lr = torch.log(torch.tensor((3 / 4, 4 / 3)))
    ar = math.exp(torch.empty(1).uniform_(float(lr[0]), float(lr[1]), generator=h).item())
    w, hh = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
    assert 0 < w <= 320 and 0 < hh <= 240
    i = torch.randint(0, 240 - hh + 1, size=(1,), generator=h).item()
    j = torch.randint(0, 320 - w + 1, size=(1,), generator=h).item()
    torch.rand(1, generator=h), torch.randperm(4, generator=h), torch.empty(1).uniform_(0.5, 1.5, generator=h)
    assert (p.i, p.j, p.h, p.w) == (i, j, hh, w) and torch.equal(g.get_state(), h.get_state())


def test_video_and_image_draws_differ():
    """the loader calls the transform once per key: two calls on one generator are two independent sets of draws"""
    t = _train(color_jitter=(0.4, 0.4, 0.1))
    g = torch.Generator().manual_seed(12)
    video, image = t.draw([(37, 53)] * 2, generator=g), t.draw([(37, 53)] * 2, generator=g)
    assert video != image and video[0] != video[1]


def test_jitter_ranges_follow_torchvision():
    from xpretrain_amd.utils.transforms import jitter_range
    assert jitter_range(0.4, "brightness") == (0.6, 1.4)
    assert jitter_range(1.5, "saturation") == (0.0, 2.5)             # the lower end is clipped at 0
    assert jitter_range(0, "brightness") is None and jitter_range((1, 1), "saturation") is None
    assert jitter_range((0.5, 2), "brightness") == (0.5, 2.0)
    hue = dict(center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)
    assert jitter_range(0.5, "hue", **hue) == (-0.5, 0.5) and jitter_range(0, "hue", **hue) is None
    assert jitter_range((-0.1, 0.3), "hue", **hue) == (-0.1, 0.3)


@pytest.mark.parametrize("kw", [
    dict(color_jitter=(0, 0, 0.6)),                # hue > 0.5
    dict(color_jitter=(-0.1, 0, 0)),               # a negative brightness
    dict(color_jitter=(0, (2, 1), 0)),             # a range the wrong way round
    dict(color_jitter=(0, 0, (-0.6, 0.1))),
    dict(color_jitter=(0, 0)),
    dict(randcrop_scale=(1.0, 0.8)),               # a bad scale pair
    dict(randcrop_scale=(0.0, 1.0)),
    dict(randcrop_scale=0.8),
    dict(input_res=(1, 2, 3)),
])
def test_factory_refusals(kw):
    from xpretrain_amd.utils import transforms as T
    for f in (T.init_transform_dict, T.init_transform_dict_image):
        with pytest.raises(ValueError):
            f(**kw)


def test_transforms_reject_cpu_and_float_inputs():
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.utils.transforms import init_transform_dict
    d = init_transform_dict(input_res=16)
    for t in d.values():
        with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
            t(torch.zeros(2, 20, 30, 3, dtype=torch.uint8))
        with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
            t([torch.zeros(2, 20, 30, 3)])
        with pytest.raises(ValueError, match="layout"):
            t(torch.zeros(2, 20, 30, 3, dtype=torch.uint8), layout="HWC")
        with pytest.raises(ValueError, match="no frames"):
            t([])
    with pytest.raises(TypeError, match="uint8 tensor on the GPU"):
        H.frames_transform([torch.zeros(2, 20, 30, 3, dtype=torch.uint8)], H.FrameGeometry(0, 0, 20, 30, 16, 24), 16, 16)
    with pytest.raises(TypeError, match="uint8 tensor on the GPU"):
        H.frames_transform([torch.zeros(2, 20, 30, 3)], H.FrameGeometry(0, 0, 20, 30, 16, 24), 16, 16)


# -------------------------------------------------------------------------------------------------------------- identities
def _in_range_image():
    rng = np.random.RandomState(2)
    x = rng.randint(0, 256, (1, 9, 11, 3)).astype(np.float64) / 255.0
    x[0, 0, 0], x[0, 0, 1], x[0, 0, 2] = 0.0, 1.0, 0.5              # black, white, grey
    return x


def test_neutral_factors_are_the_identity():
    x = _in_range_image()
    y = A.hue(A.saturation(A.brightness(x, 1.0), 1.0), 0.0)
    assert np.abs(y - x).max() <= 1e-12
    y32 = A.hue(A.saturation(A.brightness(x.astype(np.float32), 1.0), 1.0), 0.0)
    assert y32.dtype == np.float32 and np.abs(y32 - x).max() <= 1e-6


def test_hue_clamp_is_the_identity_on_in_range_input():
    x = _in_range_image()
    for f in (-0.5, -0.2, 0.1, 0.5):
        assert np.array_equal(A.hue(x, f), A.hue(x, f, clamp=False))


# ------------------------------------------------------------------------------------------------------------- refusals
_bufs = []


def _pointers():
    """(src, out): every call below is refused before anything could read them, so without a device they are made-up non-null
    addresses.  Where there is a device they are real, generous buffers: should a refusal ever be missing, the launch it lets
    through then stays inside memory the test owns (and the test fails on the return code)."""
    if not torch.cuda.is_available():
        return 0x10000, 0x20000
    if not _bufs:
        _bufs.extend([torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"), torch.zeros(1 << 20, dtype=torch.float32, device="cuda")])
    return _bufs[0].data_ptr(), _bufs[1].data_ptr()


def _desc(filter=0, n_color=0, color_op=(0, 0, 0), color_factor=(1.0, 1.0, 0.0), mid_h=18, mid_w=27, crop_y=2, crop_x=3, crop_h=16,
          crop_w=24, **kw):
    """a valid descriptor of a contiguous [2, 20, 30, 3] video: as test_frame_transform_cpu.py's for the bicubic filter (resized to
    (16, 24), window 16 x 16 at left 8, whose last tap byte is the tensor's last byte); the two-stage fields -- (18, 27) stage-1
    image, its last 16 x 24 pixels at (2, 3) as the crop, resized to (16, 24) -- are valid too and read only with filter = 1"""
    from xpretrain_amd import _lib as L
    f = dict(src=_pointers()[0], src_bytes=2 * 20 * 30 * 3, stride_t=20 * 30 * 3, stride_y=30 * 3, stride_x=3, stride_c=1, T=2, H=20,
             W=30, box_y=0, box_x=0, box_h=20, box_w=30, rh=16, rw=24, top=0, left=8, flip=0)
    f.update(kw)
    return L.XpFrameTransform(src=L.XpFrameSrc(**f), filter=filter, mid_h=mid_h, mid_w=mid_w, crop_y=crop_y, crop_x=crop_x,
                              crop_h=crop_h, crop_w=crop_w, n_color=n_color, color_op=(C.c_int32 * 3)(*color_op),
                              color_factor=(C.c_float * 3)(*color_factor))


def _call(descs, n=None, mean=R.MEAN, std=R.STD, out=None, oh=16, ow=16, null=()):
    from xpretrain_amd import _lib as L
    tab = (L.XpFrameTransform * max(len(descs), 1))(*descs)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    rc = L.lib().xp_frames_transform(None if "videos" in null else tab, len(descs) if n is None else n,
                                     None if "mean" in null else m, None if "std" in null else s,
                                     C.c_void_p(_pointers()[1] if out is None else out), oh, ow, None)
    return rc, L.lib().xp_last_error().decode()


_MAXV = 24


def test_descriptor_table_size():
    from xpretrain_amd import _lib as L
    assert L.XP_FRAMES_TRANSFORM_MAX_VIDEOS == _MAXV and C.sizeof(L.XpFrameTransform) == 152 and C.sizeof(L.XpFrameSrc) == 96
    assert _MAXV * (C.sizeof(L.XpFrameTransform) + 4) + 24 + 64 <= 4096


@pytest.mark.parametrize("kw, word", [
    (dict(null=("videos",)), "videos_host"),
    (dict(null=("mean",)), "mean3_host"),
    (dict(null=("std",)), "std3_host"),
    (dict(out=0), "out"),
    (dict(n=0), "n_videos"),
    (dict(n=_MAXV + 1), "n_videos"),
    (dict(oh=0), "oh"),
    (dict(ow=-3), "ow"),
    (dict(std=(0.2, 0.0, 0.2)), "std3_host[1]"),
    (dict(std=(0.2, 0.2, -1.0)), "std3_host[2]"),
])
@pytest.mark.parametrize("filter", [0, 1])
def test_call_level_refusals(filter, kw, word):
    rc, msg = _call([_desc(filter)], **kw)
    assert rc == -1 and msg.startswith("xp_frames_transform") and word in msg, msg


_SRC_REFUSALS = [
    (dict(src=0), "src is null"),
    (dict(src_bytes=0), "src_bytes"),
    (dict(T=0), "T="),
    (dict(H=0), "H="),
    (dict(W=-1), "W="),
    (dict(box_h=0), "box_h"),
    (dict(box_w=0), "box_w"),
    (dict(box_y=-1), "box_y"),
    (dict(box_y=1), "box_y"),
    (dict(box_x=5, box_w=26), "box_x"),
    (dict(rh=0), "rh"),
    (dict(rw=0), "rw"),
    (dict(rh=15), "window"),
    (dict(left=9), "window"),
    (dict(top=-1), "window"),
    (dict(src_bytes=2 * 20 * 30 * 3 - 1), "src_bytes"),
    (dict(stride_t=20 * 30 * 3 + 1), "stride_t"),
    (dict(stride_y=30 * 3 + 1), "stride_y"),
    (dict(stride_x=4), "stride_x"),
    (dict(stride_c=2), "stride_c"),
    (dict(stride_c=-1, left=0), "stride_c"),
    (dict(stride_y=1 << 62), "stride_y"),
]


@pytest.mark.parametrize("kw, word", _SRC_REFUSALS + [
    (dict(filter=1), "filter"),                    # differs from video 0's
    (dict(n_color=-1), "n_color"),
    (dict(n_color=4), "n_color"),
    (dict(n_color=1, color_op=(1, 0, 0)), "color_op[0]"),            # contrast
    (dict(n_color=2, color_op=(0, 7, 0)), "color_op[1]"),
    (dict(n_color=2, color_op=(3, 3, 0), color_factor=(0.1, 0.1, 0.0)), "repeats"),
    (dict(n_color=1, color_op=(0, 0, 0), color_factor=(-0.5, 1.0, 0.0)), "color_factor[0]"),
    (dict(n_color=2, color_op=(0, 2, 0), color_factor=(1.0, float("nan"), 0.0)), "color_factor[1]"),
    (dict(n_color=1, color_op=(2, 0, 0), color_factor=(float("inf"), 1.0, 0.0)), "color_factor[0]"),
    (dict(n_color=1, color_op=(3, 0, 0), color_factor=(0.51, 1.0, 0.0)), "hue"),
    (dict(n_color=3, color_op=(0, 2, 3), color_factor=(1.0, 1.0, -0.6)), "color_factor[2]"),
])
def test_descriptor_refusals_bicubic(kw, word):
    rc, msg = _call([_desc(), _desc(**kw)])
    assert rc == -1 and msg.startswith("xp_frames_transform") and "videos_host[1]" in msg and word in msg, msg


@pytest.mark.parametrize("kw, word", [c for c in _SRC_REFUSALS if c[0] != dict(stride_c=-1, left=0)] + [
    (dict(filter=0), "filter"),
    (dict(mid_h=0), "mid_h"),
    (dict(mid_w=16385), "mid_w"),
    (dict(crop_h=0), "crop_h"),
    (dict(crop_w=-2), "crop_w"),
    (dict(crop_y=-1), "crop_y"),
    (dict(crop_y=3), "crop_y"),                    # 3 + 16 > 18
    (dict(crop_x=4), "crop_x"),                    # 4 + 24 > 27
    # (bicubic's stride_c = -1 case with the crop moved to the corner: stage-1 pixel (0, 0) reads source pixel (0, 0), whose channel 2
    #  then lies in front of src; with the crop at (2, 3) the first tap is source pixel (2, 3) and a negative stride_c stays inside)
    (dict(stride_c=-1, left=0, crop_y=0, crop_x=0), "stride_c"),
    (dict(n_color=1, color_op=(3, 0, 0), color_factor=(-0.7, 1.0, 0.0)), "hue"),
])
def test_descriptor_refusals_two_stage(kw, word):
    """(the window's last column -- stage-2 column 23 = stage-1 column 3 + 23 = 26, source coordinate 28.94 -- and its last row --
    stage-1 row 2 + 15 = 17, source coordinate 18.94 -- read the image's last pixel, so the src_bytes - 1 case holds for these taps)"""
    kw = dict(dict(filter=1), **kw)
    rc, msg = _call([_desc(filter=1), _desc(**kw)])
    assert rc == -1 and msg.startswith("xp_frames_transform") and "videos_host[1]" in msg and word in msg, msg


def test_unknown_filter_is_refused():
    rc, msg = _call([_desc(filter=2)])
    assert rc == -1 and "videos_host[0].filter" in msg


def test_two_stage_extent_is_the_farthest_tap():
    """identity two-stage geometry on a 4 x 100 image (stage 1 and 2 keep the size, the crop is the whole image), window = columns
    0 .. 9: the stage-2 neighbour of column 9 is stage-1 column 10, whose own neighbour is source column 11 (weight 0, but read)"""
    d = dict(filter=1, T=1, H=4, W=100, box_h=4, box_w=100, rh=4, rw=100, top=0, left=0, stride_t=1200, stride_y=300,
             mid_h=4, mid_w=100, crop_y=0, crop_x=0, crop_h=4, crop_w=100)
    last = 3 * 300 + 11 * 3 + 2
    rc, msg = _call([_desc(src_bytes=last, **d)], oh=4, ow=10)
    assert rc == -1 and "src_bytes" in msg
    ty, _ = A.axis_table2(0, 4, 4, 4, 0, 4, 4, 0)
    tx, _ = A.axis_table2(0, 10, 100, 100, 0, 100, 100, 0)
    assert ty.max() == 3 and tx.max() == 11
