"""CPU: the frame transform's definition, geometry and refusals (xp_frames_resize_norm, xpretrain_amd.utils.transforms).

The two fp64 restatements of tests/frame_transform_ref.py -- numpy from the exact rational coordinate, and the reference's torch calls in
float64 -- agree to 1e-12 over the case table, which pins the coordinate, clamping, box and flip conventions the GPU tests hold the
kernel to.  The geometry resolver is checked against torchvision's results computed by hand; every refusal of the C entry point is
exercised through the loaded library (it answers before it touches a device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import frame_transform_ref as R


@pytest.mark.parametrize("name", R.CASES)
def test_the_two_fp64_restatements_agree(name):
    c = R.case(name)
    want = R.case_reference(name)
    got = np.concatenate([R.reference_torch(s, g, c.oh, c.ow) for s, g in zip(c.sources, c.geometry)])
    assert got.shape == want.shape == (sum(s.shape[0] for s in c.sources), 3, c.oh, c.ow)
    d = np.abs(got - want).max()
    print(f"{name}: max |numpy fp64 - torch fp64| = {d:.2e}")
    assert d <= 1e-12


def test_identity_geometry_is_the_plain_normalisation():
    c = R.case("identity")
    u = c.sources[0].astype(np.float64).transpose(0, 3, 1, 2)
    want = (u / 255.0 - np.asarray(R.MEAN)[:, None, None]) / np.asarray(R.STD)[:, None, None]
    assert np.abs(R.case_reference("identity") - want).max() <= 1e-14


def test_overshoot_is_kept():
    """the float path does not clamp: on random uint8 data the bicubic result leaves [0, 1] before the normalisation"""
    raw = R.case_reference("frame_224") * np.asarray(R.STD)[:, None, None] + np.asarray(R.MEAN)[:, None, None]
    assert raw.min() < -0.01 and raw.max() > 1.01


@pytest.mark.parametrize("hw, input_res, want", [
    ((240, 320), 224, (224, 298, 224, 224, 0, 37)),            # the issue's example: int(224 * 320 / 240) = 298, round(74 / 2) = 37
    ((240, 320), [224], (224, 298, 224, 224, 0, 37)),
    ((240, 320), (224, 224), (224, 224, 224, 224, 0, 0)),      # a pair squashes: exactly (h, w)
    ((360, 640), 224, (224, 398, 224, 224, 0, 87)),            # int(224 * 640 / 360) = int(398.2), round(174 / 2) = 87
    ((720, 1280), 224, (224, 398, 224, 224, 0, 87)),
    ((320, 240), 224, (298, 224, 224, 224, 37, 0)),            # portrait: the width is the shorter side
    ((37, 53), 16, (16, 22, 16, 16, 0, 3)),
    ((53, 37), 16, (22, 16, 16, 16, 3, 0)),
    ((24, 31), 16, (16, 20, 16, 16, 0, 2)),
    ((100, 105), 100, (100, 105, 100, 100, 0, 2)),             # (105 - 100) / 2 = 2.5 rounds to even: 2
    ((100, 107), 100, (100, 107, 100, 100, 0, 4)),             # 3.5 rounds to even: 4
    ((64, 48), (24, 40), (24, 40, 24, 40, 0, 0)),
    ((50, 50), 16, (16, 16, 16, 16, 0, 0)),
])
def test_geometry_follows_torchvision(hw, input_res, want):
    from xpretrain_amd.utils.transforms import resize_crop_geometry
    assert resize_crop_geometry(hw[0], hw[1], input_res) == want


def test_geometry_refuses_what_has_no_meaning():
    from xpretrain_amd.utils.transforms import FrameTransform, resize_crop_geometry
    with pytest.raises(ValueError):
        resize_crop_geometry(0, 10, 16)
    with pytest.raises(ValueError):
        resize_crop_geometry(10, 10, (1, 2, 3))
    with pytest.raises(ValueError):
        FrameTransform(layout="HWC")


def test_transform_dict_has_the_reference_signature():
    import inspect
    from xpretrain_amd.utils import transforms as T
    sig = inspect.signature(T.init_transform_dict_simple)
    assert list(sig.parameters) == ["video_res", "input_res", "randcrop_scale", "color_jitter", "norm_mean", "norm_std"]
    assert sig.parameters["input_res"].default == (224, 224) and sig.parameters["video_res"].default == (240, 320)
    assert sig.parameters["norm_mean"].default == (0.48145466, 0.4578275, 0.40821073)
    assert sig.parameters["norm_std"].default == (0.26862954, 0.26130258, 0.27577711)
    d = T.init_transform_dict_simple(input_res=[224, 224])
    assert sorted(d) == ["test", "train", "val"] and all(isinstance(t, T.FrameTransform) for t in d.values())
    g, oh, ow = d["train"].geometry(240, 320)
    assert (oh, ow) == (224, 224) and tuple(g) == (0, 0, 240, 320, 224, 224, 0, 0, 0)


def test_frame_transform_rejects_cpu_and_float_inputs():
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.utils.transforms import FrameTransform
    t = FrameTransform(16)
    with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
        t(torch.zeros(2, 20, 30, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
        t([torch.zeros(2, 20, 30, 3, dtype=torch.uint8)])
    with pytest.raises(TypeError, match="uint8 tensors on the GPU"):
        t(torch.zeros(2, 20, 30, 3))
    with pytest.raises(TypeError, match="uint8 tensor on the GPU"):
        H.frames_resize_norm([torch.zeros(2, 20, 30, 3, dtype=torch.uint8)], H.FrameGeometry(0, 0, 20, 30, 16, 24), 16, 16)
    with pytest.raises(TypeError, match="uint8 tensor on the GPU"):
        H.frames_resize_norm([torch.zeros(2, 20, 30, 3)], H.FrameGeometry(0, 0, 20, 30, 16, 24), 16, 16)


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


def _desc(**kw):
    """a valid descriptor of a contiguous [2, 20, 30, 3] video resized to (16, 24), window 16 x 16 at left 8: the window's last column
    (resized column 23, source coordinate 28.875) reaches the image's last column, so the last tap byte is the tensor's last byte"""
    from xpretrain_amd import _lib as L
    f = dict(src=_pointers()[0], src_bytes=2 * 20 * 30 * 3, stride_t=20 * 30 * 3, stride_y=30 * 3, stride_x=3, stride_c=1, T=2, H=20,
             W=30, box_y=0, box_x=0, box_h=20, box_w=30, rh=16, rw=24, top=0, left=8, flip=0)
    f.update(kw)
    return L.XpFrameSrc(**f)


def _call(descs, n=None, mean=R.MEAN, std=R.STD, out=None, oh=16, ow=16, null=()):
    from xpretrain_amd import _lib as L
    tab = (L.XpFrameSrc * max(len(descs), 1))(*descs)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    rc = L.lib().xp_frames_resize_norm(None if "videos" in null else tab, len(descs) if n is None else n,
                                       None if "mean" in null else m, None if "std" in null else s,
                                       C.c_void_p(_pointers()[1] if out is None else out), oh, ow, None)
    return rc, L.lib().xp_last_error().decode()


_MAXV = 32


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
def test_call_level_refusals(kw, word):
    rc, msg = _call([_desc()], **kw)
    assert rc == -1 and msg.startswith("xp_frames_resize_norm") and word in msg, msg


@pytest.mark.parametrize("kw, word", [
    (dict(src=0), "src is null"),
    (dict(src_bytes=0), "src_bytes"),
    (dict(T=0), "T="),
    (dict(H=0), "H="),
    (dict(W=-1), "W="),
    (dict(box_h=0), "box_h"),
    (dict(box_w=0), "box_w"),
    (dict(box_y=-1), "box_y"),
    (dict(box_y=1), "box_y"),                      # 1 + 20 > H
    (dict(box_x=5, box_w=26), "box_x"),            # 5 + 26 > W
    (dict(rh=0), "rh"),
    (dict(rw=0), "rw"),
    (dict(rh=15), "window"),                       # the 16-row window does not fit 15 resized rows: no padding path
    (dict(left=9), "window"),                      # 9 + 16 > 24
    (dict(top=-1), "window"),
    (dict(src_bytes=2 * 20 * 30 * 3 - 1), "src_bytes"),          # the last tap byte is at src_bytes
    (dict(stride_t=20 * 30 * 3 + 1), "stride_t"),
    (dict(stride_y=30 * 3 + 1), "stride_y"),
    (dict(stride_x=4), "stride_x"),
    (dict(stride_c=2), "stride_c"),
    (dict(stride_c=-1, left=0), "stride_c"),       # the window's first column reads source column 0: channel 2 lies in front of src
    (dict(stride_y=1 << 62), "stride_y"),          # overflows int64: an error code, not a wrapped address
])
def test_descriptor_refusals(kw, word):
    rc, msg = _call([_desc(), _desc(**kw)])
    assert rc == -1 and msg.startswith("xp_frames_resize_norm") and "videos_host[1]" in msg and word in msg, msg


def test_extent_is_the_farthest_tap_not_the_box():
    """a window that reads only the left part of a wide image needs only the bytes its taps reach; one byte fewer is refused"""
    from xpretrain_amd import _lib as L
    # identity geometry on a 4 x 100 image, window = columns 0 .. 9: the taps reach column 9 + 2 = 11
    d = dict(T=1, H=4, W=100, box_h=4, box_w=100, rh=4, rw=100, top=0, left=0, stride_t=1200, stride_y=300)
    last = 3 * 300 + 11 * 3 + 2
    rc, msg = _call([_desc(src_bytes=last, **d)], oh=4, ow=10)
    assert rc == -1 and "src_bytes" in msg
    assert L.XP_FRAMES_MAX_VIDEOS == _MAXV
