"""GPU: xp_frames_transform_aa / hip_ops.frames_transform(antialias=True) / the transforms and factories with ``antialias=True`` /
PrefetchLoader(frame_transform=<antialiased transform>) against the fp64 definition of tests/frame_antialias_ref.py (whose two
restatements tests/test_frame_antialias_cpu.py holds together).

Tolerance, per case and computed at run time: four times the deviation of torch's own float32 stack (``reference_torch`` in float32 on
the CPU, same inputs) from the fp64 definition -- the rule of tests/test_pos_resample_gpu.py; the margin is 4 because torch forms its
coordinates and weights in float32 and the kernel does not have to (its table is formed in fp64 and rounded once).  The case with
colour ops is gated as tests/test_frame_augment_gpu.py gates its colour cases: four times the float32 deviation of BOTH restatements,
the larger.  torch's float32 deviation on the CPU: 1.2e-7 (one_pixel) .. 7.1e-5 (wide_1280) in normalised units, so the gates are
4.6e-7 .. 2.9e-4.  Measured on an MI355X (max |fp32 kernel - fp64 definition|): 1.2e-7 (one_pixel), 2.8e-7 (identity, which is also
bit-exact against fp32 numpy), 5.4e-7 .. 7.6e-7 for every other case without a colour stage -- wide_1280 6.5e-7 like the others --,
1.9e-6 with flip and the three colour ops (gate 1.0e-5).  No case and no pixel is excluded."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import frame_antialias_ref as A
from tests import frame_transform_ref as R
from tests.gpu_util import OUT
from tests.guarded import Guarded, GuardedWorkspaces

pytestmark = pytest.mark.gpu


def _gate(name):
    c = A.case(name)
    return 4.0 * (A.color_float32_error(name) if any(v.ops for v in c.videos) else A.float32_error(name))


def _check(tag, got, want, tol):
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: an output element was not written (or is not finite)"
    d = float(np.abs(got - want).max())
    line = f"{tag}: max |fp32 kernel - fp64 definition| = {d:.2e} (bound {tol:.2e})"
    print(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "frame_antialias_errors.txt"), "a") as f:
        f.write(line + "\n")
    assert d <= tol, line


def _dev(src, view="THWC"):
    """the source ndarray [T, H, W, 3] on the device, indexed [T, H, W, 3], under the named memory layout"""
    t = torch.from_numpy(src)
    T, Hh, W, _ = t.shape
    if view == "THWC":
        return t.cuda()
    if view == "TCHW":
        return t.permute(0, 3, 1, 2).contiguous().cuda().permute(0, 2, 3, 1)
    g = torch.Generator().manual_seed(11)
    if view == "sliced":                      # columns 4 .. 4 + W of a wider tensor: stride_y exceeds the row
        big = torch.randint(0, 256, (T, Hh, W + 9, 3), generator=g, dtype=torch.uint8)
        big[:, :, 4:4 + W] = t
        return big.cuda()[:, :, 4:4 + W]
    if view == "odd_offset":                  # THWC starting at byte 1 of its allocation: the rows' dwords straddle both of its ends
        flat = torch.randint(0, 256, (t.numel() + 2,), generator=g, dtype=torch.uint8)
        flat[1:1 + t.numel()] = t.reshape(-1)
        return flat.cuda()[1:1 + t.numel()].view(T, Hh, W, 3)
    raise KeyError(view)


def _args(name, view="THWC"):
    from xpretrain_amd import hip_ops as H
    c = A.case(name)
    two = [H.FrameTwoStage(*v.two) for v in c.videos] if c.videos[0].two is not None else None
    color = [v.ops for v in c.videos] if any(v.ops for v in c.videos) else None
    return [_dev(s, view) for s in c.sources], [H.FrameGeometry(*v.geometry) for v in c.videos], two, color


def _run(name, view="THWC", out=None, antialias=True):
    from xpretrain_amd import hip_ops as H
    c = A.case(name)
    vids, geo, two, color = _args(name, view)
    return H.frames_transform(vids, geo, c.oh, c.ow, R.MEAN, R.STD, out=out, two_stage=two, color=color, antialias=antialias)


@pytest.mark.parametrize("name", A.CASES)
def test_case_against_fp64(name):
    _check(name, _run(name), A.case_reference(name), _gate(name))


def test_identity_geometry_is_bit_exact():
    """the table's rows are exactly (0, 1, 0, 0): fp32 (u / 255 - mean) / std to the bit"""
    u = A.case("identity").sources[0].astype(np.float32).transpose(0, 3, 1, 2)
    m, s = np.asarray(R.MEAN, np.float32)[:, None, None], np.asarray(R.STD, np.float32)[:, None, None]
    assert np.array_equal(_run("identity").cpu().numpy(), (u / np.float32(255.0) - m) / s)


@pytest.mark.parametrize("name", ["down_odd", "taps_72x128", "two_stage_3x", "train_color"])
def test_layouts_and_runs_agree_to_the_bit(name):
    """packed rows (THWC, sliced, odd_offset) are staged as aligned dwords where they lie inside the allocation, TCHW byte by byte:
    the same bytes to the same arithmetic in the same order"""
    a = _run(name)
    assert torch.equal(a, _run(name))
    for view in ("TCHW", "sliced", "odd_offset"):
        assert torch.equal(a, _run(name, view)), view


@pytest.mark.parametrize("name", ["box_flip", "four_videos", "two_stage_3x", "train_color"])
def test_antialias_false_returns_todays_bits(name):
    from xpretrain_amd import hip_ops as H
    c = A.case(name)
    vids, geo, two, color = _args(name)
    today = H.frames_transform(vids, geo, c.oh, c.ow, R.MEAN, R.STD, two_stage=two, color=color)
    assert torch.equal(today, _run(name, antialias=False))
    assert not torch.equal(today, _run(name))
    if two is None and color is None:
        assert torch.equal(today, H.frames_resize_norm(vids, geo, c.oh, c.ow, R.MEAN, R.STD))


def test_transforms_and_factories():
    """the three public transforms resolve the cases' geometry themselves; FrameTransform's calling convention holds"""
    from xpretrain_amd.utils import transforms as T
    c = A.case("two_stage_3x")
    val = T.init_transform_dict(video_res=(24, 32), input_res=(20, 20), antialias=True)["val"]
    _check("two_stage_3x/val", val(_dev(c.sources[0])), A.case_reference("two_stage_3x"), _gate("two_stage_3x"))
    c = A.case("train_color")
    train = T.init_transform_dict_image(input_res=(16, 20), antialias=True)["train"]
    got = train(_dev(c.sources[0], "TCHW").permute(0, 3, 1, 2), layout="TCHW", params=T.AugmentParams(*A.TRAIN_PARAMS))
    _check("train_color/train", got, A.case_reference("train_color"), _gate("train_color"))
    c = A.case("down_odd")
    simple = T.init_transform_dict_simple(input_res=16, antialias=True)["test"]
    one = simple(_dev(c.sources[0]))
    _check("down_odd/simple", one, A.case_reference("down_odd"), _gate("down_odd"))
    both = simple([_dev(c.sources[0]), _dev(c.sources[0][:, :24, :31].copy())])
    assert both.shape == (2, 2, 3, 16, 16) and torch.equal(both[0], one)
    assert not torch.equal(one, T.init_transform_dict_simple(input_res=16)["test"](_dev(c.sources[0])))
    with pytest.raises(ValueError, match="same number of frames"):
        simple([_dev(c.sources[0]), _dev(c.sources[0][:1])])


def test_more_videos_than_one_launch_takes():
    """more videos than XP_FRAMES_TRANSFORM_MAX_VIDEOS, five resolutions and hence five tap counts in one batch (2.5 x down to an
    up-scale): the split batch equals the per-video results, and three of them the fp64 definition"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd.utils.transforms import FrameTransform
    sizes = [(37, 53), (24, 31), (50, 40), (16, 16), (9, 12)]
    n = L.XP_FRAMES_TRANSFORM_MAX_VIDEOS + 3
    rng = np.random.RandomState(5)
    src = [rng.randint(0, 256, (1,) + sizes[k % 5] + (3,)).astype(np.uint8) for k in range(n)]
    vids = [torch.from_numpy(s).cuda() for s in src]
    t = FrameTransform(16, antialias=True)
    got = t(vids)
    assert got.shape == (n, 1, 3, 16, 16)
    for k in range(n):
        assert torch.equal(got[k], t(vids[k])), k
    for k in (0, L.XP_FRAMES_TRANSFORM_MAX_VIDEOS - 1, n - 1):
        g, oh, ow = t.geometry(*sizes[k % 5])
        want = A.reference(src[k], R.G(*g), oh, ow)
        f32 = A.reference_torch(src[k], R.G(*g), oh, ow, dtype=np.float32)
        _check(f"split/{k}", got[k], want, 4.0 * float(np.abs(f32.astype(np.float64) - want).max()))


@pytest.mark.parametrize("name", ["four_videos", "taps_72x128", "two_stage_3x", "train_color"])
def test_output_and_workspace_between_poisoned_guards(name):
    """the output at exactly its size, the tables at exactly xp_frames_transform_aa_workspace_bytes, both between poisoned guards"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    c = A.case(name)
    frames = sum(s.shape[0] for s in c.sources)
    guard = Guarded(frames * 3 * c.oh, c.ow, torch.float32)
    out = guard.mat.view(frames, 3, c.oh, c.ow)
    vids, geo, two, color = _args(name)
    want_bytes = L.lib().xp_frames_transform_aa_workspace_bytes(H.frame_transform_table(vids, geo, two, color), len(vids), c.oh, c.ow)
    with GuardedWorkspaces() as ws:
        _run(name, out=out)
    ws.check()
    guard.check("frames_transform(antialias=True)", frames * 3 * c.oh, c.ow)
    assert [(tag, nbytes) for tag, nbytes, _ in ws.records] == [("frames_aa", want_bytes)] and want_bytes > 0
    _check(f"{name}/guarded", out, A.case_reference(name), _gate(name))


def test_the_call_runs_on_the_current_stream():
    a, b = _run("taps_72x128"), _run("two_stage_3x")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_side, val_side = _run("taps_72x128"), _run("two_stage_3x")
    s.synchronize()
    assert torch.equal(a, on_side) and torch.equal(b, val_side)
    _check("taps_72x128/side stream", on_side, A.case_reference("taps_72x128"), _gate("taps_72x128"))


# ------------------------------------------------------------------------------------------------------------------- refusals
def _refusal_call(call=None, ws_bytes=None, ws_null=False, ws_shift=0, **desc):
    """xp_frames_transform_aa on one valid [2, 20, 30, 3] video (resized to (16, 24), window 16 x 16 at left 8, whose last tap is the
    tensor's last byte) with the named changes; ``ws_bytes`` maps the required size to the one passed.  Returns (rc, message, nothing
    was written to the poisoned output and workspace)."""
    from xpretrain_amd import _lib as L
    src = torch.zeros(2 * 20 * 30 * 3, dtype=torch.uint8, device="cuda")
    f = dict(src=src.data_ptr(), src_bytes=src.numel(), stride_t=20 * 30 * 3, stride_y=30 * 3, stride_x=3, stride_c=1, T=2, H=20, W=30,
             box_y=0, box_x=0, box_h=20, box_w=30, rh=16, rw=24, top=0, left=8, flip=0)
    e = dict(filter=0, mid_h=18, mid_w=27, crop_y=2, crop_x=3, crop_h=16, crop_w=24, n_color=0, color_op=(0, 0, 0),
             color_factor=(1.0, 1.0, 0.0))

    def table():
        return (L.XpFrameTransform * 1)(L.XpFrameTransform(src=L.XpFrameSrc(**f), **dict(
            e, color_op=(C.c_int32 * 3)(*e["color_op"]), color_factor=(C.c_float * 3)(*e["color_factor"]))))
    need = L.lib().xp_frames_transform_aa_workspace_bytes(table(), 1, 16, 16)
    assert need == 4 * 16 * 2 * (2 + 2 * 3 + 1)          # both axes: scale 1.25, support 2.5, 7 table columns
    for k, v in desc.items():
        (f if k in f else e)[k] = v
    kw = dict(dict(n=1, oh=16, ow=16, std=R.STD, out_null=False), **(call or {}))
    out = torch.full((2 * 3 * 16 * 16,), float("nan"), device="cuda")
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    m, s = (C.c_float * 3)(*R.MEAN), (C.c_float * 3)(*kw["std"])
    rc = L.lib().xp_frames_transform_aa(table(), kw["n"], m, s, C.c_void_p(0 if kw["out_null"] else out.data_ptr()), kw["oh"], kw["ow"],
                                        C.c_void_p(0 if ws_null else ws.data_ptr() + ws_shift), need if ws_bytes is None else ws_bytes(need),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = L.lib().xp_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, bool(torch.isnan(out).all()) and bool((ws == 0xA5).all())


def test_the_descriptor_of_the_refusal_tests_runs():
    """as it stands, with a larger workspace than needed, and at 121 table columns (30 -> 1: support 60), inside the limit"""
    for change in ({}, dict(ws_bytes=lambda need: need + 64)):
        rc, msg, untouched = _refusal_call(**change)
        assert rc == 0 and not untouched, msg
    from xpretrain_amd.utils.transforms import FrameTransform
    assert FrameTransform((16, 1), antialias=True)(torch.zeros(1, 20, 30, 3, dtype=torch.uint8, device="cuda")).shape == (1, 3, 16, 1)


@pytest.mark.parametrize("change, word", [
    (dict(ws_bytes=lambda need: need - 1), "workspace_bytes"),
    (dict(ws_bytes=lambda need: 0), "workspace_bytes"),
    (dict(ws_null=True), "workspace is null"),
    (dict(ws_shift=2), "4-byte aligned"),
    # 2100 -> 16 rows: support 262; the two-stage composite of 150 -> 1 -> 16: stage-1 support 150
    (dict(H=2100, box_h=2100, src_bytes=2 * 2100 * 30 * 3, stride_t=2100 * 30 * 3), "XP_FRAMES_AA_MAX_TAPS"),
    (dict(filter=1, mid_h=1, mid_w=1, crop_y=0, crop_x=0, crop_h=1, crop_w=1, H=150, box_h=150, src_bytes=2 * 150 * 30 * 3,
          stride_t=150 * 30 * 3), "XP_FRAMES_AA_MAX_TAPS"),
    # what xp_frames_transform refuses
    (dict(call=dict(out_null=True)), "out is null"),
    (dict(call=dict(n=0)), "n_videos"),
    (dict(call=dict(oh=0)), "oh"),
    (dict(call=dict(std=(0.2, 0.0, 0.2))), "std3_host[1]"),
    (dict(filter=2), "videos_host[0].filter"),
    (dict(src=0), "src is null"),
    (dict(box_x=1), "box_x"),
    (dict(left=9), "left"),
    (dict(filter=1, crop_x=4), "crop_x"),
    (dict(src_bytes=2 * 20 * 30 * 3 - 1), "src_bytes"),
    (dict(stride_t=20 * 30 * 3 + 1), "stride_t"),
    (dict(n_color=1, color_op=(1, 0, 0)), "color_op[0]"),
    (dict(n_color=1, color_op=(3, 0, 0), color_factor=(0.6, 1.0, 0.0)), "hue"),
])
def test_refusals_name_the_argument_and_launch_nothing(change, word):
    rc, msg, untouched = _refusal_call(**change)
    assert rc == -1 and msg.startswith("xp_frames_transform_aa:") and word in msg, (rc, msg)
    assert untouched, "a refused call wrote to the output or the workspace"


def test_binding_refuses_too_many_taps():
    from xpretrain_amd.utils.transforms import FrameTransform
    v = torch.zeros(1, 2100, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="XP_FRAMES_AA_MAX_TAPS"):
        FrameTransform((64, 8), antialias=True)(v)
    assert FrameTransform((64, 8))(v).shape == (1, 3, 64, 8)          # (the point-sampled path has no such limit)


@pytest.mark.parametrize("stream", [None, "text"])
def test_loader_hands_over_antialiased_batches(stream):
    """a two-batch list dataset of decoded uint8 videos through PrefetchLoader with the antialiased val transform: what the loader
    yields -- produced on its copy stream -- is bit for bit the direct call, and one video the fp64 definition"""
    from xpretrain_amd.modeling.CLIP_ViP import CLIPModel
    from xpretrain_amd.utils.prefetch import PrefetchLoader
    from xpretrain_amd.utils.transforms import init_transform_dict
    CLIPModel._deferred_text_work.clear()
    g = torch.Generator().manual_seed(8)
    sizes = [[(72, 96), (37, 53)], [(50, 40), (36, 36)]]
    host = [{"video": [torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8) for h, w in hw],
             "image": torch.randint(0, 256, (2, 1, 45, 60, 3), generator=g, dtype=torch.uint8),
             "text_input_ids": torch.arange(6).view(2, 3)} for hw in sizes]
    transform = init_transform_dict(video_res=(24, 32), input_res=(20, 20), antialias=True)["val"]
    plain = init_transform_dict(video_res=(24, 32), input_res=(20, 20))["val"]
    seen = 0
    for want, got in zip(host, PrefetchLoader(host, stream=stream, frame_transform=transform)):
        assert got["video"].shape == (2, 3, 3, 20, 20) and got["image"].shape == (2, 1, 3, 20, 20)
        assert got["video"].dtype == got["image"].dtype == torch.float32
        assert torch.equal(got["video"], transform([v.cuda() for v in want["video"]]))
        assert torch.equal(got["image"], transform(want["image"].cuda()))
        assert not torch.equal(got["video"], plain([v.cuda() for v in want["video"]]))
        assert torch.equal(got["text_input_ids"].cpu(), want["text_input_ids"])
        if seen == 0:
            geo, two, oh, ow = transform.geometry(72, 96)
            src = want["video"][0].numpy()
            ref = A.reference(src, R.G(*geo), oh, ow, A.Two(*two))
            f32 = A.reference_torch(src, R.G(*geo), oh, ow, A.Two(*two), dtype=np.float32)
            _check("loader/72x96", got["video"][0], ref, 4.0 * float(np.abs(f32.astype(np.float64) - ref).max()))
        seen += 1
    assert seen == 2
    CLIPModel._deferred_text_work.clear()
