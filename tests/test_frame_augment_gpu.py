"""GPU: xp_frames_transform / hip_ops.frames_transform / utils.transforms.AugmentTransform and TwoStageTransform /
PrefetchLoader(frame_transform=<train transform>) against the fp64 definition of tests/frame_augment_ref.py (whose two restatements
tests/test_frame_augment_cpu.py holds together), through ``params=`` records: nothing here depends on a random draw.

Tolerance.  Paths WITHOUT a colour stage keep xp_frames_resize_norm's bound, 2e-5 absolute: the same derivation (tests/
test_frame_transform_gpu.py) with at most 16 products of weights in [-0.3, 1.2] (cubic) or [0, 1] (two-stage: each weight is a
product of two fractions, one more rounding) and values <= 255, then / 255 / std.  Paths WITH a colour stage: the definition run in
float32 on the CPU (both restatements, the larger error) differs from float64 by at most 7.91e-6 over the colour cases (per case:
DESIGN.md 7e; the hue cases 2e-6 .. 8e-6, brightness / saturation alone below 1e-6); the gate is four times that, 3.16e-5 -- the
margin covers a different but valid fp32 operation order and fused multiply-adds -- and is computed by ``frame_augment_ref.color_gate``
at run time, not copied here.  Measured on an MI355X (max |fp32 kernel - fp64 definition|): without a colour stage 4.3e-7 .. 6.2e-7;
brightness / saturation alone 1.9e-7 .. 6.7e-7, hue 1.9e-6 .. 2.0e-6, the six orders 1.3e-6 .. 2.5e-6, greys 2.9e-7, the checkerboard
2.1e-6 .. 3.2e-6, two-stage with colour ops 8.7e-7: maximum 3.22e-6.  No case and no pixel is excluded: the branches of the hue
conversion are continuous across their boundaries."""
import os

import numpy as np
import pytest
import torch

from tests import frame_augment_ref as A
from tests import frame_transform_ref as R
from tests.gpu_util import OUT
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _tol(name):
    return A.color_gate() if A.spec(name).ops else TOL


def _check(tag, got, want, tol):
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: an output element was not written (or is not finite)"
    d = float(np.abs(got - want).max())
    line = f"{tag}: max |fp32 kernel - fp64 definition| = {d:.2e} (bound {tol:.2e})"
    print(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "frame_augment_errors.txt"), "a") as f:
        f.write(line + "\n")
    assert d <= tol, line


def _params(p):
    from xpretrain_amd.utils.transforms import AugmentParams
    return AugmentParams(*p)


def _run(name, layout="THWC", out=None):
    """the case through the public surface its kind names"""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd.utils import transforms as T
    s = A.spec(name)
    src = torch.from_numpy(A.source(name))
    dev = src.cuda() if layout == "THWC" else src.permute(0, 3, 1, 2).contiguous().cuda()
    if s.kind == "val":
        return T.init_transform_dict(video_res=s.video_res, input_res=s.input_res)["val"](dev, layout=layout)
    if s.kind == "train":
        return T.init_transform_dict_image(input_res=s.input_res)["train"](dev, layout=layout, params=_params(s.params))
    if layout == "TCHW":
        dev = dev.permute(0, 2, 3, 1)
    return H.frames_transform([dev], H.FrameGeometry(*s.geometry), s.oh, s.ow, R.MEAN, R.STD, out=out,
                              two_stage=H.FrameTwoStage(*s.two), color=[s.ops])


@pytest.mark.parametrize("name", A.CASES)
def test_case_against_fp64(name):
    _check(name, _run(name), A.case_reference(name), _tol(name))


@pytest.mark.parametrize("name", ["two_stage_37x53", "crop_flip_no_color", "order_hsb", "checker_hue_first", "two_stage_color"])
def test_layouts_and_runs_agree_to_the_bit(name):
    """THWC and TCHW views feed the same bytes to the same arithmetic; two runs are bit-equal"""
    a = _run(name)
    assert torch.equal(a, _run(name)) and torch.equal(a, _run(name, "TCHW"))


@pytest.mark.parametrize("name", ["box_flip", "four_videos"])
def test_bicubic_without_colour_is_the_old_entry_point(name):
    from xpretrain_amd import hip_ops as H
    c = R.case(name)
    vids, geo = [torch.from_numpy(s).cuda() for s in c.sources], [H.FrameGeometry(*g) for g in c.geometry]
    old = H.frames_resize_norm(vids, geo, c.oh, c.ow, R.MEAN, R.STD)
    new = H.frames_transform(vids, geo, c.oh, c.ow, R.MEAN, R.STD)
    assert torch.equal(old, new)
    # (and inside a launch that carries another video's colour ops: a video without ops keeps the bits)
    ops = [()] * (len(vids) - 1) + [(("hue", 0.2),)]
    mixed = H.frames_transform(vids, geo, c.oh, c.ow, R.MEAN, R.STD, color=ops)
    last = c.sources[-1].shape[0]
    assert torch.equal(mixed[:-last], old[:-last]) and (len(vids) == 1 or not torch.equal(mixed[-last:], old[-last:]))


def test_more_videos_than_one_launch_takes():
    """per-video records, more videos than XP_FRAMES_TRANSFORM_MAX_VIDEOS: the split batch equals the per-video results"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd.utils.transforms import AugmentParams, init_transform_dict
    n = L.XP_FRAMES_TRANSFORM_MAX_VIDEOS + 3
    rng = np.random.RandomState(5)
    vids = [torch.from_numpy(rng.randint(0, 256, (1, 5, 6, 3)).astype(np.uint8)).cuda() for _ in range(n)]
    orders = list(A.ORDERS.values())
    recs = [AugmentParams(k % 2, k % 3, 4, 4 - k % 2, bool(k % 2), orders[k % 6], 0.8 + 0.02 * k, None if k % 4 == 0 else 1.3,
                          -0.5 + k / n) for k in range(n)]
    t = init_transform_dict(input_res=(4, 4))["train"]
    got = t(vids, params=recs)
    assert got.shape == (n, 1, 3, 4, 4)
    for k in range(n):
        assert torch.equal(got[k], t(vids[k], params=recs[k])), k
    k = n - 1                                  # one of them against fp64
    g = R.G(recs[k].i, recs[k].j, recs[k].h, recs[k].w, 4, 4, 0, 0, int(recs[k].flip))
    _check("split/last", got[k], A.reference(vids[k].cpu().numpy(), g, 4, 4, None, A.color_ops(recs[k])), A.color_gate())
    val = init_transform_dict(video_res=(5, 5), input_res=(4, 4))["val"]
    both = val(vids)
    for k in (0, L.XP_FRAMES_TRANSFORM_MAX_VIDEOS - 1, L.XP_FRAMES_TRANSFORM_MAX_VIDEOS, n - 1):
        assert torch.equal(both[k], val(vids[k])), k


@pytest.mark.parametrize("name", ["two_stage_color", "two_stage_wide"])
def test_output_between_poisoned_guards(name):
    from xpretrain_amd import hip_ops as H
    s = A.spec(name)
    guard = Guarded(s.T * 3 * s.oh, s.ow, torch.float32)
    out = guard.mat.view(s.T, 3, s.oh, s.ow)
    H.frames_transform([torch.from_numpy(A.source(name)).cuda()], H.FrameGeometry(*s.geometry), s.oh, s.ow, R.MEAN, R.STD, out=out,
                       two_stage=H.FrameTwoStage(*s.two), color=[s.ops])
    torch.cuda.synchronize()
    guard.check("frames_transform", s.T * 3 * s.oh, s.ow)
    _check(f"{name}/guarded", out, A.case_reference(name), _tol(name))


def test_train_output_between_poisoned_guards():
    from xpretrain_amd import hip_ops as H
    s = A.spec("checker_hue_last")
    guard = Guarded(s.T * 3 * s.oh, s.ow, torch.float32)
    out = guard.mat.view(s.T, 3, s.oh, s.ow)
    H.frames_transform([torch.from_numpy(A.source("checker_hue_last")).cuda()], H.FrameGeometry(*s.geometry), s.oh, s.ow, R.MEAN, R.STD,
                       out=out, color=[s.ops])
    torch.cuda.synchronize()
    guard.check("frames_transform", s.T * 3 * s.oh, s.ow)
    _check("checker_hue_last/guarded", out, A.case_reference("checker_hue_last"), A.color_gate())


def test_the_call_runs_on_the_current_stream():
    a = _run("order_shb")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_side = _run("order_shb")
        val_side = _run("two_stage_37x53")
    s.synchronize()
    assert torch.equal(a, on_side) and torch.equal(val_side, _run("two_stage_37x53"))
    _check("order_shb/side stream", on_side, A.case_reference("order_shb"), A.color_gate())


def test_shapes_lists_and_drawn_calls():
    """FrameTransform's calling convention; a call without params draws from the given generator exactly what draw() returns"""
    from xpretrain_amd.utils.transforms import init_transform_dict
    d = init_transform_dict(video_res=(20, 30), input_res=16, color_jitter=(0.4, 0.4, 0.1))
    t, val = d["train"], d["val"]
    g = torch.Generator().manual_seed(8)
    vids = [torch.randint(0, 256, (2, h, w, 3), generator=g, dtype=torch.uint8).cuda() for h, w in ((37, 53), (24, 31))]
    recs = t.draw(vids, generator=torch.Generator().manual_seed(77))
    drawn = t(vids, generator=torch.Generator().manual_seed(77))
    assert drawn.shape == (2, 2, 3, 16, 16) and torch.equal(drawn, t(vids, params=recs))
    assert torch.equal(drawn[1], t(vids[1], params=recs[1]))
    stacked = torch.stack([vids[0], vids[0].flip(0)])
    assert torch.equal(t(stacked, params=[recs[0]] * 2)[1], drawn[0].flip(0))
    out = val(vids)
    assert out.shape == (2, 2, 3, 16, 24) and torch.equal(out[0], val(vids[0]))
    with pytest.raises(ValueError, match="same number of frames"):
        t([vids[0], vids[1][:1]])
    with pytest.raises(ValueError, match="parameter records"):
        t(vids, params=recs[:1])


@pytest.mark.parametrize("stream", [None, "text"])
def test_loader_hands_over_augmented_batches(stream):
    """a two-batch list dataset of decoded uint8 videos through PrefetchLoader with the train transform and a seeded generator: what the
    loader yields is bit for bit the direct call with the same records -- drawn per batch for `video`, then for `image`"""
    from xpretrain_amd.modeling.CLIP_ViP import CLIPModel
    from xpretrain_amd.utils.prefetch import PrefetchLoader
    from xpretrain_amd.utils.transforms import init_transform_dict
    CLIPModel._deferred_text_work.clear()
    g = torch.Generator().manual_seed(8)
    sizes = [[(37, 53), (24, 31)], [(50, 40), (36, 36)]]
    host = [{"video": [torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8) for h, w in hw],
             "image": torch.randint(0, 256, (2, 1, 45, 60, 3), generator=g, dtype=torch.uint8),
             "text_input_ids": torch.arange(6).view(2, 3)} for hw in sizes]
    transform = init_transform_dict(input_res=32, color_jitter=(0.4, 0.4, 0.1))["train"]
    transform.generator = torch.Generator().manual_seed(31)
    replay = torch.Generator().manual_seed(31)
    seen = 0
    for want, got in zip(host, PrefetchLoader(host, stream=stream, frame_transform=transform)):
        rec_video = transform.draw(want["video"], generator=replay)
        rec_image = transform.draw(list(want["image"]), generator=replay)
        assert rec_video != rec_image[:2]
        assert got["video"].shape == (2, 3, 3, 32, 32) and got["image"].shape == (2, 1, 3, 32, 32)
        assert got["video"].dtype == got["image"].dtype == torch.float32
        assert torch.equal(got["video"], transform([v.cuda() for v in want["video"]], params=rec_video))
        assert torch.equal(got["image"], transform(want["image"].cuda(), params=rec_image))
        assert torch.equal(got["text_input_ids"].cpu(), want["text_input_ids"])
        seen += 1
    assert seen == 2
    CLIPModel._deferred_text_work.clear()
