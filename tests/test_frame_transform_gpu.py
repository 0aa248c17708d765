"""GPU: xp_frames_resize_norm / hip_ops.frames_resize_norm / utils.transforms.FrameTransform / PrefetchLoader(frame_transform=...)
against the fp64 definition of tests/frame_transform_ref.py (whose two restatements tests/test_frame_transform_cpu.py holds together).

Tolerance: with exact source coordinates the only errors are fp32 roundings of values bounded by (1.375^2 + 0.49) / 0.26 ~ 9.2
(1.375: the largest absolute weight sum of the A = -0.75 kernel, at t = 0.5); about 32 roundings of 2^-24 give 1.8e-5 -> 2e-5
ABSOLUTE, for every case.  The measured maxima are 1.2e-7 .. 1.1e-6, the 1280-wide case 6.0e-7 like the others:
were the coordinates formed in fp32, that case would carry ~1e-4 of t times the local slope."""
import os

import numpy as np
import pytest
import torch

from tests import frame_transform_ref as R
from tests.gpu_util import OUT
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

TOL = 2e-5


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
    if view == "every_second":                # frames 0, 2, 4, ...: stride_t doubled
        big = torch.randint(0, 256, (2 * T, Hh, W, 3), generator=g, dtype=torch.uint8)
        big[::2] = t
        return big.cuda()[::2]
    if view == "odd_offset":                  # THWC starting at byte 1 of its allocation: no tap row is dword-aligned with src
        flat = torch.randint(0, 256, (t.numel() + 3,), generator=g, dtype=torch.uint8)
        flat[1:1 + t.numel()] = t.reshape(-1)
        return flat.cuda()[1:1 + t.numel()].view(T, Hh, W, 3)
    raise KeyError(view)


def _geo(g):
    from xpretrain_amd import hip_ops as H
    return H.FrameGeometry(*g)


def _check(tag, got, want):
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: an output element was not written"
    d = float(np.abs(got - want).max())
    line = f"{tag}: max |fp32 kernel - fp64 definition| = {d:.2e} (bound {TOL:.0e})"
    print(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "frame_transform_errors.txt"), "a") as f:
        f.write(line + "\n")
    assert d <= TOL, line


def _run(name, view="THWC", out=None):
    from xpretrain_amd import hip_ops as H
    c = R.case(name)
    return H.frames_resize_norm([_dev(s, view) for s in c.sources], [_geo(g) for g in c.geometry], c.oh, c.ow, R.MEAN, R.STD, out=out)


@pytest.mark.parametrize("name", R.CASES)
def test_case_against_fp64(name):
    """(four_videos: T = 2, 1, 3, 2 at four resolutions in one call -- the reference is concatenated in video order)"""
    _check(name, _run(name), R.case_reference(name))


def test_identity_geometry_is_bit_exact():
    """t = 0 everywhere: the weights are exactly (0, 1, 0, 0), so the result is fp32 (u / 255 - mean) / std to the bit"""
    u = R.case("identity").sources[0].astype(np.float32).transpose(0, 3, 1, 2)
    m, s = np.asarray(R.MEAN, np.float32)[:, None, None], np.asarray(R.STD, np.float32)[:, None, None]
    want = (u / np.float32(255.0) - m) / s
    assert want.dtype == np.float32
    assert np.array_equal(_run("identity").cpu().numpy(), want)


@pytest.mark.parametrize("view", ["TCHW", "sliced", "every_second", "odd_offset"])
def test_layouts_are_just_strides(view):
    """(THWC, sliced, every_second and odd_offset have packed rows, which the kernel reads as aligned dwords where they fit the
    allocation; TCHW loads byte by byte: the same bits either way)"""
    got = _run("down_odd", view)
    _check(f"down_odd/{view}", got, R.case_reference("down_odd"))
    assert torch.equal(got, _run("down_odd"))


def test_more_videos_than_one_launch_takes():
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    n = L.XP_FRAMES_MAX_VIDEOS + 3
    rng = np.random.RandomState(5)
    srcs = [rng.randint(0, 256, (1, 3, 4, 3)).astype(np.uint8) for _ in range(n)]
    g = R.full(3, 4, 4, 4)
    got = H.frames_resize_norm([_dev(s) for s in srcs], _geo(g), 4, 4, R.MEAN, R.STD)
    _check("split", got, np.concatenate([R.reference(s, g, 4, 4) for s in srcs]))


def test_output_between_poisoned_guards():
    c = R.case("four_videos")
    frames = sum(s.shape[0] for s in c.sources)
    guard = Guarded(frames * 3 * c.oh, c.ow, torch.float32)
    out = guard.mat.view(frames, 3, c.oh, c.ow)
    _run("four_videos", out=out)
    torch.cuda.synchronize()
    guard.check("frames_resize_norm", frames * 3 * c.oh, c.ow)
    _check("four_videos/guarded", out, R.case_reference("four_videos"))


def test_two_runs_are_bit_equal_and_streams_do_not_matter():
    a = _run("frame_224")
    b = _run("frame_224")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_side = _run("frame_224")
    s.synchronize()
    assert torch.equal(a, b) and torch.equal(a, on_side)
    _check("frame_224/side stream", on_side, R.case_reference("frame_224"))


def test_frame_transform_shapes_layouts_and_lists():
    from xpretrain_amd.utils.transforms import FrameTransform, init_transform_dict_simple
    c, want = R.case("down_odd"), R.case_reference("down_odd")
    t = FrameTransform(16)
    one = t(_dev(c.sources[0]))
    assert one.shape == (2, 3, 16, 16)
    _check("FrameTransform/[T,H,W,3]", one, want)
    tchw = torch.from_numpy(c.sources[0]).permute(0, 3, 1, 2).contiguous().cuda()
    assert torch.equal(t(tchw, layout="TCHW"), one)
    stacked = t(torch.stack([_dev(c.sources[0]), _dev(c.sources[0]).flip(0)]))
    assert stacked.shape == (2, 2, 3, 16, 16) and torch.equal(stacked[0], one) and torch.equal(stacked[1], one.flip(0))
    four = R.case("four_videos")          # a list: videos 0 and 3 have two frames each and different resolutions
    both = t([_dev(four.sources[0]), _dev(four.sources[3])])
    ref4 = R.case_reference("four_videos")
    assert both.shape == (2, 2, 3, 16, 16)
    _check("FrameTransform/list", both.view(4, 3, 16, 16), np.concatenate([ref4[:2], ref4[6:8]]))
    sq = R.case("squash_pair")
    pair = init_transform_dict_simple(input_res=(24, 40))["val"](_dev(sq.sources[0]))
    _check("FrameTransform/pair", pair, R.case_reference("squash_pair"))
    with pytest.raises(ValueError, match="same number of frames"):
        t([_dev(four.sources[0]), _dev(four.sources[1])])


@pytest.mark.parametrize("stream", [None, "text"])
def test_loader_hands_over_transformed_batches(stream):
    """a two-batch list dataset of decoded uint8 videos: what the loader yields under both keys is bit for bit the transform applied
    directly, and a tiny VidCLIP takes the batch as it comes"""
    from oracle import clipvip_oracle as O
    from tests.gpu_util import ModelArgs
    from xpretrain_amd.modeling import VidCLIP
    from xpretrain_amd.modeling.CLIP_ViP import CLIPModel
    from xpretrain_amd.utils.prefetch import PrefetchLoader
    from xpretrain_amd.utils.transforms import init_transform_dict_simple
    g = torch.Generator().manual_seed(8)
    sizes = [[(37, 53), (24, 31)], [(50, 40), (36, 36)]]
    host = []
    for b, hw in enumerate(sizes):
        _, ids, mask = O.synthetic_inputs(2, 3, 32, 12, vocab=120, seed=40 + b)
        host.append({"video": [torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8) for h, w in hw],
                     "image": torch.randint(0, 256, (2, 1, 45, 60, 3), generator=g, dtype=torch.uint8),
                     "text_input_ids": ids, "text_input_mask": mask,
                     "caption_ids": ids.flip(0)[:, None].contiguous(), "caption_masks": mask.flip(0)[:, None].contiguous()})
    transform = init_transform_dict_simple(input_res=32)["train"]
    torch.manual_seed(0)
    model = VidCLIP(ModelArgs(O.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64), 3)).cuda()
    CLIPModel._deferred_text_work.clear()
    seen = 0
    for want, got in zip(host, PrefetchLoader(host, stream=stream, frame_transform=transform)):
        assert isinstance(want["video"], list) and want["video"][0].dtype == torch.uint8          # the loader's batch is untouched
        assert got["video"].shape == (2, 3, 3, 32, 32) and got["image"].shape == (2, 1, 3, 32, 32)
        assert got["video"].dtype == got["image"].dtype == torch.float32
        assert torch.equal(got["video"], transform([v.cuda() for v in want["video"]]))
        assert torch.equal(got["image"], transform(want["image"].cuda()))
        assert torch.equal(got["text_input_ids"].cpu(), want["text_input_ids"])
        with torch.no_grad():
            out = model(**got)
        for k in ("vis_features", "text_features", "img_features", "cap_features"):
            assert out[k].shape == (2, 64) and torch.isfinite(out[k]).all(), k
        seen += 1
    assert seen == 2
    CLIPModel._deferred_text_work.clear()


def test_loader_without_a_transform_leaves_uint8_alone():
    from xpretrain_amd.utils.prefetch import PrefetchLoader
    host = [{"video": torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)}]
    (got,) = list(PrefetchLoader(host))
    assert got["video"].dtype == torch.uint8 and got["video"].is_cuda
