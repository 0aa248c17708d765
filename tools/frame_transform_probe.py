#!/usr/bin/env python
"""Time of the decoded-frame transform (xp_frames_resize_norm) at BASELINE config #2's batch: 8 videos x 12 frames of raw uint8
[T, H, W, 3] from each source resolution -> fp32 [8, 12, 3, 224, 224] with the shipped input_res (224, 224).

Two figures per source, both device events around `calls` back-to-back calls after `warmup` calls, `rounds` rounds with the sources
interleaved:
  call    utils.transforms.FrameTransform as the loader calls it: geometry, descriptor table, output allocation and launch -- the
          host part of the call is inside the figure, and where it is the longer part the figure is the host's;
  launch  the C entry point alone on a descriptor table and an output built once: what the kernel takes back to back (plus the
          host's argument checks, a few microseconds).
Bytes: every source byte once (what a perfect cache hierarchy reads) and every output byte once; the rate is those bytes over the
launch time -- an end-to-end rate of the launch, not a share of peak.  Alone on the GPU: the cost beside a running training step is
NOT measured here.

    python tools/frame_transform_probe.py [--calls 200] [--warmup 50] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
from xpretrain_amd import _lib as L  # noqa: E402
from xpretrain_amd import hip_ops as H  # noqa: E402
from xpretrain_amd.utils.transforms import init_transform_dict_simple  # noqa: E402

B, T, RES = 8, 12, (224, 224)
SOURCES = ((240, 320), (360, 640), (720, 1280))


def timed(f, warmup, calls):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_transform_probe: needs an MI355X (a time taken anywhere else says nothing)")
    transform = init_transform_dict_simple(input_res=RES)["train"]
    g = torch.Generator().manual_seed(7)
    batches = {hw: [torch.randint(0, 256, (T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)] for hw in SOURCES}
    out = torch.empty((B * T, 3) + RES, dtype=torch.float32, device="cuda")
    mean, std = (C.c_float * 3)(*transform.mean), (C.c_float * 3)(*transform.std)
    tables = {hw: H.frame_table(batches[hw], [transform.geometry(*hw)[0]] * B) for hw in SOURCES}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(hw):
        L.check(L.lib().xp_frames_resize_norm(tables[hw], B, mean, std, C.c_void_p(out.data_ptr()), RES[0], RES[1], stream),
                "xp_frames_resize_norm")

    lines = [f"xp_frames_resize_norm, {B} videos x {T} frames -> fp32 [{B}, {T}, 3, {RES[0]}, {RES[1]}]; {a.calls} back-to-back calls after "
             f"{a.warmup} warm-up calls, device events, {a.rounds} interleaved rounds"]
    call, kern = {hw: [] for hw in SOURCES}, {hw: [] for hw in SOURCES}
    for r in range(a.rounds):
        for hw in SOURCES:
            call[hw].append(timed(lambda: transform(batches[hw]), a.warmup, a.calls))
            kern[hw].append(timed(lambda: launch(hw), a.warmup, a.calls))
            assert torch.equal(transform(batches[hw]).view_as(out), out) and bool(torch.isfinite(out).all())
            lines.append(f"round {r} source {hw[0]:4d} x {hw[1]:4d}: call {call[hw][-1]:7.1f} us | launch {kern[hw][-1]:7.1f} us")
    for hw in SOURCES:
        rd, wr = B * T * hw[0] * hw[1] * 3, B * T * 3 * RES[0] * RES[1] * 4
        mc, mk = statistics.median(call[hw]), statistics.median(kern[hw])
        lines.append(f"source {hw[0]:4d} x {hw[1]:4d}: call median {mc:7.1f} us = {B / mc * 1e6:7.0f} videos/s | launch median {mk:7.1f} us "
                     f"(spread {(max(kern[hw]) - min(kern[hw])) / mk * 100:.1f} %): read {rd / 1e6:6.1f} MB + written {wr / 1e6:5.1f} MB "
                     f"= {(rd + wr) / mk / 1e6:5.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
