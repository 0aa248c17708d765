#!/usr/bin/env python
"""Time of the augmenting and two-stage frame transforms (xp_frames_transform) beside the unchanged centre-crop launch
(xp_frames_resize_norm) at BASELINE config #2's batch: 8 videos x 12 frames of raw uint8 [T, H, W, 3] from each source resolution
-> fp32 [8, 12, 3, 224, 224].

Paths, each the C entry point alone on a descriptor table and an output built once (what the kernel takes back to back, plus the
host's argument checks, a few microseconds):
  simple      xp_frames_resize_norm: init_transform_dict_simple, the yardstick
  baseline    the same entry point of ANOTHER build of the library (--baseline-lib: the parent commit's), where given: the
              yardstick's own round-to-round spread and any drift of the unchanged path show here, in the same process
  train       xp_frames_transform, bicubic on a drawn RandomResizedCrop box (scale 0.8 .. 1) with flip, no colour ops
  train+cj    the same records with brightness, saturation and hue in a drawn order
  val         xp_frames_transform, two-stage bilinear: Resize(240, 320), CenterCrop(216, 288), Resize(224, 224)
and `call`, the train+cj transform as the loader calls it (draws, geometry, table, allocation, launch: the host part is inside).
Device events around `calls` back-to-back calls after `warmup` calls; `rounds` rounds with all paths and sources interleaved, so that
drift of the box lands on every path alike.  A path's figure means something only outside the spread of `simple`.  Alone on the GPU:
the cost beside a running training step is NOT measured here.

    python tools/frame_augment_probe.py [--calls 200] [--warmup 50] [--rounds 5] [--baseline-lib FILE] [--out FILE]
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
from xpretrain_amd.utils import transforms as T  # noqa: E402

B, FRAMES, RES = 8, 12, (224, 224)
SOURCES = ((240, 320), (360, 640))


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_augment_probe: needs an MI355X (a time taken anywhere else says nothing)")
    lib = L.lib()
    sig = L.SIGNATURES["xp_frames_resize_norm"]
    base = None
    if a.baseline_lib:
        base = C.CDLL(os.path.abspath(a.baseline_lib)).xp_frames_resize_norm
        base.restype, base.argtypes = sig
    simple = T.init_transform_dict_simple(input_res=RES)["train"]
    d = T.init_transform_dict(video_res=(240, 320), input_res=RES, color_jitter=(0.4, 0.4, 0.1))
    train, val = d["train"], d["val"]
    g = torch.Generator().manual_seed(7)
    batches = {hw: [torch.randint(0, 256, (FRAMES, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
               for hw in SOURCES}
    out = torch.empty((B * FRAMES, 3) + RES, dtype=torch.float32, device="cuda")
    mean, std = (C.c_float * 3)(*simple.mean), (C.c_float * 3)(*simple.std)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outp = C.c_void_p(out.data_ptr())
    tables, records = {}, {}
    for hw in SOURCES:
        v = batches[hw]
        recs = records[hw] = train.draw(v, generator=torch.Generator().manual_seed(hw[0]))
        geo = [train.geometry(hw[0], hw[1], p)[0] for p in recs]
        vg = [val.geometry(*hw) for _ in v]
        tables[hw] = {
            "simple": H.frame_table(v, [simple.geometry(*hw)[0]] * B),
            "train": H.frame_transform_table(v, geo),
            "train+cj": H.frame_transform_table(v, geo, color=[p.color_ops() for p in recs]),
            "val": H.frame_transform_table(v, [x[0] for x in vg], two_stage=[x[1] for x in vg]),
        }

    def launch(path, hw):
        if path == "simple":
            rc = lib.xp_frames_resize_norm(tables[hw]["simple"], B, mean, std, outp, RES[0], RES[1], stream)
        elif path == "baseline":
            rc = base(tables[hw]["simple"], B, mean, std, outp, RES[0], RES[1], stream)
        else:
            rc = lib.xp_frames_transform(tables[hw][path], B, mean, std, outp, RES[0], RES[1], stream)
        if rc != 0:
            raise RuntimeError(f"{path}: {lib.xp_last_error().decode()}")

    paths = ["simple"] + (["baseline"] if base else []) + ["train", "train+cj", "val"]
    lines = [f"frame transforms, {B} videos x {FRAMES} frames -> fp32 [{B}, {FRAMES}, 3, {RES[0]}, {RES[1]}]; the C entry point on a prebuilt "
             f"table, {a.calls} back-to-back calls after {a.warmup} warm-up calls, device events, {a.rounds} interleaved rounds; "
             f"crop records drawn with scale (0.8, 1.0), colour_jitter (0.4, 0.4, 0.1)"]
    if base:                                    # the unchanged path computes what the other build computes
        for hw in SOURCES:
            launch("baseline", hw)
            ref = out.clone()
            launch("simple", hw)
            assert torch.equal(ref, out), "xp_frames_resize_norm differs from the baseline library's"
        lines.append("xp_frames_resize_norm of this build and of the baseline library: outputs bit-equal on both sources")
    t = {(p, hw): [] for p in paths + ["call"] for hw in SOURCES}
    for r in range(a.rounds):
        for hw in SOURCES:
            for p in paths:
                t[p, hw].append(timed(lambda: launch(p, hw), a.warmup, a.calls))
            t["call", hw].append(timed(lambda: train(batches[hw]), a.warmup, a.calls))
            lines.append(f"round {r} source {hw[0]} x {hw[1]}: " + " | ".join(f"{p} {t[p, hw][-1]:6.1f}" for p in paths + ["call"]) + "  us")
    for hw in SOURCES:
        ref = statistics.median(t["simple", hw])
        spread = (max(t["simple", hw]) - min(t["simple", hw])) / ref * 100
        lines.append(f"source {hw[0]} x {hw[1]}: simple median {ref:6.1f} us, round-to-round spread {spread:.1f} %")
        for p in paths[1:] + ["call"]:
            m = statistics.median(t[p, hw])
            lines.append(f"    {p:9s} median {m:6.1f} us (min {min(t[p, hw]):6.1f}, max {max(t[p, hw]):6.1f}) = {m / ref:5.3f} x simple")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
