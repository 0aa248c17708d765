#!/usr/bin/env python
"""Time of the antialiased frame transforms (xp_frames_transform_aa) beside the existing point-sampled launches at BASELINE config
#2's batch: 8 videos x 12 frames of raw uint8 [T, H, W, 3] from each source resolution -> fp32 [8, 12, 3, 224, 224].

Paths, each the C entry point alone on a descriptor table, an output and a workspace built once (what the kernels take back to back,
plus the host's argument checks and planning, a few microseconds):
  simple      xp_frames_resize_norm: init_transform_dict_simple, bicubic, the parent's launch
  simple+aa   xp_frames_transform_aa on the same geometry (table kernel + resample)
  val         xp_frames_transform, two-stage bilinear: Resize(240, 320), CenterCrop(216, 288), Resize(224, 224)
  val+aa      xp_frames_transform_aa on the same geometry (composite table rows)
and `call+aa`, FrameTransform(antialias=True) as the loader calls it (geometry, table, sizing, workspace, launch: the host part is
inside).  Device events around `calls` back-to-back calls after `warmup` calls; `rounds` rounds with all paths and sources interleaved
in one process, so that drift of the box lands on every path alike.  Rates are source-box bytes + output bytes per second: the
antialiased path reads every byte of the box, the point-sampled one a sparse subset of it, so only the antialiased rate is a memory
rate.  The table kernel's own time comes from the profiler's kernel records of a few calls (n/a where it records none).  Alone on
the GPU: the cost beside a running training step is NOT measured here.

    python tools/frame_antialias_probe.py [--calls 100] [--warmup 20] [--rounds 3] [--out FILE]
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


def kernel_times(f, calls=10):
    """{kernel name fragment: mean device microseconds} of the two kernels of one antialiased call, from the profiler"""
    from torch.profiler import ProfilerActivity, profile
    f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        for frag in ("aa_table_kernel", "aa_apply_kernel"):
            if frag in ev.name:
                t = getattr(ev, "device_time", None)
                out.setdefault(frag, []).append(t if t is not None else ev.cuda_time)
    return {k: sum(v) / len(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_antialias_probe: needs an MI355X (a time taken anywhere else says nothing)")
    lib = L.lib()
    simple = T.init_transform_dict_simple(input_res=RES)["train"]
    simple_aa = T.init_transform_dict_simple(input_res=RES, antialias=True)["train"]
    val = T.init_transform_dict(video_res=(240, 320), input_res=RES)["val"]
    g = torch.Generator().manual_seed(7)
    out = torch.empty((B * FRAMES, 3) + RES, dtype=torch.float32, device="cuda")
    mean, std = (C.c_float * 3)(*simple.mean), (C.c_float * 3)(*simple.std)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outp = C.c_void_p(out.data_ptr())
    batches, tables, spaces = {}, {}, {}
    for hw in SOURCES:
        v = batches[hw] = [torch.randint(0, 256, (FRAMES, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
        vg = [val.geometry(*hw) for _ in v]
        tables[hw] = {"simple": H.frame_table(v, [simple.geometry(*hw)[0]] * B),
                      "simple+aa": H.frame_transform_table(v, [simple.geometry(*hw)[0]] * B),
                      "val": H.frame_transform_table(v, [x[0] for x in vg], two_stage=[x[1] for x in vg])}
        tables[hw]["val+aa"] = tables[hw]["val"]
        for p in ("simple+aa", "val+aa"):
            n = lib.xp_frames_transform_aa_workspace_bytes(tables[hw][p], B, RES[0], RES[1])
            spaces[hw, p] = (torch.empty(n, dtype=torch.uint8, device="cuda"), n)

    def launch(path, hw):
        if path == "simple":
            rc = lib.xp_frames_resize_norm(tables[hw][path], B, mean, std, outp, RES[0], RES[1], stream)
        elif path == "val":
            rc = lib.xp_frames_transform(tables[hw][path], B, mean, std, outp, RES[0], RES[1], stream)
        else:
            ws, n = spaces[hw, path]
            rc = lib.xp_frames_transform_aa(tables[hw][path], B, mean, std, outp, RES[0], RES[1], C.c_void_p(ws.data_ptr()), n, stream)
        if rc != 0:
            raise RuntimeError(f"{path}: {lib.xp_last_error().decode()}")

    paths = ["simple", "simple+aa", "val", "val+aa"]
    lines = [f"antialiased frame transforms, {B} videos x {FRAMES} frames -> fp32 [{B}, {FRAMES}, 3, {RES[0]}, {RES[1]}]; the C entry point "
             f"on a prebuilt table, {a.calls} back-to-back calls after {a.warmup} warm-up calls, device events, {a.rounds} interleaved "
             "rounds; alone on the GPU (nothing measured beside a running training step)"]
    t = {(p, hw): [] for p in paths + ["call+aa"] for hw in SOURCES}
    for r in range(a.rounds):
        for hw in SOURCES:
            for p in paths:
                t[p, hw].append(timed(lambda: launch(p, hw), a.warmup, a.calls))
            t["call+aa", hw].append(timed(lambda: simple_aa(batches[hw]), a.warmup, a.calls))
            lines.append(f"round {r} source {hw[0]} x {hw[1]}: " + " | ".join(f"{p} {t[p, hw][-1]:7.1f}" for p in paths + ["call+aa"]) + "  us")
    out_bytes = out.numel() * 4
    for hw in SOURCES:
        box = B * FRAMES * hw[0] * hw[1] * 3
        n = spaces[hw, "simple+aa"][1]
        lines.append(f"source {hw[0]} x {hw[1]}: box {box / 1e6:.1f} MB + output {out_bytes / 1e6:.1f} MB; tables {n} bytes (simple+aa), "
                     f"{spaces[hw, 'val+aa'][1]} bytes (val+aa)")
        for p in paths + ["call+aa"]:
            m = statistics.median(t[p, hw])
            ref = statistics.median(t["simple" if p.startswith(("simple", "call")) else "val", hw])
            lines.append(f"    {p:9s} median {m:7.1f} us (min {min(t[p, hw]):7.1f}, max {max(t[p, hw]):7.1f}) = {m / ref:6.2f} x its "
                         f"point-sampled launch; {(box + out_bytes) / m / 1e6:5.2f} TB/s of box + output bytes")
        for p in ("simple+aa", "val+aa"):
            try:
                k = kernel_times(lambda: launch(p, hw))
                lines.append(f"    {p:9s} kernels (profiler): table " + (f"{k['aa_table_kernel']:.1f}" if "aa_table_kernel" in k else "n/a") +
                             " us, resample " + (f"{k['aa_apply_kernel']:.1f}" if "aa_apply_kernel" in k else "n/a") + " us")
            except Exception as exc:          # the profiler is a convenience here: its absence must not lose the timings above
                lines.append(f"    {p:9s} kernels (profiler): n/a ({type(exc).__name__}: {exc})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
