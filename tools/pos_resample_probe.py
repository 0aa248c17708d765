#!/usr/bin/env python
"""Time of the position-table resample (xp_pos_resample_fwd / _bwd) at BASELINE config #4's table: 14 x 14 -> 28 x 28 at D = 768,
i.e. [197, 768] -> [785, 768] fp32 forward and [785, 768] -> [197, 768] backward.

Per direction: device events around `calls` back-to-back calls of the C entry point on buffers built once, after `warmup` calls,
`rounds` rounds with the two directions interleaved.  The figure is what the launch takes back to back (kernel plus the host's
argument checks); a single launch inside a training step also pays its launch latency, which back-to-back calls hide.  Bytes: the
table once in, the result once out.  Alone on the GPU: the cost beside a running training step is NOT measured here.

    python tools/pos_resample_probe.py [--calls 2000] [--warmup 200] [--rounds 5] [--out FILE]
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

G0, GH, GW, D = 14, 28, 28, 768


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
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pos_resample_probe: needs an MI355X (a time taken anywhere else says nothing)")
    g = torch.Generator().manual_seed(7)
    pos = (0.02 * torch.randn(1 + G0 * G0, D, generator=g)).cuda()
    cot = torch.randn(1 + GH * GW, D, generator=g).cuda()
    out, d_pos = torch.empty_like(cot), torch.empty_like(pos)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def fwd():
        L.check(L.lib().xp_pos_resample_fwd(p(pos), p(out), G0, GH, GW, D, stream), "xp_pos_resample_fwd")

    def bwd():
        L.check(L.lib().xp_pos_resample_bwd(p(cot), p(d_pos), G0, GH, GW, D, stream), "xp_pos_resample_bwd")

    lines = [f"xp_pos_resample_fwd / _bwd, {G0} x {G0} -> {GH} x {GW}, D {D}; {a.calls} back-to-back calls after {a.warmup} warm-up calls, "
             f"device events, {a.rounds} interleaved rounds"]
    tf, tb = [], []
    for r in range(a.rounds):
        tf.append(timed(fwd, a.warmup, a.calls))
        tb.append(timed(bwd, a.warmup, a.calls))
        lines.append(f"round {r}: forward {tf[-1]:6.2f} us | backward {tb[-1]:6.2f} us")
    assert torch.equal(out, H.pos_resample_fwd(pos, GH, GW)) and torch.equal(d_pos, H.pos_resample_bwd(cot, G0, GH, GW))
    nbytes = (pos.numel() + cot.numel()) * 4
    for tag, t in (("forward", tf), ("backward", tb)):
        m = statistics.median(t)
        lines.append(f"{tag}: median {m:6.2f} us (spread {(max(t) - min(t)) / m * 100:.1f} %); {nbytes / 1e6:.2f} MB in + out = "
                     f"{nbytes / m / 1e6:.3f} TB/s end to end")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
