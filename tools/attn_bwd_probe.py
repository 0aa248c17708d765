#!/usr/bin/env python
"""The attention backward of one video-tower layer, isolated.  Default geometry: BASELINE cfg #2 (B=8, H=12, (M,N,L)=(4,12,196)), N
launches of the fused kernel and of the dQ / dKV pair (XPRETRAIN_DEBUG=attn_bwd_split) -- the workload of the rocprofv3 kernel-trace /
PMC passes of round 6 (tools/profile.sh, tools/pmc.sh):

    python tools/attn_bwd_probe.py [iters] [fused|split|both|wide] [colsum] [--geom M,N,L] [--batch B] [--heads H] [--rounds R]

`wide`: the dQ / dKV pair against the opt-in one-launch backward for wide windows (attn_bwd6_kernel, hip_ops.set_attn_bwd_wide) in one
process, interleaved round by round, median over the rounds -- e.g. configs[3] at the bench batch:
    python tools/attn_bwd_probe.py 50 wide colsum --geom 4,8,784"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from xpretrain_amd import hip_ops as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("iters", nargs="?", type=int, default=50)
ap.add_argument("which", nargs="?", default="both", choices=["fused", "split", "both", "wide"])
ap.add_argument("colsum", nargs="?", default=None)
ap.add_argument("--geom", default="4,12,196")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--heads", type=int, default=12)
ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()
iters, which, colsum = a.iters, a.which, a.colsum is not None
B, Hh = a.batch, a.heads
M, N, Lp = (int(v) for v in a.geom.split(","))
S = M + N * Lp
torch.manual_seed(0)
qkv = torch.randn(B * S, 3 * Hh * 64, device="cuda").to(torch.bfloat16)
out, stats = H.attn_fwd(qkv, B, S, Hh, size=(M, N, Lp))
dout = torch.randn_like(out)


def timed(n, warm):
    d = H.DeferredReduce(qkv.device) if colsum else None
    def once():
        r = H.attn_bwd(qkv, out, dout, stats, B, S, Hh, size=(M, N, Lp), q_scale=0.125, colsum_defer=d)
        if d is not None:
            d.segs.clear(); d._keep.clear(); d._names.clear()
        return r
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(n):
        once()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / n * 1e3


def run(tag):
    print(f"attn bwd {tag:5s} colsum={int(colsum)}: {timed(iters, 300):7.1f} us per call (all launches of the call)")


if which in ("fused", "both"):
    os.environ.pop("XPRETRAIN_DEBUG", None)
    run("fused")
if which in ("split", "both"):
    os.environ["XPRETRAIN_DEBUG"] = "attn_bwd_split"
    run("split")
if which == "wide":
    os.environ.pop("XPRETRAIN_DEBUG", None)
    prev = H.get_attn_bwd_wide()
    res = {"pair": [], "bwd6": []}
    try:
        for r in range(a.rounds + 1):                   # (round 0: warm-up of both, not counted)
            for tag, on in (("pair", False), ("bwd6", True)):
                H.set_attn_bwd_wide(on)
                kernel = H.attn_plan(B, S, Hh, size=(M, N, Lp), backward=True)["kernel"]
                assert kernel == ("bwd6" if on else "bwd_pair"), f"({M},{N},{Lp}) plans {kernel} with the switch {'on' if on else 'off'}"
                t = timed(iters, 100 if r == 0 else 10)
                if r:
                    res[tag].append(t)
    finally:
        H.set_attn_bwd_wide(prev)
    print(f"attn bwd (M,N,L)=({M},{N},{Lp}) B={B} H={Hh} colsum={int(colsum)}: {a.rounds} interleaved rounds of {iters} calls, us per call "
          "(all launches of the call)")
    for tag in res:
        v = res[tag]
        print(f"  {tag:5s} " + " ".join(f"{t:7.1f}" for t in v) + f"  || median {statistics.median(v):7.1f}  spread {max(v) - min(v):5.1f}")
