#!/usr/bin/env python
"""Forward-only cost of the pooled last layer: VidCLIP.forward_video (retrieval feature extraction) under torch.no_grad() at the
bench shape, dense and pooled (CLIPModel.pooled_last_layer) in ONE process, interleaved, timed with HIP events.

    python tools/pooled_forward_video.py [--iters 30] [--warmup 5] [--batch 8] [--frames 12] [--res 224]

Prints the median ms per call of either setting and the largest feature difference between them."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench as B  # noqa: E402
from xpretrain_amd import workload as O  # noqa: E402
from xpretrain_amd.modeling import VidCLIP  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--res", type=int, default=224)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model = VidCLIP(B.Args(O.vit_b_config(16, a.res))).to(dev).eval()
    video = O.synthetic_inputs(a.batch, a.frames, a.res, 32, seed=4321)[0].to(dev)
    times = {False: [], True: []}
    feats = {}
    with torch.no_grad():
        for it in range(a.warmup + a.iters):
            for pooled in (False, True):
                model.clipmodel.pooled_last_layer = pooled
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                feats[pooled] = model.forward_video(video)
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[pooled].append(e0.elapsed_time(e1))
    d = (feats[True] - feats[False]).abs().max().item()
    md, mp = statistics.median(times[False]), statistics.median(times[True])
    print(f"VidCLIP.forward_video, torch.no_grad, batch {a.batch} x {a.frames} frames of {a.res}^2, HIP events, interleaved, "
          f"median of {a.iters} after {a.warmup} warm-up calls:")
    print(f"  dense  {md:.3f} ms (min {min(times[False]):.3f})")
    print(f"  pooled {mp:.3f} ms (min {min(times[True]):.3f})   {100 * (md - mp) / md:+.2f} % ; max |d feature| = {d:.2e}")


if __name__ == "__main__":
    main()
