#!/usr/bin/env python
"""Time of the retrieval evaluation and of top-k search, materialised against streamed (csrc/retrieval_stream.hip):

    1000 x 1000 x 512         MSR-VTT 1k-A: metrics.retrieval_metrics | retrieval_metrics_streamed | the count vectors of each alone
                              (no host summary) | topk k = 10, 100
    4096 x 16384 x 512        the same six
    8192 x 1048576 x 512      topk k = 10, 100 only (--big; the materialised path would need a 32 GiB matrix)

Per entry: device events around `calls` back-to-back calls on features built once (unit-norm rows around a common centre, the
paired rows pulled together: tests/retrieval_stream_ref.py::real_inputs drawn on the device), after `warmup` calls, `rounds` rounds
with the entries of a size interleaved in one process.  The evaluations include their device-to-host copies of the count vectors
and the host's summary -- what a caller of validate() waits for.  TFLOP/s: 2 nq ng d per score pass (the streamed evaluation makes
three: simple counts, DSL statistics, DSL counts; top-k one) against the 157.3 TFLOP/s fp32 peak.  Alone on the GPU: the cost beside
a running training step is NOT measured here.

    python tools/retrieval_stream_probe.py [--calls 3] [--warmup 1] [--rounds 5] [--big] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
from xpretrain_amd.utils import metrics  # noqa: E402

PEAK = 157.3


def features(nq, ng, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    c = torch.nn.functional.normalize(rn(1, d), dim=1)
    gal = c + 0.35 * rn(ng, d) / d ** 0.5
    q = c + 0.35 * rn(nq, d) / d ** 0.5
    n = min(nq, ng)
    q[:n] += 0.5 * (gal[:n] - c)
    return torch.nn.functional.normalize(q, dim=1).contiguous(), torch.nn.functional.normalize(gal, dim=1).contiguous()


def materialised(q, g, v2t_labels, summarise=metrics._summarise):
    """the body of metrics.retrieval_metrics, with labels for the direction that has more queries than candidates (which
    retrieval_metrics itself, diagonal only, refuses): the same three kernels over the [nq, ng] matrix"""
    sim = metrics.cal_cossim(q, g)
    out = {}
    for setting in ("simple", "DSL"):
        if setting == "DSL":
            sim = metrics.dsl_rerank(sim, 100.0)
        out[setting] = {"v2t": summarise(*metrics._rank_counts(sim, labels=v2t_labels, transpose=True)),
                        "t2v": summarise(*metrics._rank_counts(sim))}
    return out


def counts_only(*counts):
    return counts


def streamed_counts(q, g, v2t_labels):
    return [metrics.rank_counts_streamed(q, g, v2t_labels=v2t_labels, dsl_theta=th) for th in (None, 100.0)]


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
    return s.elapsed_time(e) / calls           # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big", action="store_true", help="the 8192 x 1048576 search as well")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_stream_probe: needs an MI355X (a time taken anywhere else says nothing)")
    lines = [f"retrieval evaluation and top-k, materialised (utils/metrics.py::retrieval_metrics) vs streamed; device events, {a.calls} "
             f"back-to-back calls after {a.warmup} warm-up call(s), {a.rounds} interleaved rounds; alone on the GPU"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    sizes = [(1000, 1000, 512, True, a.rounds, a.calls, a.warmup), (4096, 16384, 512, True, a.rounds, a.calls, a.warmup)]
    if a.big:
        sizes.append((8192, 1 << 20, 512, False, a.rounds, a.calls, a.warmup))      # a pass is 8.8 TFLOP, a 2 GiB gallery
    for nq, ng, d, both, rounds, calls, warmup in sizes:
        q, g = features(nq, ng, d)
        entries = {}
        v2t = None if ng <= nq else torch.arange(ng, device="cuda") % nq          # every video needs a labelled text
        if both:
            entries["retrieval_metrics (materialised)"] = (lambda: materialised(q, g, v2t), 1)
            entries["retrieval_metrics_streamed"] = (lambda: metrics.retrieval_metrics_streamed(q, g, v2t_labels=v2t), 3)
            # the same two without the host's summary of the count vectors (which both pay alike): kernels and copies
            entries["counts (materialised)"] = (lambda: materialised(q, g, v2t, counts_only), 1)
            entries["counts (streamed)"] = (lambda: streamed_counts(q, g, v2t), 3)
        entries["topk k=10"] = (lambda: metrics.topk(q, g, 10), 1)
        entries["topk k=100"] = (lambda: metrics.topk(q, g, 100), 1)
        times = {name: [] for name in entries}
        for r in range(rounds):
            for name, (f, _) in entries.items():
                times[name].append(timed(f, warmup, calls))
            emit(f"{nq} x {ng} x {d} round {r}: " + " | ".join(f"{name} {times[name][-1]:9.3f} ms" for name in entries))
        for name, (_, passes) in entries.items():
            t = times[name]
            m = statistics.median(t)
            tf = 2.0 * nq * ng * d * passes / (m * 1e-3) / 1e12
            emit(f"{nq} x {ng} x {d} {name}: median {m:9.3f} ms (min {min(t):.3f}, max {max(t):.3f}, spread {(max(t) - min(t)) / m * 100:.1f} %); "
                 f"{passes} score pass(es) = {tf:6.1f} TFLOP/s = {tf / PEAK * 100:4.1f} % of the {PEAK} TFLOP/s fp32 peak")
        if both:
            same = materialised(q, g, v2t), metrics.retrieval_metrics_streamed(q, g, v2t_labels=v2t)
            emit(f"{nq} x {ng} x {d} simple t2v: materialised {same[0]['simple']['t2v']} | streamed {same[1]['simple']['t2v']}")
            emit(f"{nq} x {ng} x {d} DSL    t2v: materialised {same[0]['DSL']['t2v']} | streamed {same[1]['DSL']['t2v']}")
        del q, g
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
