#!/usr/bin/env python
"""Time of DSL-weighted top-k search (csrc/retrieval_stream.hip: xp_retrieval_dsl_stats, xp_retrieval_topk_dsl):

    4096 x 16384 x 512        the statistics pass alone (per gallery row, per query) | topk plain / dsl_of="gallery" / dsl_of="queries"
                              at k = 10, 100 | the whole DSL search (statistics + top-k, both modes) against the materialised route,
                              dsl_rerank(cal_cossim(...)) followed by torch.topk (per-query mode: of the transposed problem)
    8192 x 1048576 x 512      the same without the materialised route (--big; its matrix would be 32 GiB)

Per entry: device events around `calls` back-to-back calls on features built once (tools/retrieval_stream_probe.py::features),
after `warmup` calls, `rounds` rounds with the entries of a size interleaved in one process.  TFLOP/s: 2 nq ng d per score pass (the
statistics one, top-k one, a search two) against the 157.3 TFLOP/s fp32 peak -- a whole call's rate, not a kernel's.  Ratios are
taken round by round (both entries of a ratio ran in the same round) and given as median (min .. max).  Alone on the GPU.

    python tools/retrieval_dsl_probe.py [--calls 3] [--warmup 1] [--rounds 5] [--big] [--out profiles/retrieval_dsl_probe.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
from xpretrain_amd.utils import metrics  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from retrieval_stream_probe import PEAK, features, timed  # noqa: E402

THETA = 100.0


def dsl_search(q, g, k, mode):
    st = metrics.dsl_stats(q, g, THETA) if mode == "gallery" else metrics.dsl_stats(g, q, THETA)
    return metrics.topk(q, g, k, dsl=st, dsl_of=mode, theta=THETA)


def materialised(q, g, k, mode):
    """the only route without this change: the [queries, gallery] matrix, re-ranked in place, then a sort"""
    if mode == "gallery":
        return torch.topk(metrics.dsl_rerank(metrics.cal_cossim(q, g), THETA), k, dim=1)
    return torch.topk(metrics.dsl_rerank(metrics.cal_cossim(g, q), THETA), k, dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big", action="store_true", help="8192 x 1048576 as well")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_dsl_probe: needs an MI355X (a time taken anywhere else says nothing)")
    lines = [f"DSL-weighted top-k search; device events, {a.calls} back-to-back calls after {a.warmup} warm-up call(s), {a.rounds} "
             f"interleaved rounds; alone on the GPU; theta = {THETA}"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    sizes = [(4096, 16384, 512, True)]
    if a.big:
        sizes.append((8192, 1 << 20, 512, False))                     # a pass is 8.8 TFLOP, a 2 GiB gallery
    for nq, ng, d, mat in sizes:
        q, g = features(nq, ng, d)
        st = {"gallery": metrics.dsl_stats(q, g, THETA), "queries": metrics.dsl_stats(g, q, THETA)}
        entries = {"stats gallery": (lambda: metrics.dsl_stats(q, g, THETA), 1), "stats queries": (lambda: metrics.dsl_stats(g, q, THETA), 1)}
        for k in (10, 100):
            entries[f"topk plain k={k}"] = (lambda k=k: metrics.topk(q, g, k), 1)
            for mode in ("gallery", "queries"):
                entries[f"topk {mode} k={k}"] = (lambda k=k, mode=mode: metrics.topk(q, g, k, dsl=st[mode], dsl_of=mode, theta=THETA), 1)
                entries[f"search {mode} k={k}"] = (lambda k=k, mode=mode: dsl_search(q, g, k, mode), 2)
                if mat:
                    entries[f"materialised {mode} k={k}"] = (lambda k=k, mode=mode: materialised(q, g, k, mode), 1)
        times = {name: [] for name in entries}
        for r in range(a.rounds):
            for name, (f, _) in entries.items():
                times[name].append(timed(f, a.warmup, a.calls))
            emit(f"{nq} x {ng} x {d} round {r}: " + " | ".join(f"{name} {times[name][-1]:.3f}" for name in entries) + " ms")
        for name, (_, passes) in entries.items():
            t = times[name]
            m = statistics.median(t)
            tf = 2.0 * nq * ng * d * passes / (m * 1e-3) / 1e12
            emit(f"{nq} x {ng} x {d} {name}: median {m:9.3f} ms (min {min(t):.3f}, max {max(t):.3f}, spread {(max(t) - min(t)) / m * 100:.1f} %); "
                 f"{passes} score pass(es) = {tf:6.1f} TFLOP/s = {tf / PEAK * 100:4.1f} % of the {PEAK} TFLOP/s fp32 peak")

        def ratio(what, num, den):
            """num / den round by round; den: one entry or the sum of several"""
            den = [den] if isinstance(den, str) else den
            r = [times[num][i] / sum(times[n][i] for n in den) for i in range(a.rounds)]
            emit(f"{nq} x {ng} x {d} {what}: {statistics.median(r):.3f} ({min(r):.3f} .. {max(r):.3f})")
        for k in (10, 100):
            for mode in ("gallery", "queries"):
                ratio(f"topk {mode} / topk plain, k={k}", f"topk {mode} k={k}", f"topk plain k={k}")
                ratio(f"search {mode} / (topk plain + stats {mode}), k={k}", f"search {mode} k={k}", [f"topk plain k={k}", f"stats {mode}"])
                if mat:
                    ratio(f"search {mode} / materialised {mode}, k={k}", f"search {mode} k={k}", f"materialised {mode} k={k}")
        if mat:                                                        # the two routes rank the same rows
            for mode in ("gallery", "queries"):
                ours, ref = dsl_search(q, g, 10, mode)[1], materialised(q, g, 10, mode)[1]
                ref = ref if mode == "gallery" else ref.t()
                emit(f"{nq} x {ng} x {d} {mode} k=10: {(ours == ref).float().mean().item() * 100:.3f} % of the list positions hold the "
                     f"materialised route's index (its statistics are summed in another order)")
        del q, g, st
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
