"""The bits of the loss family, the pair losses and the materialised retrieval-evaluation kernels, pinned in
``tests/golden/loss_bits.json`` (a helper, not a test).

    python -m tests.loss_bits --record [--commit HASH] [--out PATH]      (on the MI355X, with the library built from the commit to pin)

``tests/test_loss_bits_gpu.py`` only reads the fixture and applies no tolerance.  What is pinned, every case a few launches:

  * ``xp_contrastive_loss``, log_scale 4.6, all eight kinds at (n, d) = (1, 4) (no negatives: the merged form's exact zero), (8, 512)
    (small-logits form, two trips of its k loop), (70, 32) (small form past the 64-lane stride), (9, 30) (d % 4 != 0: the tiled form)
    and (130, 36) (n > 128: the tiled form over several tiles); ``vidimg`` and ``vidimg_divide`` also at (n, m, d) = (6, 4, 32) and
    (70, 9, 30).  Recorded: the loss, every gradient the kind has, d_log_scale.
  * ``xp_pair_loss``: every entry of ``pair_loss_ref.configs(n)`` (bag 3 and the order measure among them) at (n, d) = (1, 30),
    (5, 64), (70, 30).  The inputs keep ``pair_loss_ref.MIN_MARGIN`` from every switch of a selecting loss (checked on the CPU by
    ``check_pair_margins``; the recorder refuses inputs that do not), so a digest cannot hang on a comparison that rounding decides.
  * ``xp_sim_matrix`` at 33 x 70 x 30 (and 70 x 33, 33 x 33); ``xp_dsl_rerank`` in place on the 70 x 33 matrix, theta 100, ``multiply``
    0 and 1; ``xp_retrieval_ranks`` on the re-ranked matrix with explicit labels and on the 33 x 33 one with diagonal labels, both
    ``transpose`` values.

The inputs come from integer arithmetic alone (``tests.optim_bits.values``, the LCG): a row of 24-bit integers, its squared norm
summed exactly in int64, then one fp64 square root, one fp64 division and one rounding to fp32 per element -- no generator of any
torch version and no summation order is part of the fixture.  The fixture holds a digest of the inputs; the test fails when they
differ.

Recorded per output tensor: SHA-256 over its raw bytes; the loss and d_log_scale as fp32 bit patterns.

When the fixture was recorded the library still had one C entry each for ``nce`` and ``vsc_fc`` beside the family entry; the
recorder of that day ran both kinds through those as well, at every shape above, and refused to write unless their records
equalled the family entry's (``legacy_entries_equal_family`` in the header).  Those entries are gone; the family entry carries
their bits."""
import argparse
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import torch

from tests import loss_family_ref as R
from tests import pair_loss_ref as P
from tests.optim_bits import lcg, values

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_bits.json")
LOG_SCALE = 4.6
FAMILY_SHAPES = ((1, 4), (8, 512), (70, 32), (9, 30), (130, 36))
VIDIMG_SHAPES = ((6, 4, 32), (70, 9, 30))
# (n, d) -> seed of the pair-loss inputs: the first of 1, 2, 3, ... whose draw keeps MIN_MARGIN for every configuration
PAIR_SEEDS = {(1, 30): 1, (5, 64): 1, (70, 30): 1}
RETRIEVAL = (33, 70, 30)                        # rows of a, rows of b, d
FAMILY_OUTPUTS = ("loss", "d_vis", "d_txt", "d_img", "d_cap", "d_log_scale")


def unit_rows(rows, d, seed):
    """[rows, d] fp32, unit-norm rows: integers k of 24 bits, k / sqrt(sum k^2) in fp64 (the sum exact in int64), rounded to fp32"""
    k = values(rows * d, seed, 23).astype(np.int64).reshape(rows, d)
    norm = np.sqrt((k * k).sum(axis=1, keepdims=True).astype(np.float64))
    assert (norm > 0).all()
    return torch.from_numpy((k.astype(np.float64) / norm).astype(np.float32))


@functools.lru_cache(maxsize=None)
def family_feats(n, m, d):
    """[vis, txt [n, d], img, cap [m, d]] as CPU tensors"""
    return [unit_rows(r, d, 1000003 * (i + 1) + 7919 * n + 104729 * m + d) for i, r in enumerate((n, n, m, m))]


@functools.lru_cache(maxsize=None)
def pair_feats(n, d):
    """(vis [n, d], txt [n, d], the bag-3 txt [3n, d]) as CPU tensors"""
    s = 50000000 + 1000 * PAIR_SEEDS[(n, d)] + 100000 * n + d
    return unit_rows(n, d, s), unit_rows(n, d, s + 1), unit_rows(3 * n, d, s + 2)


@functools.lru_cache(maxsize=None)
def retrieval_inputs():
    """(a [33, 30], b [70, 30], labels of the 70 row queries in [0, 33), labels of the 33 column queries in [0, 70))"""
    na, nb, d = RETRIEVAL
    lab = lambda q, cnt, seed: torch.from_numpy(((lcg(q, seed) >> np.uint32(8)) % np.uint32(cnt)).astype(np.int64))
    return unit_rows(na, d, 90000001), unit_rows(nb, d, 90000002), lab(nb, na, 90000003), lab(na, nb, 90000004)


def family_cases():
    """(kind, n, m, d) of every family case"""
    out = [(kind, n, n, d) for kind in R.KINDS for n, d in FAMILY_SHAPES]
    return out + [(kind, *s) for kind in ("vidimg", "vidimg_divide") for s in VIDIMG_SHAPES]


def pair_cases():
    """(kind, params, n, d) of every pair-loss case"""
    return [(kind, params, n, d) for n, d in PAIR_SEEDS for kind, params in P.configs(n)]


def check_pair_margins():
    """every selecting configuration is at least MIN_MARGIN from its nearest switch, in fp64 on the CPU"""
    for kind, params, n, d in pair_cases():
        vis, txt, _ = pair_feats(n, d)
        margin = P.decision_margin(kind, params, [vis, txt])
        assert margin >= P.MIN_MARGIN, f"pair inputs at n={n} d={d}: {kind} {params} is {margin:.2e} from a switch (< {P.MIN_MARGIN})"


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def bits(t):
    return f"{t.detach().cpu().reshape(()).view(torch.int32).item() & 0xFFFFFFFF:08x}"


def inputs_digest():
    fam = [f for _, n, m, d in family_cases() for f in family_feats(n, m, d)]
    return sha(*fam, *(f for nd in PAIR_SEEDS for f in pair_feats(*nd)), *retrieval_inputs())


def family_name(kind, n, m, d):
    return f"family {kind} n={n} m={m} d={d}"


def pair_name(kind, params, n, d):
    return f"pair {kind} n={n} d={d} " + " ".join(f"{k}={v}" for k, v in sorted(params.items()))


def _record(names, outs):
    """scalars as bit patterns, tensors as digests, nothing for an output the kind does not have"""
    return {k: (bits(t) if t.dim() == 0 else sha(t)) for k, t in zip(names, outs) if t is not None}


def run_family(kind, n, m, d):
    from xpretrain_amd import hip_ops as H
    v, t, i, c = R.operands(kind, [f.cuda() for f in family_feats(n, m, d)])
    ls = torch.tensor(LOG_SCALE, dtype=torch.float32, device="cuda")
    return _record(FAMILY_OUTPUTS, H.contrastive_loss(R.KIND_IDS[kind], v, t, i, c, log_scale=ls))


def run_pair(kind, params, n, d):
    from xpretrain_amd import hip_ops as H
    vis, txt, txt3 = pair_feats(n, d)
    txt = txt3 if params.get("bag", 1) == 3 else txt
    return _record(("loss", "d_vis", "d_txt"), H.pair_loss(P.KIND_IDS[kind], vis.cuda(), txt.cuda(), **params))


def run_retrieval():
    """{case name: record} of the three materialised retrieval-evaluation kernels"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    lib = L.lib()
    a, b, lab_rows, lab_cols = (x.cuda() for x in retrieval_inputs())

    def sim(x, y):
        out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device="cuda")
        L.check(lib.xp_sim_matrix(H._p(x), H._p(y), H._p(out), x.shape[0], y.shape[0], x.shape[1], H._stream()), "xp_sim_matrix")
        return out

    def rerank(x, multiply):
        out = x.clone()
        L.check(lib.xp_dsl_rerank(H._p(out), out.shape[0], out.shape[1], 100.0, multiply, H._stream()), "xp_dsl_rerank")
        return out

    def ranks(x, labels, transpose):
        q = x.shape[1] if transpose else x.shape[0]
        g, e = (torch.empty(q, dtype=torch.int32, device="cuda") for _ in range(2))
        L.check(lib.xp_retrieval_ranks(H._p(x), None if labels is None else H._p(labels), x.shape[0], x.shape[1], transpose,
                                       H._p(g), H._p(e), H._stream()), "xp_retrieval_ranks")
        return {"greater": sha(g), "equal": sha(e)}

    wide, tall, square = sim(a, b), sim(b, a), sim(a, b[:a.shape[0]].contiguous())
    soft, ranked = rerank(tall, 0), rerank(tall, 1)
    return {"sim_matrix 33x70x30": {"sim": sha(wide)}, "sim_matrix 70x33x30": {"sim": sha(tall)},
            "sim_matrix 33x33x30": {"sim": sha(square)},
            "dsl_rerank 70x33 theta=100 multiply=0": {"sim": sha(soft)}, "dsl_rerank 70x33 theta=100 multiply=1": {"sim": sha(ranked)},
            "retrieval_ranks 70x33 labels transpose=0": ranks(ranked, lab_rows, 0),
            "retrieval_ranks 70x33 labels transpose=1": ranks(ranked, lab_cols, 1),
            "retrieval_ranks 33x33 diagonal transpose=0": ranks(square, None, 0),
            "retrieval_ranks 33x33 diagonal transpose=1": ranks(square, None, 1)}


RETRIEVAL_NAMES = ("sim_matrix 33x70x30", "sim_matrix 70x33x30", "sim_matrix 33x33x30", "dsl_rerank 70x33 theta=100 multiply=0",
                   "dsl_rerank 70x33 theta=100 multiply=1", "retrieval_ranks 70x33 labels transpose=0",
                   "retrieval_ranks 70x33 labels transpose=1", "retrieval_ranks 33x33 diagonal transpose=0",
                   "retrieval_ranks 33x33 diagonal transpose=1")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def check_inputs():
    assert inputs_digest() == recorded()["header"]["inputs_sha256"], \
        "the inputs differ from the ones the fixture was recorded on (tests/loss_bits.py): no digest can be compared"


def check(name, got):
    """the record `got` of case `name` is the recorded one, output for output"""
    check_inputs()
    want = recorded()["cases"][name]
    diff = [f"{k}: recorded {want.get(k)}, got {got.get(k)}" for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
    assert not diff, f"{name}: bits differ from the library at {recorded()['header']['recorded_at_commit'][:7]}:\n" + "\n".join(diff)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    check_pair_margins()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True, check=True).stdout
    cases ={family_name(*c): run_family(*c) for c in family_cases()}
    cases.update({pair_name(*c): run_pair(*c) for c in pair_cases()})
    cases.update(run_retrieval())
    doc = {"header": {"recorded_at_commit": commit, "hipcc": [l.strip() for l in hipcc.splitlines()[:2]],
                      "device": torch.cuda.get_device_name(0), "inputs_sha256": inputs_digest(),
                      "what": "tests/loss_bits.py: SHA-256 of the raw bytes of every output; loss and d_log_scale as fp32 bit patterns"},
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}: {len(cases)} cases at {commit}")


if __name__ == "__main__":
    main()
