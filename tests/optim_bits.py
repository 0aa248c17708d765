"""The bits of the three optimizer updates on the ragged tensor set, pinned in ``tests/golden/optim_bits.json`` (a helper, not a test).

    python -m tests.optim_bits --record [--commit HASH] [--out PATH]      (on the MI355X, with the library built from the commit to pin)

``tests/test_optim_bits_gpu.py`` only reads the fixture.  What is pinned: the unguarded ``AdamW``, ``Adam`` and ``Adamax`` steps, with
clip ``None`` and ``0.5``, three steps each (gradient scales x1, x0.01, x1: the clip is active, idle, active), on the ragged set of
``tests/test_guarded_step_gpu.py`` (its ``SIZES`` and index constants; see its docstring for what each tensor is there for).  The guarded
kernels are tied to the same bits by ``test_finite_steps_have_the_unguarded_bits`` there.

The inputs come from integer arithmetic alone, so that no generator of any torch version is part of the fixture: one 32-bit LCG
(Numerical Recipes' 1664525 x + 1013904223, mod 2^32, jumped ahead in closed form), its top 24 bits as a signed integer times a power
of two.  The one float operation is the correctly rounded fp32 product with 0.01 for the second step's gradients.  The fixture holds a
digest of the inputs; the test fails when they differ.

Recorded per case, SHA-256 over the raw bytes after the third step: p, m and v of every named tensor (all but the 247 fillers), one
joint digest over p, m, v of the fillers in order, every shadow buffer, and the three gradient norms as fp32 bit patterns where the
step clipped."""
import argparse
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import torch

from tests import guarded_step_ref as G
from tests import test_guarded_step_gpu as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_bits.json")
CLIPS = T.CLIPS
SCALES = (1.0, 0.01, 1.0)
FILLER = range(12, T.I_LAST)                    # SIZES[12:-1]: the 247 tiny tensors that make the second launch table
assert len(FILLER) == 247 and T.I_TABLE2 in FILLER and all(T.SIZES[i] < 8 for i in FILLER)
NAMED = [i for i in range(len(T.SIZES)) if i not in FILLER]


def lcg(n, seed):
    """x_1 .. x_n of x_{k+1} = 1664525 x_k + 1013904223 (mod 2^32) from x_0 = seed: x_k = a^k x_0 + c (1 + a + .. + a^(k-1)), every
    product and sum wrapping in uint32"""
    a, c = np.uint32(1664525), np.uint32(1013904223)
    ak = np.cumprod(np.full(n, a, dtype=np.uint32), dtype=np.uint32)
    geo = np.cumsum(np.concatenate([np.ones(1, dtype=np.uint32), ak[:-1]]), dtype=np.uint32)
    return ak * np.uint32(seed) + c * geo


def values(n, seed, log2_scale):
    """n fp32 values on the grid 2^(log2_scale - 23) in [-2^log2_scale, 2^log2_scale): exact in fp32"""
    k = (lcg(n, seed) >> np.uint32(8)).astype(np.int32) - np.int32(1 << 23)
    return k.astype(np.float32) * np.float32(2.0 ** (log2_scale - 23))


@functools.lru_cache(maxsize=None)
def inputs():
    """(initial parameters, gradients of the three steps) as CPU tensors: |p| < 1/8, |g| < 1/16 times the step's scale"""
    init = [torch.from_numpy(values(n, 1000 + i, -3)) for i, n in enumerate(T.SIZES)]
    grads = [[torch.from_numpy(values(n, 100000 * (t + 1) + i, -4) * np.float32(SCALES[t])) for i, n in enumerate(T.SIZES)]
             for t in range(3)]
    return init, grads


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def inputs_digest():
    init, grads = inputs()
    return sha(*init, *(g for step in grads for g in step))


def ragged_set(kind):
    """``test_guarded_step_gpu.ragged_set(kind, False)`` on the inputs above"""
    from xpretrain_amd.functional import WEIGHTS
    init, _ = inputs()
    params = [torch.nn.Parameter(T.off_by_one(p.cuda()) if i == T.I_MIS_P else p.clone().cuda()) for i, p in enumerate(init)]
    WEIGHTS.get(params[T.I_BF_SMALL], T.BF), WEIGHTS.get(params[T.I_BF_CHUNK], T.BF)
    WEIGHTS.fused(tuple(params[i] for i in T.I_BIAS), torch.float32)
    half = len(params) // 2
    opt = T.ours(kind)([dict(params=params[:half], weight_decay=0.3, lr=1e-2), dict(params=params[half:], weight_decay=0.0, lr=3e-3)],
                       betas=T.BETAS)
    a, b = G.STATE[kind]
    p = params[T.I_MIS_S]
    opt.state[p] = {"step": 0, a: T.off_by_one(torch.zeros_like(p)), b: torch.zeros_like(p)}
    return T.Set(params, opt, lambda i, g: T.off_by_one(g) if i == T.I_MIS_G else g)


def run(kind, clip):
    """the digests of one case, in the fixture's layout"""
    s = ragged_set(kind)
    norms = []
    for step in inputs()[1]:
        s.step([g.cuda() for g in step], clip)
        if clip is not None:
            norms.append(s.opt.last_grad_norm.clone())
    T.finish(s)
    assert clip is None or float(norms[0]) > clip > float(norms[1]) and float(norms[2]) > clip, "the clip is not active, idle, active"
    assert len(s.opt._plan["launches"]) == 2 and s.opt._plan["n_chunks"] == T.N_CHUNKS and s.steps() == [3] * len(T.SIZES)
    sh = s.shadows_hold()
    assert [buf.dtype for buf, _ in sh] == [T.BF, T.BF, torch.float32]
    t = s.tensors()                                                        # p, m, v per parameter
    return {"tensors": {str(i): dict(zip("pmv", (sha(x) for x in t[3 * i:3 * i + 3]))) for i in NAMED},
            "fillers": sha(*(x for i in FILLER for x in t[3 * i:3 * i + 3])),
            "shadows": [sha(buf) for buf, _ in sh],
            "norms": [f"{n.cpu().view(torch.int32).item() & 0xFFFFFFFF:08x}" for n in norms]}


def case_name(kind, clip):
    return f"{kind} clip={clip}"


def differences(want, got):
    """what differs between two case records, one line per digest"""
    out = [f"tensor {i} (numel {T.SIZES[int(i)]}): {k} differs" for i, d in want["tensors"].items() for k in "pmv" if got["tensors"][i][k] != d[k]]
    if want["fillers"] != got["fillers"]:
        out.append("the 247 filler tensors (both launch tables): p, m or v differs")
    out += [f"shadow buffer {j}: differs" for j, (a, b) in enumerate(zip(want["shadows"], got["shadows"])) if a != b]
    out += [f"gradient norm of step {j}: recorded 0x{a}, got 0x{b}" for j, (a, b) in enumerate(zip(want["norms"], got["norms"])) if a != b]
    if len(want["shadows"]) != len(got["shadows"]) or len(want["norms"]) != len(got["norms"]):
        out.append("the number of shadow buffers or norms differs")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True, check=True).stdout
    doc = {"header": {"recorded_at_commit": commit, "hipcc": [l.strip() for l in hipcc.splitlines()[:2]],
                      "device": torch.cuda.get_device_name(0), "inputs_sha256": inputs_digest(),
                      "what": "tests/optim_bits.py: SHA-256 of the raw bytes after three unguarded steps on the ragged set"},
           "cases": {case_name(kind, clip): run(kind, clip) for kind in G.KINDS for clip in CLIPS}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}: {len(doc['cases'])} cases at {commit}")


if __name__ == "__main__":
    main()
