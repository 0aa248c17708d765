#!/usr/bin/env python
"""Where the HOST time of a training step goes: cProfile over bench.py's step loop (no device sync inside the loop), and the
wall-clock host time inside EncoderLayerFn / PooledEncoderLayerFn forward and backward per step (the backward runs on autograd's
thread, which cProfile does not see: those four are timed by wrappers).  Run from the root of the tree to measure.
Usage (GPU box): python tools/host_profile.py [steps]"""
import cProfile
import io
import math
import pstats
import sys
import time

sys.path.insert(0, ".")
import torch  # noqa: E402

import bench  # noqa: E402
from xpretrain_amd import workload as O  # noqa: E402  (config + synthetic inputs)
from xpretrain_amd import distributed as D  # noqa: E402
from xpretrain_amd.modeling import VidCLIP  # noqa: E402
from xpretrain_amd.optimization import AdamW, NCELearnableTempLoss, build_e2e_optimizer_w_lr_mul, get_lr_sched  # noqa: E402

import xpretrain_amd.functional as XF  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
LAYER_HOST = {}      # "Class.method" -> [calls, seconds]


def _timed(cls, name):
    fn, acc = getattr(cls, name), LAYER_HOST.setdefault(f"{cls.__name__}.{name}", [0, 0.0])

    def wrapper(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            acc[0] += 1
            acc[1] += time.perf_counter() - t0
    setattr(cls, name, staticmethod(wrapper))


for _cls in (XF.EncoderLayerFn, XF.PooledEncoderLayerFn):
    _timed(_cls, "forward")
    _timed(_cls, "backward")
dev = torch.device("cuda", 0)
torch.manual_seed(1234)
model = VidCLIP(bench.Args(O.vit_b_config(16, 224))).to(dev).train()
loss_fn = NCELearnableTempLoss()
reducer = D.GradBucketReducer(model.parameters(), bucket_mb=64.0, average=True)
groups = build_e2e_optimizer_w_lr_mul(list(model.named_parameters()), 5e-6, 0.05, lr_mul=1, lr_mul_prefix="")
opt = AdamW([g for g in groups if g["params"]], lr=5e-6, betas=(0.9, 0.98))
video, ids, mask = (t.to(dev) for t in O.synthetic_inputs(8, 12, 224, 32))
ls = model.clipmodel.logit_scale


def step(i):
    with torch.no_grad():
        ls.clamp_(0, math.log(200.0))
    out = model(video, ids, mask)
    vis, txt = D.gather_features(out["vis_features"], out["text_features"])
    loss = loss_fn(vis, txt, ls)
    loss.backward()
    reducer.synchronize()
    lr = get_lr_sched(1000 + i, "cosine", 5e-6, 100000, warmup_ratio=0.01)
    for g in opt.param_groups:
        g["lr"] = lr
    opt.clip_and_step(5.0)
    reducer.zero_grad()


for i in range(3):
    step(i)
torch.cuda.synchronize()
for acc in LAYER_HOST.values():
    acc[0], acc[1] = 0, 0.0
pr = cProfile.Profile()
pr.enable()
for i in range(steps):
    step(i)
pr.disable()
torch.cuda.synchronize()
s = io.StringIO()
pstats.Stats(pr, stream=s).sort_stats("tottime").print_stats(28)
print(f"(totals over {steps} steps)")
for name, (calls, secs) in LAYER_HOST.items():
    print(f"layer host time  {name:32s} {calls / steps:6.1f} calls/step  {1e3 * secs / steps:8.3f} ms/step")
print(f"layer host time  {'all four':32s} {'':17s}  {1e3 * sum(s for _, s in LAYER_HOST.values()) / steps:8.3f} ms/step")
print("\n".join(line[:150] for line in s.getvalue().splitlines()[:60]))
