"""GPU: the four fixed-temperature losses behind xp_pair_loss -- TripletContrastiveLoss, NCEContrastiveLoss, HardNegLoss,
MILNCEContrastiveLoss -- against the reference's fixtures (tests/golden/pair_losses.pt), against fp64 autograd of
tests/pair_loss_ref.py, for determinism, exact workspaces, refusals, and through VidCLIP's backward.

Three of the losses select (top-k, hardest negative, hinge): every input of a gradient comparison is first asserted to keep
pair_loss_ref.MIN_MARGIN from every switch (pair_loss_ref.decision_margin), so an fp32 rounding cannot change a selection."""
import ctypes as C
import functools

import pytest
import torch

from tests import pair_loss_ref as R
from tests.gpu_util import ModelArgs, report
from tests.guarded import GuardedWorkspaces

pytestmark = pytest.mark.gpu

# (n, d, seed): more than two waves, more than four 32-tiles, past the 128-row small-logits form; d % 4 != 0 (tiled logits)
BIG, ODD_D = (130, 96, 1529), (9, 30, 1039)
LOSS_ONLY = (300, 64, 1364)
KINDS = list(R.KINDS)


def _module(kind, p):
    from xpretrain_amd.optimization import build_loss_func
    return build_loss_func(dict(loss_name=R.KINDS[kind], margin=p["margin"], measure="order" if p["order_measure"] else "cosine",
                                max_violation=bool(p["max_violation"]), temp=p["temp"], hard_negative_num=p["hard_negative_num"]))


def _key(p):
    return tuple(sorted(dict(R.DEFAULTS, **p).items()))


@functools.lru_cache(maxsize=None)
def _fp64(kind, n, d, seed, key, grads=True):
    """(fp32-rounded features, decision margin, fp64 loss, fp64 grads | None) on the CPU: computed once, shared, never modified"""
    p = dict(key)
    feats = [f.float() for f in R.unit_feats(n, d, seed, bag=p["bag"])]
    if not grads:
        return feats, None, R.loss(kind, *[f.double() for f in feats], **p), None
    return (feats, R.decision_margin(kind, p, feats), *R.loss_and_grads(kind, feats, **p))


def _run(kind, feats, p):
    from xpretrain_amd import hip_ops as H
    q = dict(R.DEFAULTS, **p)
    return H.pair_loss(R.KIND_IDS[kind], feats[0].cuda(), feats[1].cuda(), **q)


def _raw(kind, prm, vis, txt, loss, dv, dt, ws, n=None, ws_bytes=None):
    """xp_pair_loss itself on the caller's buffers (None: a null pointer); returns (rc, message)"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    ptr = [C.c_void_p(0 if t is None else t.data_ptr()) for t in (vis, txt, loss, dv, dt, ws)]
    rc = L.lib().xp_pair_loss(kind, None if prm is None else C.byref(prm), *ptr[:5], vis.shape[0] if n is None else n, vis.shape[1],
                              ptr[5], (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, H._stream())
    return rc, L.lib().xp_last_error().decode()


def _params(p):
    from xpretrain_amd import _lib as L
    q = dict(R.DEFAULTS, **p)
    return L.XpPairLossParams(q["temp"], q["margin"], q["max_violation"], q["order_measure"], q["hard_negative_num"], q["bag"])


@pytest.mark.parametrize("kind", KINDS)
def test_pair_losses_against_reference_fixtures(golden, kind):
    """1. every case of pair_losses.pt through the module surface and autograd, incoming scalar 2.0; the bounds of
    test_family_against_reference_fixtures: loss within 1e-3 of max(1, |ref|), gradients within 1e-3 relative to
    max(max|ref|, R.grad_scale_floor)."""
    cases = [c for c in golden("pair_losses.pt") if R.KIND_NAMES[c["kind"]] == kind]
    assert len(cases) == {"triplet": 24, "nce": 12, "hardneg": 18, "milnce": 12}[kind]
    for c in cases:
        p = c["params"]
        assert R.decision_margin(kind, p, c["feats"]) >= R.MIN_MARGIN
        feats = [f.cuda().requires_grad_() for f in c["feats"]]
        loss = _module(kind, p)(*feats)
        grads = torch.autograd.grad(loss * 2.0, feats)
        ref = c["loss"].item()
        tag = f"{kind} n={c['n']} d={c['d']} " + " ".join(f"{k}={v}" for k, v in p.items() if v != R.DEFAULTS[k])
        print(f"{tag}: loss {loss.item():.6f} ref {ref:.6f}")
        assert abs(loss.item() - ref) <= 1e-3 * max(1.0, abs(ref)), tag
        floor = R.grad_scale_floor(R.grad_scale(kind, p))
        for name, g, r in zip(("dV", "dT"), grads, c["grads"]):
            assert g.shape == r.shape and torch.isfinite(g).all()
            assert report(f"{tag} {name}", g / 2.0, r, 1e-3, scale_floor=floor) <= 1e-3


@pytest.mark.parametrize("shape,kind,key", [(s, k, _key(p)) for s in (BIG, ODD_D) for k, p in R.configs(s[0])])
def test_pair_losses_against_fp64(shape, kind, key):
    """2. every kind and configuration against fp64 autograd of the helper on the same fp32-rounded features: loss within 1e-4
    relative, gradients within 1e-4 (the bounds of test_family_against_fp64)"""
    p = dict(key)
    feats, margin, rl, rg = _fp64(kind, *shape, key)
    assert margin >= R.MIN_MARGIN, margin
    out = _run(kind, feats, p)
    tag = f"{kind} fp64 n={shape[0]} d={shape[1]} " + " ".join(f"{k}={v}" for k, v in p.items() if v != R.DEFAULTS[k])
    print(f"{tag}: loss {out[0].item():.7f} fp64 {rl.item():.7f} margin {margin:.3e}")
    assert abs(out[0].item() - rl.item()) <= 1e-4 * abs(rl.item()), tag
    floor = R.grad_scale_floor(R.grad_scale(kind, p))
    for name, g, r in zip(("dV", "dT"), out[1:], rg):
        assert g.shape == r.shape
        assert report(f"{tag} {name}", g, r, 1e-4, scale_floor=floor) <= 1e-4


@pytest.mark.parametrize("kind,p", [("hardneg", dict(hard_negative_num=40)), ("hardneg", dict(hard_negative_num=300)),
                                    ("triplet", dict(margin=0.2, max_violation=1)),
                                    ("triplet", dict(margin=0.2, max_violation=1, order_measure=1))])
def test_loss_value_at_300_rows(kind, p):
    """3. the loss alone at (300, 64) -- it is continuous in the features, so no margin is needed: within 1e-4 relative of fp64"""
    feats, _, rl, _ = _fp64(kind, *LOSS_ONLY, _key(p), grads=False)
    out = _run(kind, feats, p)
    print(f"{kind} {p}: loss {out[0].item():.7f} fp64 {rl.item():.7f}")
    assert abs(out[0].item() - rl.item()) <= 1e-4 * abs(rl.item())
    assert all(torch.isfinite(t).all() for t in out)


@pytest.mark.parametrize("kind", KINDS)
def test_pair_losses_are_deterministic_and_write_everything(kind):
    """4. two runs of every configuration on NaN-filled outputs: identical bits, every element finite afterwards"""
    from xpretrain_amd import _lib as L
    for n, d, seed in (BIG, (1, 32, 1033)):
        for k, p in R.configs(n):
            if k != kind:
                continue
            prm = _params(p)
            vis, txt = (f.float().cuda() for f in R.unit_feats(n, d, seed, bag=prm.bag))
            ws = torch.empty(L.lib().xp_pair_loss_workspace_bytes(R.KIND_IDS[k], C.byref(prm), n, d), dtype=torch.uint8, device="cuda")
            runs = []
            for _ in range(2):
                out = [torch.full(s, float("nan"), device="cuda") for s in ((), vis.shape, txt.shape)]
                ws.view(torch.int16).fill_(0x7FA5)
                rc, msg = _raw(R.KIND_IDS[k], prm, vis, txt, *out, ws)
                assert rc == 0, msg
                assert all(torch.isfinite(t).all() for t in out), (k, p, n)
                runs.append(out)
            assert all(torch.equal(a, b) for a, b in zip(*runs)), (k, p, n)
            if n == 1 and k == "triplet":
                assert all((t == 0).all() for t in runs[0])                      # no negative at all: zeros, written


@pytest.mark.parametrize("shape", [(70, 32, 1103), BIG])
@pytest.mark.parametrize("kind", KINDS)
def test_pair_losses_stay_inside_their_exact_workspace(kind, shape):
    """5. under GuardedWorkspaces (exact size, poisoned, guards on both sides): guards intact, bits equal to the ordinary run"""
    n, d, seed = shape
    for k, p in R.configs(n):
        if k != kind:
            continue
        feats = [f.float() for f in R.unit_feats(n, d, seed, bag=dict(R.DEFAULTS, **p)["bag"])]
        plain = _run(k, feats, p)
        torch.cuda.synchronize()
        with GuardedWorkspaces() as gw:
            guarded = _run(k, feats, p)
        gw.check()
        assert [(t, b) for t, b, _ in gw.records] == [("loss", 4 * (2 * n * feats[1].shape[0] + 2 * n + (n if k == "milnce" else 0)))]
        assert all(torch.equal(a, b) for a, b in zip(plain, guarded)), (k, p)


def test_refusals():
    """6. refused before any launch: the NaN-filled outputs are untouched and the message names the reason"""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    n, d = 6, 32
    vis, txt = (f.float().cuda() for f in R.unit_feats(n, d, 3))
    txt3 = R.unit_feats(n, d, 3, bag=3)[1].float().cuda()
    out = [torch.full(s, float("nan"), device="cuda") for s in ((), vis.shape, txt3.shape)]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    NCE, TRI, HN, MIL = (R.KIND_IDS[k] for k in ("nce", "triplet", "hardneg", "milnce"))

    def refused(match, kind, p, *, v=vis, t=txt, o=out, w=ws, **kw):
        rc, msg = _raw(kind, None if p is None else _params(p), v, t, *o, w, **kw)
        assert rc == -1 and match in msg, (rc, msg)
        torch.cuda.synchronize()
        assert all(torch.isnan(x).all() for x in out)

    for kind in (4, -1, 1000):
        refused("unknown kind", kind, {})
    refused("null pointer", NCE, None)
    refused("null pointer", NCE, {}, o=[None, out[1], out[2]])
    refused("null pointer", TRI, {}, o=[out[0], None, out[2]])
    refused("null pointer", HN, {}, o=[out[0], out[1], None])
    refused("hard_negative_num", HN, dict(hard_negative_num=0))
    refused("hard_negative_num", HN, dict(hard_negative_num=n + 1))
    refused("temp", NCE, dict(temp=0.0))
    refused("temp", MIL, dict(temp=-1.0))
    refused("bag", NCE, dict(bag=3))
    refused("bag", MIL, dict(bag=0))
    refused("16384", NCE, {}, n=16385)
    refused("16384", MIL, dict(bag=3), t=txt3, n=5462)                           # 5462 * 3 = 16386
    refused("workspace too small", NCE, {}, w=None)
    need = L.lib().xp_pair_loss_workspace_bytes(MIL, C.byref(_params(dict(bag=3))), n, d)
    assert need == 4 * (2 * n * 3 * n + 3 * n)
    refused("workspace too small", MIL, dict(bag=3), t=txt3, ws_bytes=need - 1)
    for bad in (dict(kind=7, p={}), dict(kind=HN, p=dict(hard_negative_num=n + 1)), dict(kind=NCE, p=dict(temp=0.0))):
        assert L.lib().xp_pair_loss_workspace_bytes(bad["kind"], C.byref(_params(bad["p"])), n, d) == 0
    # the tensor wrapper: text rows against n * bag, and the library's refusals as RuntimeError
    with pytest.raises(ValueError, match=r"n \* bag = 6 \* 1 rows"):
        H.pair_loss(NCE, vis, txt3)
    with pytest.raises(ValueError, match=r"n \* bag = 6 \* 2 rows"):
        H.pair_loss(MIL, vis, txt3, bag=2)
    with pytest.raises(RuntimeError, match=r"xp_pair_loss\(hardneg\): hard_negative_num outside \[1, n\]"):
        H.pair_loss(HN, vis, txt, hard_negative_num=7)
    with pytest.raises(ValueError, match="no multiple"):
        _module("milnce", dict(R.DEFAULTS, temp=0.05))(vis[:4], txt)
    rc, msg = _raw(MIL, _params(dict(temp=0.05, bag=3)), vis, txt3, *out, ws)    # and the same buffers are accepted when all is well
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in out)


def _param_grads(model, loss):
    for p in model.parameters():
        p.grad = None
    loss.backward()
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_model_hand_off_hardneg_and_triplet():
    """7. the tiny seeded model of test_model_hand_off_vs_vc_fc_and_dsl (B = 4): VidCLIP.forward, the fused loss and backward
    against the same model with the loss restated in fp32 torch ops on the same features -- loss within 1e-3, every parameter
    gradient within that test's 8e-2 under report(), the same set of parameters with gradients."""
    from oracle import clipvip_oracle as O
    from xpretrain_amd.modeling import VidCLIP
    torch.manual_seed(11)
    cfgd = O.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64)
    model = VidCLIP(ModelArgs(cfgd, 4))
    with torch.no_grad():
        model.clipmodel.vision_model.embeddings.temporal_embedding.normal_(0, 0.1)
    B = 4
    video, ids, mask = O.synthetic_inputs(B, 4, 32, 8, vocab=120)
    model.cuda().train()
    for kind, params in (("hardneg", dict(hard_negative_num=2)), ("triplet", dict(margin=0.2, max_violation=1))):
        p = dict(R.DEFAULTS, **params)
        fn = _module(kind, p)
        got, want = {}, {}
        for store, fused in ((got, True), (want, False)):
            out = model(video.cuda(), ids.cuda(), mask.cuda())
            feats = [out["vis_features"], out["text_features"]]
            margin = R.decision_margin(kind, p, feats)
            assert margin >= R.MIN_MARGIN, (kind, margin)
            loss = fn(*feats) if fused else R.loss(kind, *feats, **p)
            store["loss"] = loss.item()
            store["grads"] = _param_grads(model, loss)
        print(f"hand-off {kind}: loss {got['loss']:.5f} torch ops {want['loss']:.5f} margin {margin:.3e}")
        assert abs(got["loss"] - want["loss"]) <= 1e-3 * max(1.0, abs(want["loss"]))
        assert set(got["grads"]) == set(want["grads"])
        worst = 0.0
        for name, ref in want["grads"].items():
            if ref.abs().max() > 1e-5:
                worst = max(worst, report(f"hand-off {kind} grad {name}", got["grads"][name], ref, 8e-2))
        assert worst <= 8e-2
