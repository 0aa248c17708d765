"""GPU: custom ``position_ids`` of the text tower -- xp_text_embed_fwd_pos / xp_text_embed_bwd_pos (csrc/text_embed_pos.hip) through
the C ABI with every output in a guard buffer, and the argument through the model.

Kernels: exact.  The forward is an index map and one fp32 add (bf16: one more rounding), the backward fp32 adds in row order, so a
result either has the bits of tests/text_position_ref.py or is wrong (torch.equal; a NaN matches a NaN).  Every case runs twice and
must give the same bits.  D = 4 (one lane), 512, 1028 (257 float4 columns: a second 256-thread column pass of the backward); both
output / gradient types; one shared map (pos_B = 1) and one per sample; store and accumulate.  The ballot rounds of the backward
(256 rows from the owner's row + 1 on) are crossed with one key on the rows at both sides of the boundaries; n_pos = 1 puts all 385
rows on one key.

Model: the four cases of tests/golden/text_position_ids.pt (the UNMODIFIED reference's fp32 results) under the gates
tests/test_model_gpu.py applies to the same kinds of quantity, fixed before the first run --
    float32 compute mode   outputs |d| <= TOL["fp32_abs"] = 1e-3 absolute; table gradients 5e-3 of the tensor scale
                           (test_fp32_compute_mode_against_oracle)
    bfloat16               outputs TOL["hidden_ref"] = 3.5e-2, table gradients TOL["grad_ref_2d"] = 7.5e-2 of the tensor scale
                           (hidden states / weight gradients against the reference's fp32 values)
Only the gathered position row differs from the default path, whose deviations those gates were set for.  Measured on the MI355X:
DESIGN.md 7."""
import pytest
import torch

from tests import embed_ref as R
from tests import text_position_ref as P
from tests.gpu_util import TOL, load_golden, report
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
CASES = ("offset", "reversed", "left_pad", "long")
_ids = str


def _H():
    from xpretrain_amd import hip_ops as H
    return H, H.L.lib()


def _dt(dtype):
    return {BF16: 0, F32: 1}[dtype]


def _ok(rc, lib):
    assert rc == 0, lib.xp_last_error()
    torch.cuda.synchronize()


def _filled(old):
    g = Guarded(old.shape[0], old.shape[1], old.dtype)
    g.mat.copy_(old.cuda())
    return g


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _fwd(inp, dtype, n_pos=None):
    H, lib = _H()
    B, Lt = inp["ids"].shape
    V, D = inp["tok"].shape
    n_pos = inp["pos"].shape[0] if n_pos is None else n_pos
    pos_ids = inp["pos_ids"].reshape(-1, Lt).contiguous()
    g = Guarded(B * Lt, D, dtype)
    dev = [t.cuda() for t in (inp["ids"], pos_ids, inp["tok"], inp["pos"])]
    _ok(lib.xp_text_embed_fwd_pos(H._p(dev[0]), H._p(dev[1]), pos_ids.shape[0], H._p(dev[2]), H._p(dev[3]), H._p(g.mat), B, Lt, D, V,
                                  n_pos, _dt(dtype), H._stream()), lib)
    g.check("text_embed_fwd_pos", B * Lt, D)
    return g.mat.view(B, Lt, D).cpu()


def _bwd(inp, accumulate):
    H, lib = _H()
    B, Lt = inp["ids"].shape
    V, D = inp["tok"].shape
    n_pos = inp["pos"].shape[0]
    pos_ids = inp["pos_ids"].reshape(-1, Lt).contiguous()
    gt = _filled(inp["old_tok"]) if accumulate else Guarded(V, D, F32)
    gp = _filled(inp["old_pos"]) if accumulate else Guarded(n_pos, D, F32)
    dev = [t.cuda() for t in (inp["ids"], pos_ids, inp["dx"])]
    _ok(lib.xp_text_embed_bwd_pos(H._p(dev[0]), H._p(dev[1]), pos_ids.shape[0], H._p(dev[2]), H._p(gt.mat), H._p(gp.mat), B, Lt, D, V,
                                  n_pos, _dt(inp["dx"].dtype), int(accumulate), H._stream()), lib)
    gt.check("text_embed_bwd_pos d_tok", V, D)
    gp.check("text_embed_bwd_pos d_pos", n_pos, D)
    return gt.mat.cpu(), gp.mat.cpu()


def _check_bwd(inp, accumulate):
    """both tables against the ordered fp32 sums, the untouched rows by their bits, and a second run"""
    V, n_pos = inp["tok"].shape[0], inp["pos"].shape[0]
    B, Lt = inp["ids"].shape
    d_tok, d_pos = _bwd(inp, accumulate)
    old = (inp["old_tok"], inp["old_pos"]) if accumulate else (None, None)
    rt, rp = P.text_embed_bwd_pos(inp["ids"], inp["pos_ids"], inp["dx"], V, n_pos, *old)
    named = set(p for p in P.position_rows(inp["pos_ids"], B, Lt).reshape(-1).tolist() if 0 <= p < n_pos)
    absent = torch.tensor([p not in named for p in range(n_pos)])
    if accumulate:
        assert R.same(d_pos[absent], inp["old_pos"][absent]), "accumulate: the rows no id names must keep their bits"
    else:
        assert bool((d_pos[absent].view(torch.int32) == 0).all()), "store: the rows no id names must be zero bits"
    assert torch.equal(d_pos, rp), f"d_pos: rows {sorted(set((d_pos != rp).nonzero()[:, 0].tolist()))} differ from the ordered fp32 sum"
    assert torch.equal(d_tok, rt), f"d_tok: rows {sorted(set((d_tok != rt).nonzero()[:, 0].tolist()))} differ from the ordered fp32 sum"
    t2, p2 = _bwd(inp, accumulate)
    assert R.same(t2, d_tok) and R.same(p2, d_pos), "second run differs"
    return d_tok, d_pos, absent


SIZES = [4, 512, 1028]
B0, LT0, V0, NPOS0 = 3, 7, 11, 5


@pytest.mark.parametrize("pos_B", [1, B0], ids=["shared", "per_sample"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("D", SIZES)
def test_forward_is_the_index_map_and_one_add(D, dtype, pos_B):
    inp = P.inputs(B0, LT0, D, V0, NPOS0, pos_B, dtype, seed=D + pos_B)
    got = _fwd(inp, dtype)
    assert R.same(got, R.store(P.text_embed_pos(inp["ids"], inp["pos_ids"], inp["tok"], inp["pos"]), dtype))
    assert R.same(_fwd(inp, dtype), got), "second run differs"


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("pos_B", [1, B0], ids=["shared", "per_sample"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
@pytest.mark.parametrize("D", SIZES)
def test_backward_is_the_ordered_sum(D, dtype, pos_B, accumulate):
    """the table has an unreferenced row (``hole``) between referenced ones: zero bits (store) or its old bits (accumulate)"""
    inp = P.inputs(B0, LT0, D, V0, NPOS0, pos_B, dtype, seed=D + pos_B, accumulate=bool(accumulate))
    _, _, absent = _check_bwd(inp, accumulate)
    assert bool(absent[inp["hole"]]) and not bool(absent[inp["hole"] - 1]) and not bool(absent[inp["hole"] + 1])


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_backward_across_the_ballot_rounds(dtype, accumulate):
    """5 x 77 = 385 rows.  Key 3 sits on rows 0, 255, 256 and 384: its owner (row 0) looks at rows 1..256 and 257..384 -- the last
    row of the first round, the first of the second, the last row of all.  Key 5 has its owner on row 1: rounds 2..257 and 258..384,
    with occurrences on 257 and 258.  Every other row draws from the other keys."""
    B, Lt, D, V, n_pos = 5, 77, 8, 13, 8
    inp = P.inputs(B, Lt, D, V, n_pos, B, dtype, seed=77, accumulate=bool(accumulate))
    g = R.gen(5)
    flat = torch.tensor([0, 1, 2, 6, 7])[torch.randint(0, 5, (B * Lt,), generator=g)]       # (n_pos // 2 = 4 stays the hole)
    flat[[0, 255, 256, 384]] = 3
    flat[[1, 257, 258]] = 5
    inp["pos_ids"] = flat.view(B, Lt)
    _check_bwd(inp, accumulate)


@pytest.mark.parametrize("pos_B", [1, 5], ids=["shared", "per_sample"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_a_table_of_one_row_takes_every_row(dtype, pos_B):
    B, Lt, D, V = 5, 77, 8, 13
    inp = P.inputs(B, Lt, D, V, 1, pos_B, dtype, seed=1)
    assert not bool(inp["pos_ids"].any())
    got = _fwd(inp, dtype)
    assert R.same(got, R.store(P.text_embed_pos(inp["ids"], inp["pos_ids"], inp["tok"], inp["pos"]), dtype))
    _, d_pos, _ = _check_bwd(inp, 0)
    assert d_pos.shape == (1, D)


@pytest.mark.parametrize("pos_B", [1, B0], ids=["shared", "per_sample"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_identity_ids_give_the_default_entries_bits(dtype, pos_B):
    """pos_ids[., t] = t against xp_text_embed_fwd / xp_text_embed_bwd (hip_ops wrappers): the same bits, forward and backward; the
    table is longer than the sequence, and its rows >= Lt are zero on both paths"""
    H, _ = _H()
    D, n_pos = 512, 9
    inp = P.inputs(B0, LT0, D, V0, n_pos, pos_B, dtype, seed=9)
    pos_ids = torch.arange(LT0).expand(pos_B, LT0).contiguous()
    ids, tok, pos, dx = (inp[k].cuda() for k in ("ids", "tok", "pos", "dx"))
    a = H.text_embed_fwd(ids, tok, pos, dtype)
    b = H.text_embed_fwd_pos(ids, pos_ids.cuda(), tok, pos, dtype)
    assert torch.equal(a, b)
    at, ap = H.text_embed_bwd(ids, dx.view(-1, D), V0, n_pos)
    bt, bp = H.text_embed_bwd_pos(ids, pos_ids.cuda(), dx.view(-1, D), V0, n_pos)
    assert torch.equal(at, bt) and torch.equal(ap, bp) and not bool(bp[LT0:].any()) and bool(bp[:LT0].any())


@pytest.mark.parametrize("bad", [NPOS0, -1, 1 << 40, -(1 << 62)])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ids)
def test_an_id_outside_the_table_is_a_nan_row_and_no_contribution(dtype, bad):
    """decided on the device: the row is NaN in every element, its neighbours are finite and have their bits, nothing outside the
    outputs is written (the guards), and the row adds to no row of d_pos"""
    D = 512
    inp = P.inputs(B0, LT0, D, V0, NPOS0, B0, dtype, seed=4)
    good = R.store(P.text_embed_pos(inp["ids"], inp["pos_ids"], inp["tok"], inp["pos"]), dtype)
    inp["pos_ids"] = inp["pos_ids"].clone()
    inp["pos_ids"][1, 3] = bad
    got = _fwd(inp, dtype)
    nan = torch.isnan(got)
    assert bool(nan[1, 3].all()) and int(nan.sum()) == D and bool(torch.isfinite(got[~nan]).all())
    assert R.same(got[~nan], good[~nan]) and R.same(_fwd(inp, dtype), got)
    for accumulate in (0, 1):
        case = dict(inp, **({"old_tok": R.randn(V0, D, seed=21), "old_pos": R.randn(NPOS0, D, seed=22)} if accumulate else {}))
        d_tok, d_pos, _ = _check_bwd(case, accumulate)
        assert bool(torch.isfinite(d_pos).all()) and bool(torch.isfinite(d_tok).all())


def test_refused_calls_write_nothing():
    """each refusal of the header, with real device buffers in guards: an argument error that names the entry, the outputs untouched"""
    H, lib = _H()
    inp = P.inputs(2, 3, 8, 5, 4, 1, BF16)
    ids, pos_ids, tok, pos, dx = (inp[k].cuda() for k in ("ids", "pos_ids", "tok", "pos", "dx"))
    good = dict(pos_B=1, D=8, n_pos=4, dtype=0)
    for change in (dict(pos_B=3), dict(D=6), dict(n_pos=0), dict(dtype=2)):
        a = dict(good, **change)
        gx, gt, gp = Guarded(6, 8, BF16), Guarded(5, 8, F32), Guarded(4, 8, F32)
        rc = lib.xp_text_embed_fwd_pos(H._p(ids), H._p(pos_ids), a["pos_B"], H._p(tok), H._p(pos), H._p(gx.mat), 2, 3, a["D"], 5,
                                       a["n_pos"], a["dtype"], H._stream())
        assert rc == -1 and b"xp_text_embed_fwd_pos" in lib.xp_last_error(), change
        rc = lib.xp_text_embed_bwd_pos(H._p(ids), H._p(pos_ids), a["pos_B"], H._p(dx), H._p(gt.mat), H._p(gp.mat), 2, 3, a["D"], 5,
                                       a["n_pos"], a["dtype"], 0, H._stream())
        assert rc == -1 and b"xp_text_embed_bwd_pos" in lib.xp_last_error(), change
        torch.cuda.synchronize()
        for g in (gx, gt, gp):
            g.check(f"refused {change}", 0, 0)


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def fx():
    return load_golden("text_position_ids.pt")


@pytest.fixture(scope="module")
def model(fx):
    """the fixture's model, rebuilt from its seeds (held to its fingerprint), on the GPU"""
    from oracle import clipvip_oracle as O
    from tests.golden import make_golden_position_ids as G
    from tests.gpu_util import seeded_model, weight_fingerprint
    m = seeded_model(O.hf_config_dict(**G.CONFIG), G.TEMPORAL_SIZE)
    for k, (total, picks) in weight_fingerprint(m.state_dict()).items():
        assert total == fx["fingerprint"][k][0] and torch.equal(picks, fx["fingerprint"][k][1]), k
    return m.cuda().train()


def _tables(model):
    emb = model.clipmodel.text_model.embeddings
    return emb.token_embedding.weight, emb.position_embedding.weight


def _tower(model, c, position_ids="fixture", **kw):
    """one text-tower call and the fixture's loss behind it: (pooler_output, last_hidden_state, d_tok, d_pos)"""
    clip = model.clipmodel
    for p in model.parameters():
        p.grad = None
    pos_ids = c["position_ids"] if isinstance(position_ids, str) else position_ids
    out = clip.text_model(input_ids=c["ids"].cuda(), attention_mask=None if c["mask"] is None else c["mask"].cuda(),
                          position_ids=pos_ids, **kw)
    pooled, last = out["pooler_output"], out["last_hidden_state"]
    ((pooled.float() * c["c_pool"].cuda()).sum() + (last.float() * c["c_last"].cuda()).sum()).backward()
    torch.cuda.synchronize()
    tok, pos = _tables(model)
    return pooled.detach().float().cpu(), last.detach().float().cpu(), tok.grad.clone().cpu(), pos.grad.clone().cpu(), out


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("name", CASES)
def test_model_against_the_reference_fixture(fx, model, name, dtype):
    c = fx["cases"][name]
    clip = model.clipmodel
    clip.set_compute_dtype(dtype)
    try:
        pooled, last, d_tok, d_pos, _ = _tower(model, c)
        with torch.no_grad():
            feats = clip.get_text_features(input_ids=c["ids"].cuda(), attention_mask=None if c["mask"] is None else c["mask"].cuda(),
                                           position_ids=c["position_ids"]).cpu()
    finally:
        clip.set_compute_dtype(BF16)
    tag = f"position_ids {name} {dtype}"
    if dtype == F32:
        dev = {k: (a - c[k]).abs().max().item() for k, a in (("pooler_output", pooled), ("last_hidden_state", last), ("text_features", feats))}
        grads = {k: report(f"{tag} {k}", a, c[k], 5e-3) for k, a in (("d_tok", d_tok), ("d_pos", d_pos))}
        print(f"{tag}: max |d| {dev}; gradients (of the tensor scale) {grads}")
        assert all(v <= TOL["fp32_abs"] for v in dev.values()), dev
        assert all(v <= 5e-3 for v in grads.values()), grads
    else:
        dev = {k: report(f"{tag} {k}", a, c[k], TOL["hidden_ref"])
               for k, a in (("pooler_output", pooled), ("last_hidden_state", last), ("text_features", feats))}
        grads = {k: report(f"{tag} {k}", a, c[k], TOL["grad_ref_2d"]) for k, a in (("d_tok", d_tok), ("d_pos", d_pos))}
        print(f"{tag}: of the tensor scale: {dev}; gradients {grads}")
        assert all(v <= TOL["hidden_ref"] for v in dev.values()), dev
        assert all(v <= TOL["grad_ref_2d"] for v in grads.values()), grads
    assert bool((d_pos[[p for p in range(16) if p not in set(P.position_rows(c["position_ids"], *c["ids"].shape).reshape(-1).tolist())]] == 0).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
def test_model_embedding_stage_is_the_restatement(fx, model, dtype):
    """hidden_states[0] of the long case (24 tokens over a table of 16) has the restatement's bits; with output_hidden_states and
    output_attentions the other outputs keep theirs"""
    c = fx["cases"]["long"]
    clip = model.clipmodel
    clip.set_compute_dtype(dtype)
    try:
        p0, l0, t0, q0, _ = _tower(model, c)
        p1, l1, t1, q1, out = _tower(model, c, output_hidden_states=True, output_attentions=True)
    finally:
        clip.set_compute_dtype(BF16)
    tok, pos = (w.detach().cpu() for w in _tables(model))
    want = R.store(P.text_embed_pos(c["ids"], c["position_ids"], tok, pos), dtype)
    assert R.same(out["hidden_states"][0].detach().cpu(), want)
    if out["hidden_side_rows"] is not None:         # bf16: the fp32 residual stream beside the bf16 rows starts from the same map
        assert torch.equal(out["hidden_side_rows"][0].cpu(), P.text_embed_pos(c["ids"], c["position_ids"], tok, pos))
    assert len(out["attentions"]) == 2 and out["attentions"][0].shape == (4, 2, 24, 24)
    assert torch.equal(p0, p1) and torch.equal(l0, l1) and torch.equal(t0, t1) and torch.equal(q0, q1)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("form", ["list", "cpu_1d", "gpu_int32_rows"])
def test_identity_ids_through_the_model_equal_the_default_path(fx, model, dtype, form):
    """arange(Lt) in every accepted form goes through the new entries and gives the default path's bits, forward and backward; and
    the default path before and after it is bit-equal to itself (no state leaks)"""
    c = fx["cases"]["left_pad"]
    ids = {"list": list(range(12)), "cpu_1d": torch.arange(12),
           "gpu_int32_rows": torch.arange(12, dtype=torch.int32).expand(4, 12).cuda()}[form]
    clip = model.clipmodel
    clip.set_compute_dtype(dtype)
    try:
        before = _tower(model, c, position_ids=None)[:4]
        custom = _tower(model, c, position_ids=ids)[:4]
        shifted = _tower(model, c)[:4]
        after = _tower(model, c, position_ids=None)[:4]
    finally:
        clip.set_compute_dtype(BF16)
    for a, b, d in zip(before, custom, after):
        assert torch.equal(a, b) and torch.equal(a, d)
    assert not torch.equal(shifted[0], before[0])


def test_gradient_checkpointing_gives_the_same_bits(fx, model):
    c = fx["cases"]["left_pad"]
    clip = model.clipmodel
    plain = _tower(model, c)[:4]
    clip.gradient_checkpointing_enable()
    try:
        assert clip.text_model.encoder.gradient_checkpointing and model.training
        ckpt = _tower(model, c)[:4]
    finally:
        clip.gradient_checkpointing_disable()
    assert all(torch.equal(a, b) for a, b in zip(plain, ckpt))


@pytest.mark.parametrize("overlap", [True, False], ids=["side_stream", "plain"])
def test_clipmodel_forward_passes_position_ids_to_the_text_tower(fx, model, overlap, monkeypatch):
    """CLIPModel.forward(position_ids=...), on the text tower's side stream and on the caller's: text_embeds are get_text_features'"""
    from oracle import clipvip_oracle as O
    c = fx["cases"]["offset"]
    clip = model.clipmodel
    monkeypatch.setattr(type(clip), "overlap_text_tower", overlap)
    video, _, _ = O.synthetic_inputs(4, 3, 32, 12, vocab=120)
    ids, mask, pos_ids = c["ids"].cuda(), c["mask"].cuda(), c["position_ids"].cuda()
    with torch.no_grad():
        out = clip(input_ids=ids, pixel_values=video.cuda(), attention_mask=mask, position_ids=pos_ids)
        want = clip.get_text_features(input_ids=ids, attention_mask=mask, position_ids=pos_ids, if_norm=True)
        default = clip(input_ids=ids, pixel_values=video.cuda(), attention_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(out.text_embeds, want) and not torch.equal(out.text_embeds, default.text_embeds)
    assert torch.equal(out.image_embeds, default.image_embeds)


def test_gpu_ids_are_not_read_on_the_host_and_a_bad_one_is_a_nan_row(fx, model):
    """a CPU tensor with an id outside the table is refused on the host; the same ids on the GPU run, and the kernel's rule shows:
    exactly that token's embedding is NaN.  Behind the tower the token's own output is NaN (not swallowed) and every other sample
    is finite (not leaked); inside the sample the attention kernels may spread it (a masked key's NaN value times a zero weight:
    measured on the MI355X, all 12 rows of the sample), which is theirs to say, not this entry's"""
    c = fx["cases"]["offset"]
    bad = torch.arange(12).repeat(4, 1)
    bad[2, 11] = 16
    with pytest.raises(ValueError, match="outside the position table"):
        model.clipmodel.text_model(input_ids=c["ids"].cuda(), position_ids=bad)
    with torch.no_grad():
        out = model.clipmodel.text_model(input_ids=c["ids"].cuda(), position_ids=bad.cuda(), output_hidden_states=True)
    nan = torch.isnan(out["hidden_states"][0].float()).cpu()
    assert bool(nan[2, 11].all()) and int(nan.sum()) == 128
    last = torch.isnan(out["last_hidden_state"].float()).cpu()
    assert bool(last[2, 11].all()) and not bool(last[[0, 1, 3]].any())
