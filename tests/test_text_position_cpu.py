"""CPU: custom ``position_ids`` of the text tower -- the restatement tests/text_position_ref.py against what the UNMODIFIED reference
computed (tests/golden/text_position_ids.pt, made by tests/golden/make_golden_position_ids.py), and the host-side refusals.

The embedding stage of the fixture is ``embeds`` (hidden_states[0] = tok[ids] + pos[position_ids]) forward and, backward, the two
table gradients as sums of the rows of ``d_embeds``.  The fp64 restatement is held to the reference's fp32 values with bounds that
come from the number format, not from a measurement: one fp32 rounding of the sum forward (2^-24 relative), the recursive-summation
bound (n - 1) 2^-24 sum |dx_i| per table row backward (text_position_ref.sum_bound).  The measured figures are printed.  The fp32
restatement -- one add; adds in row order -- is compared bit for bit forward; backward torch's own scatter order is not ours to
pin, so it is held to twice that bound (two fp32 sums of the same rows)."""
import ctypes as C

import pytest
import torch

from tests import text_position_ref as P
from tests.gpu_util import load_golden

CASES = ("offset", "reversed", "left_pad", "long")
VOCAB, N_POS, D = 120, 16, 128


@pytest.fixture(scope="module")
def fx():
    return load_golden("text_position_ids.pt")


def _weights():
    from oracle import clipvip_oracle as O
    from tests.golden import make_golden_position_ids as G
    from tests.gpu_util import seeded_model
    return seeded_model(O.hf_config_dict(**G.CONFIG), G.TEMPORAL_SIZE)


@pytest.fixture(scope="module")
def tables(fx):
    """the two embedding tables, rebuilt from the fixture's seeds and held to its fingerprint"""
    from tests.gpu_util import weight_fingerprint
    sd = _weights().state_dict()
    for k, (total, picks) in weight_fingerprint(sd).items():
        assert total == fx["fingerprint"][k][0] and torch.equal(picks, fx["fingerprint"][k][1]), k
    pre = "clipmodel.text_model.embeddings."
    return sd[pre + "token_embedding.weight"], sd[pre + "position_embedding.weight"]


def test_the_fixture_holds_the_four_cases(fx):
    assert tuple(fx["cases"]) == CASES
    shapes = {n: tuple(c["position_ids"].shape) for n, c in fx["cases"].items()}
    assert shapes == {"offset": (1, 12), "reversed": (12,), "left_pad": (4, 12), "long": (1, 24)}
    assert fx["cases"]["long"]["ids"].shape[1] > N_POS and int(fx["cases"]["long"]["position_ids"].max()) == N_POS - 1
    lp = fx["cases"]["left_pad"]
    assert bool((lp["mask"][:, 0] == 0).any()) and bool((lp["mask"][:, -1] == 1).all())
    assert len({tuple(r) for r in lp["position_ids"].tolist()}) > 1, "left_pad: the rows must differ"
    for c in fx["cases"].values():
        assert all(torch.isfinite(c[k]).all() for k in ("pooler_output", "last_hidden_state", "embeds", "d_tok", "d_pos"))


@pytest.mark.parametrize("name", CASES)
def test_forward_restatement_reproduces_the_reference_embeddings(fx, tables, name):
    c = fx["cases"][name]
    tok, pos = tables
    x32 = P.text_embed_pos(c["ids"], c["position_ids"], tok, pos)
    x64 = P.text_embed_pos64(c["ids"], c["position_ids"], tok, pos)
    dev = ((x64 - c["embeds"].double()).abs() / x64.abs().clamp_min(1e-300)).max().item()
    print(f"{name}: fp64 restatement vs the reference's fp32 embeds: max relative deviation {dev:.3e} (bound 2^-24 = {2.0 ** -24:.3e})")
    assert bool(((x64 - c["embeds"].double()).abs() <= 2.0 ** -24 * x64.abs()).all())
    assert torch.equal(x32, c["embeds"]), "one fp32 add has one result"


@pytest.mark.parametrize("name", CASES)
def test_backward_restatement_reproduces_the_reference_table_gradients(fx, name):
    c = fx["cases"][name]
    B, Lt = c["ids"].shape
    t64, p64 = P.text_embed_bwd_pos64(c["ids"], c["position_ids"], c["d_embeds"], VOCAB, N_POS)
    t32, p32 = P.text_embed_bwd_pos(c["ids"], c["position_ids"], c["d_embeds"], VOCAB, N_POS)
    keys = {"d_tok": (c["ids"].reshape(-1).tolist(), VOCAB), "d_pos": (P.position_rows(c["position_ids"], B, Lt).reshape(-1).tolist(), N_POS)}
    for label, r64, r32 in (("d_tok", t64, t32), ("d_pos", p64, p32)):
        bound = P.sum_bound(*keys[label], c["d_embeds"])
        e64, e32 = (r64 - c[label].double()).abs(), (r32.double() - c[label].double()).abs()
        print(f"{name} {label}: |fp64 restatement - reference fp32| max {e64.max().item():.3e}, largest bound {bound.max().item():.3e}; "
              f"|fp32 restatement - reference| max {e32.max().item():.3e}; {int((e32 == 0).all())} = bit-equal")
        assert bool((e64 <= bound).all()), label
        assert bool((e32 <= 2 * bound).all()), label
        absent = torch.tensor([k not in set(keys[label][0]) for k in range(keys[label][1])])
        assert bool((c[label][absent] == 0).all()) and bool((r32[absent] == 0).all())
    if name == "long":
        assert keys["d_pos"][0].count(N_POS - 1) == B * (Lt - N_POS + 1)        # the clamped tail lands on the last table row


def test_restatement_gives_a_nan_row_and_no_contribution_for_an_id_outside_the_table():
    inp = P.inputs(2, 5, 8, 7, 4, 2, torch.float32, seed=3)
    bad = inp["pos_ids"].clone()
    bad[1, 2] = 4
    x = P.text_embed_pos(inp["ids"], bad, inp["tok"], inp["pos"])
    good = P.text_embed_pos(inp["ids"], inp["pos_ids"], inp["tok"], inp["pos"])
    nan = torch.isnan(x)
    assert bool(nan[1, 2].all()) and int(nan.sum()) == 8 and torch.equal(x[~nan], good[~nan])
    zero = inp["dx"].clone()
    zero[1, 2] = 0                # a row of +0 under its valid id leaves the ordered sum of the other rows as it is
    t_bad, d_bad = P.text_embed_bwd_pos(inp["ids"], bad, inp["dx"], 7, 4)
    _, d_rest = P.text_embed_bwd_pos(inp["ids"], inp["pos_ids"], zero, 7, 4)
    t_good, d_good = P.text_embed_bwd_pos(inp["ids"], inp["pos_ids"], inp["dx"], 7, 4)
    assert torch.equal(d_bad, d_rest) and not torch.equal(d_bad, d_good) and torch.equal(t_bad, t_good)


# ------------------------------------------------------------------------------------------------------------------ host refusals
def _embeddings():
    return _weights().clipmodel.text_model.embeddings


@pytest.mark.parametrize("ids, why", [
    (torch.zeros(3, 12, dtype=torch.int64), "shape"),            # neither 1 nor B = 4 rows
    (torch.zeros(4, 11, dtype=torch.int64), "shape"),            # not Lt columns
    (torch.zeros(1, 4, 12, dtype=torch.int64), "shape"),
    (torch.zeros(12), "integer"),                                # a floating dtype
    ([[0.5] * 12], "integer"),
    (torch.arange(12) + 5, "outside the position table"),        # 16 is one past the table
    ([-1] + [0] * 11, "outside the position table"),
    (torch.full((4, 12), 16, dtype=torch.int32), "outside the position table"),
])
def test_host_refusals_of_cpu_position_ids(ids, why):
    emb = _embeddings()
    with pytest.raises(ValueError, match=why):
        emb(torch.zeros(4, 12, dtype=torch.int64), ids)


@pytest.mark.parametrize("ids", [torch.arange(12), torch.arange(12)[None].to(torch.int32), [list(range(12))] * 4,
                                 torch.arange(12, dtype=torch.uint8).expand(4, 12)])
def test_accepted_forms_become_int64_rows(ids):
    rows = _embeddings().position_rows(ids, 4, 12, torch.device("cpu"))
    assert rows.dtype == torch.int64 and rows.is_contiguous() and rows.shape in ((1, 12), (4, 12))
    assert torch.equal(rows[0], torch.arange(12))


def test_without_position_ids_a_sequence_longer_than_the_table_is_still_refused():
    emb = _embeddings()
    with pytest.raises(ValueError, match="max_position_embeddings"):
        emb(torch.zeros(2, 17, dtype=torch.int64))


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """pos_B outside {1, B}, D % 4, an empty table, a bad dtype, a null pointer: argument errors that name the entry.  The pointers
    are never followed -- a refused call launches nothing -- so this runs without a GPU."""
    from xpretrain_amd import _lib as L
    lib = L.lib()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    good = dict(pos_B=1, B=2, Lt=3, D=8, vocab=5, n_pos=4, dtype=L.XP_BF16)
    bad = [("pos_B", dict(pos_B=3)), ("pos_B", dict(pos_B=0)), ("D=", dict(D=6)), ("D=", dict(D=0)), ("n_pos", dict(n_pos=0)),
           ("dtype", dict(dtype=2)), ("null", dict(null=True))]
    for entry in ("xp_text_embed_fwd_pos", "xp_text_embed_bwd_pos"):
        for word, change in bad:
            a = dict(good, **change)
            last = None if a.pop("null", False) else p
            if entry.endswith("fwd_pos"):
                rc = lib.xp_text_embed_fwd_pos(p, p, a["pos_B"], p, p, last, a["B"], a["Lt"], a["D"], a["vocab"], a["n_pos"], a["dtype"], None)
            else:
                rc = lib.xp_text_embed_bwd_pos(p, p, a["pos_B"], p, p, last, a["B"], a["Lt"], a["D"], a["vocab"], a["n_pos"], a["dtype"], 0, None)
            msg = lib.xp_last_error().decode()
            assert rc == L.XP_ERR_ARG and entry in msg and word in msg, (entry, change, rc, msg)
    # pos_B == B is the other accepted value: the same call with pos_B = 2 = B is refused for nothing but the dtype we break
    assert lib.xp_text_embed_fwd_pos(p, p, 2, p, p, p, 2, 3, 8, 5, 4, 7, None) == L.XP_ERR_ARG and "dtype" in lib.xp_last_error().decode()
