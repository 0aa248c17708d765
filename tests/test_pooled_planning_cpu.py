"""CPU: the host-only plan of the single-query proxy attention (xp_debug_attn_pooled_plan at a given CU count: nothing is
launched, no GPU needed) held to its rules, the pooled layer's workspace queries, and argument validation of the pooled entry
points (an XP_ERR_* return, never a launch)."""
import ctypes as C

import pytest

from xpretrain_amd import _lib as L

GEOMS = [(8, 12, 2356), (2, 12, 6276), (2, 12, 788), (8, 12, 200), (1, 2, 9), (3, 5, 201), (64, 16, 1028), (1, 1, 1), (1, 12, 100000)]
XP_ERR_ARG = -1


def _plan(B, H, S, dtype, backward, cus):
    info = L.XpAttnPooledPlanInfo()
    rc = L.lib().xp_debug_attn_pooled_plan(B, H, S, dtype, int(backward), cus, C.byref(info))
    assert rc == 0, L.lib().xp_last_error()
    return info


@pytest.mark.parametrize("cus", [256, 80, 64])
@pytest.mark.parametrize("dtype", [L.XP_BF16, L.XP_F32])
@pytest.mark.parametrize("B,H,S", GEOMS)
def test_pooled_attention_plan_rules(B, H, S, dtype, cus):
    lib = L.lib()
    total = lib.xp_attn_pooled_workspace_bytes(B, H, S, dtype)
    for backward in (False, True):
        p = _plan(B, H, S, dtype, backward, cus)
        assert p.chunks >= 1 and p.chunk_keys >= 1
        # chunk c covers [c*chunk_keys, min(S, (c+1)*chunk_keys)): together [0, S) exactly once, none of them empty
        bounds = [(c * p.chunk_keys, min(S, (c + 1) * p.chunk_keys)) for c in range(p.chunks)]
        assert bounds[0][0] == 0 and bounds[-1][1] == S
        assert all(a < b for a, b in bounds) and all(bounds[i][1] == bounds[i + 1][0] for i in range(p.chunks - 1))
        assert p.grid == B * H * p.chunks and p.combine_grid == B * H
        # no finer than 64 keys, whole workgroup steps (32 keys), at most 64 chunks; no more chunks than give every CU two workgroups
        assert p.chunk_keys % 32 == 0 and p.chunks <= 64 and (p.chunks == 1 or p.chunk_keys >= 64)
        assert p.chunks == 1 or B * H * (p.chunks - 1) < 2 * cus
        regions = [tuple(r) for r in (p.part_ml, p.part_acc, p.part_dq) if r[1] > 0]
        used = (p.part_dq,) if backward else (p.part_ml, p.part_acc)
        assert len(regions) == len(used)
        need = [B * H * p.chunks * 64 * 4] if backward else [B * H * p.chunks * 2 * 4, B * H * p.chunks * 64 * 4]
        for (off, nbytes), n in zip(used, need):
            assert off % 16 == 0 and nbytes >= n and off + nbytes <= p.workspace_bytes
        regions.sort()
        assert all(regions[i][0] + regions[i][1] <= regions[i + 1][0] for i in range(len(regions) - 1))
        assert 0 < p.workspace_bytes <= total
        assert p.colsum_rows == B * p.chunks <= lib.xp_attn_pooled_colsum_rows_max(B, S)


@pytest.mark.parametrize("B,H,S", GEOMS)
def test_pooled_attention_plan_fills_the_chip(B, H, S):
    """a smaller CU budget never cuts finer; where the keys allow it (>= 64 per chunk) every CU of the larger device gets work"""
    big, small = _plan(B, H, S, L.XP_BF16, False, 256), _plan(B, H, S, L.XP_BF16, False, 64)
    assert small.chunks <= big.chunks
    if B * H < 256 and S >= 64 * -(-256 // (B * H)):
        assert big.grid >= 256
    # both directions cut the keys the same way (the backward re-reads the forward's statistics per problem, not per chunk)
    assert _plan(B, H, S, L.XP_BF16, True, 256).chunks == big.chunks


def test_pooled_attention_rejects_bad_arguments():
    lib = L.lib()
    info = L.XpAttnPooledPlanInfo()
    for B, H, S in ((8, 12, 0), (8, 12, -5), (0, 12, 100), (8, 0, 100)):
        assert lib.xp_debug_attn_pooled_plan(B, H, S, L.XP_BF16, 0, 256, C.byref(info)) == XP_ERR_ARG
        assert lib.xp_attn_pooled_workspace_bytes(B, H, S, L.XP_BF16) == 0
    assert lib.xp_debug_attn_pooled_plan(8, 12, 100, 7, 0, 256, C.byref(info)) == XP_ERR_ARG
    assert lib.xp_debug_attn_pooled_plan(8, 12, 100, L.XP_BF16, 0, 256, None) == XP_ERR_ARG
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    # validation comes before any use of the device: these return without a GPU
    assert lib.xp_attn_pooled_fwd(None, p, 1536, p, p, 1, 12, 9, L.XP_BF16, p, 4096, None) == XP_ERR_ARG           # null q
    assert lib.xp_attn_pooled_fwd(p, p, 1536, p, p, 1, 12, 0, L.XP_BF16, p, 4096, None) == XP_ERR_ARG              # S == 0
    assert lib.xp_attn_pooled_fwd(p, p, 768, p, p, 1, 12, 9, L.XP_BF16, p, 4096, None) == XP_ERR_ARG               # ldkv < 2*H*64
    assert lib.xp_attn_pooled_fwd(p, p, 1540, p, p, 1, 12, 9, L.XP_BF16, p, 4096, None) == XP_ERR_ARG              # ldkv % 8
    assert lib.xp_attn_pooled_fwd(p, p, 1536, p, p, 1, 12, 9, 5, p, 4096, None) == XP_ERR_ARG                      # dtype
    assert lib.xp_attn_pooled_bwd(p, p, 1536, p, p, p, None, 768, p, 1536, 0.125, 1, 12, 9, L.XP_BF16, p, 4096, None, None) == XP_ERR_ARG
    assert lib.xp_attn_pooled_bwd(p, p, 1536, p, p, p, p, 64, p, 1536, 0.125, 1, 12, 9, L.XP_BF16, p, 4096, None, None) == XP_ERR_ARG
    assert b"" != lib.xp_last_error()


def _dims(B=2, S=9, D=128, Dff=512, heads=2, M=1, N=2, Lp=4, mode=L.ATTN_PROXY, dtype=L.XP_BF16):
    d = L.XpLayerDims()
    d.rows, d.D, d.Dff, d.B, d.S, d.heads, d.M, d.N, d.L = B * S, D, Dff, B, S, heads, M, N, Lp
    d.attn_mode, d.dtype, d.q_scale, d.ln_eps = mode, dtype, 0.125, 1e-5
    return d


def test_pooled_layer_entry_points_reject_bad_arguments():
    lib = L.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)

    def fwd(dims, null=None):
        a = L.XpLayerPooledFwd()
        a.dims = dims
        for name, typ in a._fields_:
            if typ is L.vp and name != null:
                setattr(a, name, p)
        a.workspace_bytes = 1 << 40
        return a

    def bwd(dims, null=None):
        a = L.XpLayerPooledBwd()
        a.dims = dims
        for name, typ in a._fields_:
            if typ is L.vp and name != null:
                setattr(a, name, p)
        a.workspace_bytes = 1 << 40
        return a

    bad = [_dims(D=192),                         # heads * 64 != D
           _dims(S=10),                          # S != M + N*L
           _dims(M=0, N=1, Lp=9),                # token 0 is not a proxy row
           _dims(mode=L.ATTN_CAUSAL),            # the text tower has no pooled form
           _dims(dtype=3), _dims(B=0)]
    for d in bad:
        assert lib.xp_encoder_layer_pooled_fwd(C.byref(fwd(d)), None) == XP_ERR_ARG
        assert lib.xp_encoder_layer_pooled_bwd(C.byref(bwd(d)), None) == XP_ERR_ARG
    for name in ("x", "Wqkv", "kv", "h1p", "q", "stats", "x3", "mean1p"):
        assert lib.xp_encoder_layer_pooled_fwd(C.byref(fwd(_dims(), null=name)), None) == XP_ERR_ARG, name
    for name in ("x", "kv", "q", "pre", "dx3", "dx", "rstd1p"):
        assert lib.xp_encoder_layer_pooled_bwd(C.byref(bwd(_dims(), null=name)), None) == XP_ERR_ARG, name
    assert lib.xp_encoder_layer_pooled_fwd(None, None) == XP_ERR_ARG and lib.xp_encoder_layer_pooled_bwd(None, None) == XP_ERR_ARG
    # side rows: side_in without side_out / outside bf16
    a = fwd(_dims(dtype=L.XP_F32))
    assert lib.xp_encoder_layer_pooled_fwd(C.byref(a), None) == XP_ERR_ARG
    # workspace too small
    a = fwd(_dims()); a.side_in = a.side_out = a.side_x2 = None; a.workspace_bytes = 16
    assert lib.xp_encoder_layer_pooled_fwd(C.byref(a), None) == XP_ERR_ARG
    a = bwd(_dims()); a.side_in = a.side_x2 = None; a.workspace_bytes = 16
    assert lib.xp_encoder_layer_pooled_bwd(C.byref(a), None) == XP_ERR_ARG


def test_pooled_layer_workspace_queries():
    """sizes are answered on the host; the pooled backward needs less scratch than the dense one at the bench shape (its
    activation-gradient temporaries are [B, .] but for dqkv and dh1)"""
    lib = L.lib()
    d = _dims(B=8, S=2356, D=768, Dff=3072, heads=12, M=4, N=12, Lp=196)
    f, b = lib.xp_encoder_layer_pooled_fwd_workspace_bytes(C.byref(d)), lib.xp_encoder_layer_pooled_bwd_workspace_bytes(C.byref(d))
    assert f >= lib.xp_attn_pooled_workspace_bytes(8, 12, 2356, L.XP_BF16) + 2 * 8 * 768 * 4
    assert 0 < b < lib.xp_encoder_layer_bwd_workspace_bytes(C.byref(d))
    assert b >= 8 * 2356 * 4 * 768 * 2 + lib.xp_attn_pooled_colsum_rows_max(8, 2356) * 2 * 768 * 4
    assert lib.xp_encoder_layer_pooled_fwd_workspace_bytes(None) == 0 and lib.xp_encoder_layer_pooled_bwd_workspace_bytes(None) == 0
