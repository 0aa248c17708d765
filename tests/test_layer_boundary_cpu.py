"""CPU: the boundary between functional.py and the four native layer calls (xp_encoder_layer_fwd / _bwd / _pooled_fwd / _pooled_bwd).
The argument structs are built from CPU tensors (building one launches nothing and takes no workspace): the plan's table of saved
pieces covers every pointer field, the two half-batch chains tile the full-batch buffers, the four workspace sizes are the ones
tests/golden/layer_workspace_bytes.json records, and every entry point refuses a workspace one byte short of its own query before
it touches a device.

The fixture was written by ``python tests/test_layer_boundary_cpu.py --record`` with the library built from the commit BEFORE the
workspaces were carved by one function per call (063f648): the sizes are part of the C ABI and must not move."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpretrain_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_workspace_bytes.json")
XP_ERR_ARG = -1
DTYPES = [torch.bfloat16, torch.float32]
B, S, SIZE, D, HEADS, DFF = 4, 10, (2, 2, 4), 128, 2, 512            # the tiny shape
# name: (B, S, D, Dff, heads, size | None)
SHAPES = {"tiny_video": (B, S, D, DFF, HEADS, SIZE), "tiny_text": (B, S, D, DFF, HEADS, None),
          "bench_video": (8, 2356, 768, 3072, 12, (4, 12, 196)), "video_448": (2, 6276, 768, 3072, 12, (4, 8, 784)),
          "text_32": (8, 32, 512, 2048, 8, None)}
QUERIES = ("xp_encoder_layer_fwd_workspace_bytes", "xp_encoder_layer_bwd_workspace_bytes",
           "xp_encoder_layer_pooled_fwd_workspace_bytes", "xp_encoder_layer_pooled_bwd_workspace_bytes")


def _dims(shape, dtype=L.XP_BF16, act=L.ACT_QUICK_GELU):
    b, s, d_, dff, heads, size = shape
    d = L.XpLayerDims()
    d.rows, d.D, d.Dff, d.B, d.S, d.heads = b * s, d_, dff, b, s, heads
    d.M, d.N, d.L = size if size else (0, 1, s)
    d.attn_mode = L.ATTN_PROXY if size else L.ATTN_CAUSAL
    d.dtype, d.q_scale, d.ln_eps, d.act = dtype, 0.125, 1e-5, act
    return d


def _sizes():
    """{"shape-dtype-act": [the four queries' answers; the pooled ones only for a video shape]}"""
    lib = L.lib()
    out = {}
    for name, shape in SHAPES.items():
        for dt, dn in ((L.XP_BF16, "bf16"), (L.XP_F32, "fp32")):
            for act, an in ((L.ACT_QUICK_GELU, "quick_gelu"), (L.ACT_GELU, "gelu")):
                d = _dims(shape, dt, act)
                out[f"{name}-{dn}-{an}"] = [int(getattr(lib, q)(C.byref(d))) for q in (QUERIES if shape[5] else QUERIES[:2])]
    return out


def test_workspace_sizes_equal_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _sizes()
    assert set(got) == set(want) and len(got) == 20
    assert all(v > 256 for vs in got.values() for v in vs)
    assert got == want


# ------------------------------------------------------------------------------------------------ the table covers the structs
def _pointer_fields(a):
    return [n for n, t in a._fields_ if t is L.vp]


def _layer_inputs(dtype, sided, size=SIZE, pooled=False):
    """CPU stand-ins for what a layer call is handed: (x, forward params, backward params, pad_mask, side, side_out, side_x2)"""
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    cd = lambda *shape: torch.zeros(shape, dtype=dtype)
    p = dict(ln1_w=f32(D), ln1_b=f32(D), Wqkv=cd(3 * D, D), bqkv=f32(3 * D), Wo=cd(D, D), bo=f32(D), ln2_w=f32(D), ln2_b=f32(D),
             W1=cd(DFF, D), b1=f32(DFF), W2=cd(D, DFF), b2=f32(D))
    import xpretrain_amd.functional as XF
    fwd, bwd = [p[n] for n in XF._FWD_PARAMS], [p[n] for n in XF._BWD_PARAMS]
    pad = None if size is not None else torch.ones(B, S, dtype=torch.int64)
    n_side, n_out = (B * size[0] if size is not None else B * S), (B if pooled else B * size[0] if size is not None else B * S)
    side, side_out, side_x2 = (f32(n_side, D), f32(n_out, D), f32(n_out, D)) if sided else (None, None, None)
    return cd(B * S, D), fwd, bwd, pad, side, side_out, side_x2


def _four_structs(kind, dtype, training=True):
    """the argument structs of a pass of one layer kind, built on the CPU: {entry point: (struct, plan, arena)}"""
    import xpretrain_amd.functional as XF
    sided = dtype == torch.bfloat16               # side rows exist only beside a bf16 stream
    size = None if kind == "text" else SIZE
    x, fwd, bwd, pad, side, side_out, side_x2 = _layer_inputs(dtype, sided, size, kind == "pooled")
    plan = (XF._pooled_plan if kind == "pooled" else XF._layer_plan)(B * S, D, DFF, B, S, HEADS, size, dtype)
    grads = {n: torch.zeros(k) for n, k in zip(plan.gnames, plan.gsizes)}
    if kind == "pooled":
        arena = torch.zeros(plan.arena_bytes, dtype=torch.uint8)
        x3, dx3 = torch.zeros(B, D, dtype=dtype), torch.zeros(B, D, dtype=dtype)
        out = {"xp_encoder_layer_pooled_fwd": XF._pooled_fwd_args(plan, x, fwd, arena, x3, training, side, side_out, side_x2)}
        if training:
            out["xp_encoder_layer_pooled_bwd"] = XF._pooled_bwd_args(plan, x, bwd, arena, dx3, side, side_x2, torch.zeros_like(x), grads)
    else:
        arena = torch.zeros(plan.arena_bytes, dtype=torch.uint8)
        if not training:
            side_x2 = None                        # (as _layer_fwd_native: the x2 side rows then live in the workspace)
        out = {"xp_encoder_layer_fwd": XF._layer_fwd_args(plan, plan.dims, x, fwd, pad, arena, torch.zeros_like(x), training, side,
                                                          side_out, side_x2)}
        if training:
            out["xp_encoder_layer_bwd"] = XF._layer_bwd_args(plan, x, bwd, arena, torch.zeros_like(x), pad, side, side_x2,
                                                             torch.zeros_like(x), grads)
    return {k: (a, plan, arena) for k, a in out.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["video", "text", "pooled"])
def test_the_table_covers_every_pointer_of_the_four_structs(kind, dtype):
    """A training pass (with side rows in bf16): every pointer field is set but ``pad_mask`` of a video layer, the side pointers of
    an fp32 pass -- and ``workspace``, which building a struct leaves alone (_call_native takes it at the launch).  A forward-only
    pass nulls exactly ``pre`` (and the dense forward's ``side_x2``).  The pieces sit 256-byte aligned, disjoint, inside the arena, and the
    typed views of the op-by-op path (_piece_views) are those pieces: same addresses as the struct fields, each exactly its piece."""
    import xpretrain_amd.functional as XF
    sides = {"side_in", "side_out", "side_x2"}
    for training in (True, False):
        structs = _four_structs(kind, dtype, training)
        assert len(structs) == (2 if training else 1)
        for entry, (a, plan, arena) in structs.items():
            null = {n for n in _pointer_fields(a) if not getattr(a, n)}
            want = {"workspace"} | ({"pad_mask"} & set(_pointer_fields(a)) if kind != "text" else set())
            if dtype != torch.bfloat16:
                want |= sides & set(_pointer_fields(a))
            if not training:
                want |= {"pre"} | ({"side_x2"} if kind != "pooled" else set())
            assert null == want, (entry, training, sorted(null ^ want))
            assert a.workspace_bytes == 0
            # the saved pieces: every one a field of this struct, in table order, aligned, disjoint, inside the arena
            end = 0
            for (name, n, bpr), (fname, off, fbpr) in zip(plan.pieces, plan.fill):
                assert name == fname and bpr == fbpr and name in _pointer_fields(a)
                assert off % 256 == 0 and off >= end
                if getattr(a, name):
                    assert getattr(a, name) == arena.data_ptr() + off
                end = off + n * bpr
            assert end <= plan.arena_bytes == arena.numel()
            # the typed views the op-by-op sequencers compute through: one per piece, at the address the struct field of the same
            # name holds, covering exactly its piece, in the dtype and shape the hip_ops wrappers expect
            views = XF._piece_views(plan, arena)
            assert list(views) == [n for n, _, _ in plan.pieces]
            for (name, n, bpr), (_, off, _) in zip(plan.pieces, plan.fill):
                v = views[name]
                f32 = name == "stats" or name[:4] in ("mean", "rstd")          # (fp32 statistics: flat, taken by element count)
                assert v.dtype == (torch.float32 if f32 else dtype) and v.is_contiguous(), name
                assert tuple(v.shape) == ((n * bpr // 4,) if f32 else (n, bpr // v.element_size())), name
                assert v.data_ptr() == arena.data_ptr() + off and v.numel() * v.element_size() == n * bpr, name
                if getattr(a, name):
                    assert v.data_ptr() == getattr(a, name), name
            # ... and nothing but the pieces points into the arena
            inside = {n for n in _pointer_fields(a) if arena.data_ptr() <= (getattr(a, n) or 0) < arena.data_ptr() + arena.numel()}
            assert inside == {n for n, _, _ in plan.pieces} - null


def test_the_two_forward_chains_tile_the_full_batch_buffers():
    """dense video layer, bf16 with side rows, two chains of 20 rows: for every saved piece, x, x3 and the side buffers, chain 0's
    region and chain 1's are adjacent and together the full-batch region"""
    import xpretrain_amd.functional as XF
    dtype = torch.bfloat16
    x, fwd, _, pad, side, side_out, side_x2 = _layer_inputs(dtype, True)
    x3 = torch.zeros_like(x)
    plan, hp = XF._layer_plan(B * S, D, DFF, B, S, HEADS, SIZE, dtype), XF._layer_plan(B * S // 2, D, DFF, B // 2, S, HEADS, SIZE, dtype)
    arena = torch.zeros(plan.arena_bytes, dtype=torch.uint8)
    r1 = B * S // 2
    assert r1 == 20 and r1 % 4 == 0
    full, c0, c1 = (XF._layer_fwd_args(plan, d, x, fwd, pad, arena, x3, True, side, side_out, side_x2, r0)
                    for d, r0 in ((plan.dims, 0), (hp.dims, 0), (hp.dims, r1)))
    assert (c0.dims.rows, c0.dims.B, c1.dims.rows, c1.dims.B) == (r1, B // 2, r1, B // 2)
    regions = [(n, rows // 2 * bpr, rows * bpr) for n, rows, bpr in plan.pieces]
    regions += [("x", r1 * D * 2, x.numel() * 2), ("x3", r1 * D * 2, x3.numel() * 2)]
    regions += [(n, B // 2 * SIZE[0] * D * 4, t.numel() * 4) for n, t in (("side_in", side), ("side_out", side_out), ("side_x2", side_x2))]
    assert len(regions) == 12 + 2 + 3
    for name, half, whole in regions:
        p, p0, p1 = getattr(full, name), getattr(c0, name), getattr(c1, name)
        assert p0 == p and p1 == p0 + half and 2 * half == whole, name
    assert (c1.side_S, c1.side_M) == (S, SIZE[0])


# ------------------------------------------------------------------------------------------------ a short workspace is refused
def _dummy_args(struct, dims, buf, sided):
    a = struct()
    a.dims = dims
    for n in _pointer_fields(a):
        setattr(a, n, C.addressof(buf))
    if not sided:
        for n in ("side_in", "side_out", "side_x2"):
            if hasattr(a, n):
                setattr(a, n, None)
    return a


@pytest.mark.parametrize("dt", [L.XP_BF16, L.XP_F32], ids=["bf16", "fp32"])
def test_a_workspace_one_byte_short_is_refused_before_any_launch(dt):
    """each entry point, all pointers dummy, ``workspace_bytes`` one less than its own query: the argument error that names the
    entry point (nothing touches a device: this runs without one).  fp32 has no side rows, and the dense forward without them
    needs less than its query reports (which sizes for the side rows a caller may pass): bf16 only there."""
    lib = L.lib()
    buf = (C.c_char * 4096)()
    d = _dims(SHAPES["tiny_video"], dt)
    for struct, query in zip((L.XpLayerFwd, L.XpLayerBwd, L.XpLayerPooledFwd, L.XpLayerPooledBwd), QUERIES):
        if struct is L.XpLayerFwd and dt != L.XP_BF16:
            continue
        a = _dummy_args(struct, d, buf, dt == L.XP_BF16)
        if hasattr(a, "side_S"):
            a.side_S, a.side_M = d.S, d.M
        entry = query[:-len("_workspace_bytes")]
        a.workspace_bytes = getattr(lib, query)(C.byref(d)) - 1
        assert getattr(lib, entry)(C.byref(a), None) == XP_ERR_ARG, entry
        err = lib.xp_last_error()
        assert entry.encode() + b":" in err and b"workspace too small" in err, err


def test_the_dense_forward_refuses_side_rows_beyond_the_query():
    """the query assumes B*M side rows for a video layer; side_S = side_M = 1 (every row a side row) needs rows of them"""
    lib = L.lib()
    buf = (C.c_char * 4096)()
    d = _dims(SHAPES["tiny_video"])
    a = _dummy_args(L.XpLayerFwd, d, buf, True)
    a.side_x2 = None                                  # (the x2 side rows would live in the workspace)
    a.side_S, a.side_M = 1, 1
    a.workspace_bytes = lib.xp_encoder_layer_fwd_workspace_bytes(C.byref(d))
    assert lib.xp_encoder_layer_fwd(C.byref(a), None) == XP_ERR_ARG
    assert b"xp_encoder_layer_fwd: workspace too small" in lib.xp_last_error()


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(GOLDEN, "w") as f:
        json.dump(_sizes(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}")
