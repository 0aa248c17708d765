"""GPU: the summation ORDER of the fp32 row reductions (csrc/reduce.hip, and xp_layernorm_bwd's two levels in csrc/layernorm.hip)
against tests/reduce_emulation.py, bit for bit.

The kernels only add: no multiplies, no fast-math, seeded randn inputs (no denormals, no overflow).  The result of a sequence of
IEEE fp32 additions is determined by its order, so the tolerance is zero -- derived, not measured -- and every comparison is
``torch.equal``.  tests/test_reduce_order_cpu.py shows that the orders restated there are distinguishable on such inputs.
Every output is pre-filled with 3.0 and every case runs with accumulate off and on."""
import functools

import pytest
import torch

from tests import reduce_emulation as E

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float32]
FILL = 3.0


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _filled(n, device="cuda"):
    return torch.full((n,), FILL, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------ xp_reduce_rows_batch (H.DeferredReduce)
# (nrows, width, stride): every nrows of {1, 4, 5, 8, 9, 13, 64, 65, 589, 1024, 1025} -- one row, the residues of tree A's 8-row
# stride, both sides of RB_DIRECT = 64, a ragged last group (589 = 31 * 19), 32 full groups and one more -- and every (width, stride)
# of {(4, 8), (64, 64), (200, 256), (260, 260), (768, 1536)} -- one vector lane, one scalar block, a pitch, a ragged last block of
# either kernel form, three vector blocks.  Every segment is 16-byte addressable: the batch runs four columns per lane.
VECTOR = ((1, 4, 8), (4, 64, 64), (5, 200, 256), (8, 260, 260), (9, 768, 1536), (13, 4, 8), (64, 64, 64), (65, 200, 256),
          (589, 260, 260), (1024, 768, 1536), (1025, 4, 8), (1025, 768, 1536), (64, 260, 260), (65, 64, 64), (13, 200, 256))
SCALAR = VECTOR + ((9, 6, 7),)             # one segment that is not: the whole batch runs one column per lane
CHUNKED = tuple((n, 64, 64) for n in (1, 4, 5, 8, 9, 13, 64, 65, 589, 1024, 1025, 2, 3, 66, 100, 33, 7))    # 17 > XP_REDUCE_MAX_SEGS


@functools.lru_cache(maxsize=None)
def _batch_case(specs):
    """(inputs [nrows, stride] on the CPU, emulated sums) per segment.  Shared: never modify."""
    parts = [_randn(nrows, stride, seed=100 * i + nrows) for i, (nrows, _, stride) in enumerate(specs)]
    return parts, [E.batch_segment(p[:, :width].contiguous()) for p, (_, width, _) in zip(parts, specs)]


@pytest.mark.parametrize("flip", [0, 1], ids=["acc-odd", "acc-even"])
@pytest.mark.parametrize("specs", [VECTOR, SCALAR, CHUNKED], ids=["vector", "scalar", "17-segments"])
def test_reduce_rows_batch(specs, flip):
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    assert (len(specs) > L.XP_REDUCE_MAX_SEGS) == (specs is CHUNKED)
    parts, sums = _batch_case(specs)
    d = H.DeferredReduce(torch.device("cuda"))
    dev, outs = [p.cuda() for p in parts], []
    for i, ((nrows, width, stride), p) in enumerate(zip(specs, dev)):
        outs.append(_filled(width))
        d.add(p, 0, outs[-1], nrows, width, stride, accumulate=(i + flip) % 2 == 1)
    d.flush()
    for i, (spec, o, t) in enumerate(zip(specs, outs, sums)):
        acc = (i + flip) % 2 == 1
        assert torch.equal(o.cpu(), E.finish(t, torch.full_like(t, FILL), acc)), (spec, acc)


# ------------------------------------------------------------------------------------ xp_colsum_partials + flush, xp_colsum
# 1056 and 2048 rows of 256 columns are 33 and 64 chunks: the range in which xp_colsum's partition of the chunk partials (pairs
# first) and the batch path's (direct) differ; (10923, 3072) is the smallest row count at which cs_rows returns 64
COLSUM = [(1, 4), (7, 64), (33, 200), (1056, 256), (2048, 256), (2356, 768)]
COLSUM_CASES = [(r, c, dt) for r, c in COLSUM for dt in DTYPES] + [(10923, 3072, torch.bfloat16)]


@functools.lru_cache(maxsize=None)
def _colsum_case(rows, cols, dtype):
    """(X on the CPU in `dtype`, emulated xp_colsum, emulated partials + batch flush).  Shared: never modify."""
    X = _randn(rows, cols, seed=rows + cols).to(dtype)
    return X, E.colsum(X), E.colsum_deferred(X)


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("rows,cols,dtype", COLSUM_CASES, ids=[f"{r}x{c}-{str(dt)[6:]}" for r, c, dt in COLSUM_CASES])
def test_colsum(rows, cols, dtype, accumulate):
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    X, t_colsum, t_deferred = _colsum_case(rows, cols, dtype)
    assert L.lib().xp_colsum_partial_rows(rows, cols) == E.cdiv(rows, E.cs_rows(rows, cols))
    if (rows, cols) == (10923, 3072):
        assert E.cs_rows(rows, cols) == 64
    Xd, fill = X.cuda(), torch.full((cols,), FILL)
    out = H.colsum(Xd, rows, cols, out=_filled(cols), accumulate=accumulate)
    assert torch.equal(out.cpu(), E.finish(t_colsum, fill, accumulate))
    d = H.DeferredReduce(Xd.device)
    out = H.colsum_deferred(Xd, rows, cols, d, out=_filled(cols), accumulate=accumulate)
    d.flush()
    assert torch.equal(out.cpu(), E.finish(t_deferred, fill, accumulate))


# ------------------------------------------------------------------------------------ xp_splitk_reduce
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("splits", [1, 2, 3, 4, 5, 7, 8, 9])
def test_splitk_reduce_order(splits, accumulate):
    from xpretrain_amd import hip_ops as H
    n = 4 * 300
    slabs = _randn(splits, n, seed=splits)
    out = H.splitk_reduce(slabs.cuda(), _filled(n), accumulate=accumulate)
    assert torch.equal(out.cpu(), E.splitk_reduce(slabs, torch.full((n,), FILL), accumulate))


# ------------------------------------------------------------------------------------ xp_layernorm_bwd (immediate form)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("cols", [192, 768])
@pytest.mark.parametrize("rows", [16, 144, 600, 4712])          # 1, 9, 38, 295 partial rows: groups of 1, 1, 2, 10 at level 1
def test_layernorm_bwd_param_reduce(rows, cols, dtype):
    """dgamma / dbeta of H.layernorm_bwd without a DeferredReduce are tree A over groups of ceil(blocks / 32) of the per-block
    partial rows ln_bwd_kernel left in the "ln" workspace (rows_reduce_kernel), then tree B (ln_param_reduce2_kernel)."""
    from xpretrain_amd import _lib as L
    from xpretrain_amd import hip_ops as H
    x = _randn(rows, cols, seed=rows + cols).to(dtype).cuda()
    dy = _randn(rows, cols, seed=rows + cols + 1).to(dtype).cuda()
    gamma = _randn(cols, seed=cols).cuda()
    mean, rstd = x.float().mean(1), 1.0 / x.float().var(1, unbiased=False).add(1e-5).sqrt()
    blocks = E.ln_bwd_blocks(rows)
    assert L.lib().xp_layernorm_bwd_partial_rows(rows) == blocks
    for accumulate in (False, True):
        _, dg, db = H.layernorm_bwd(dy, x, gamma, mean, rstd, rows, cols, dgamma=_filled(cols), dbeta=_filled(cols),
                                    accumulate=accumulate)
        ws = H.workspace(L.lib().xp_layernorm_bwd_workspace_bytes(rows, cols), x.device, "ln")      # grow-only: the buffer the call used
        part = ws[:blocks * 2 * cols * 4].view(torch.float32).view(blocks, 2 * cols).cpu()
        fill = torch.full((cols,), FILL)
        want_g, want_b = E.ln_param_reduce(part, cols, fill, fill, accumulate)
        assert torch.equal(dg.cpu(), want_g), ("dgamma", accumulate)
        assert torch.equal(db.cpu(), want_b), ("dbeta", accumulate)
