"""A CPU restatement of the summation ORDER of the fp32 row reductions in csrc/reduce.hip and csrc/layernorm.hip (plain helper
module).  Everything here is fp32 additions on torch CPU tensors, one row at a time, vectorised over the columns: with adds only,
no fast-math and finite normal inputs the GPU result is determined bit for bit by the order, so tests/test_reduce_gpu.py compares
with ``torch.equal``.

    tree A   wave w of 4 takes rows r0+w, r0+w+8, ... into s0 and rows r0+w+4, r0+w+12, ... into s1; the wave result is s0 + s1;
             the four wave results are combined as ((W0 + W1) + W2) + W3                              (reduce.hip::tree_a)
    tree B   one accumulator per wave over rows w, w+4, ...; the same four-wave combine             (ln_param_reduce2_kernel)

and the partitions that feed rows to them:

    batch    nrows <= 64: tree A over all rows.  Otherwise nsum = ceil(nrows / 32): tree A over each group of nsum consecutive rows,
             then tree A over the ceil(nrows / nsum) group sums                                        (xp_reduce_rows_batch)
    colsum   chunks of cs_rows(rows, cols) rows of X, tree A each; then ALWAYS two levels, lvl = ceil(chunks / 32): tree A over each
             group of lvl chunk partials, tree A over the ceil(chunks / lvl) group sums               (xp_colsum)

The two partitions give the same tree except for 33..64 partial rows (batch: direct; colsum: groups of 2).  Nothing here is measured
on a GPU."""
import torch

RB_DIRECT = 64


def cdiv(a, b):
    return (a + b - 1) // b


def tree_a(x, r0=0, r1=None):
    """sum of rows [r0, r1) of x [rows, width] (fp32) in tree A's order -> [width]"""
    r1 = x.shape[0] if r1 is None else r1
    waves = []
    for w in range(4):
        s0 = torch.zeros(x.shape[1], dtype=torch.float32)
        s1 = torch.zeros(x.shape[1], dtype=torch.float32)
        r = r0 + w
        while r + 4 < r1:
            s0 = s0 + x[r]
            s1 = s1 + x[r + 4]
            r += 8
        if r < r1:
            s0 = s0 + x[r]
        waves.append(s0 + s1)
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def tree_b(x):
    """sum of all rows of x [rows, width] in tree B's order -> [width]"""
    waves = []
    for w in range(4):
        s = torch.zeros(x.shape[1], dtype=torch.float32)
        for r in range(w, x.shape[0], 4):
            s = s + x[r]
        waves.append(s)
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def groups_a(x, nsum):
    """tree A over each group of nsum consecutive rows of x -> [ceil(rows / nsum), width]"""
    n = x.shape[0]
    return torch.stack([tree_a(x, r0, min(r0 + nsum, n)) for r0 in range(0, n, nsum)])


def finish(t, out, accumulate):
    return out + t if accumulate else t


def batch_segment(x, out=None, accumulate=False):
    """one segment of xp_reduce_rows_batch: x = the segment's [nrows, width] columns (pitch already removed)"""
    n = x.shape[0]
    t = tree_a(x) if n <= RB_DIRECT else tree_a(groups_a(x, cdiv(n, 32)))
    return finish(t, out, accumulate)


def cs_rows(rows, cols):
    """rows per chunk of colsum_partial_kernel (reduce.hip::cs_rows)"""
    per = rows * cdiv(cols, 256) // 2048
    return 128 if per >= 128 else 64 if per >= 64 else 32


def colsum_partials(X):
    """xp_colsum_partials: one tree-A partial row per chunk of cs_rows rows; bf16 is widened to fp32 first, as the kernel's loads do"""
    return groups_a(X.float(), cs_rows(*X.shape))


def colsum(X, out=None, accumulate=False):
    """xp_colsum: its own two-level partition of the chunk partials"""
    part = colsum_partials(X)
    part2 = groups_a(part, cdiv(part.shape[0], 32))
    return finish(tree_a(part2), out, accumulate)


def colsum_deferred(X, out=None, accumulate=False):
    """xp_colsum_partials, finished by xp_reduce_rows_batch (hip_ops.colsum_deferred + DeferredReduce.flush)"""
    return batch_segment(colsum_partials(X), out, accumulate)


def splitk_reduce(slabs, out=None, accumulate=False):
    """xp_splitk_reduce: slabs [splits, n]; s = accumulate ? out : 0, groups of four slabs as s += (a+b)+(c+d), the rest one by one"""
    s = out.clone() if accumulate else torch.zeros(slabs.shape[1], dtype=torch.float32)
    z, splits = 0, slabs.shape[0]
    while z + 4 <= splits:
        s = s + ((slabs[z] + slabs[z + 1]) + (slabs[z + 2] + slabs[z + 3]))
        z += 4
    while z < splits:
        s = s + slabs[z]
        z += 1
    return s


def ln_bwd_blocks(rows):
    """partial rows ln_bwd_kernel writes (layernorm.hip::bwd_blocks)"""
    return max(1, min(512, cdiv(rows, 16)))


def ln_param_reduce(part, cols, dgamma=None, dbeta=None, accumulate=False):
    """xp_layernorm_bwd's two levels over the per-block partial rows part [blocks, 2 * cols]: tree A over groups of
    ceil(blocks / 32) rows, then tree B; the result is split into (dgamma, dbeta)"""
    t = tree_b(groups_a(part, cdiv(part.shape[0], 32)))
    return finish(t[:cols], dgamma, accumulate), finish(t[cols:], dbeta, accumulate)
