"""The embedding / pooling / normalise / cast kernels of csrc/embed.hip, restated on the CPU, and the ONE set of case tables that
tests/test_embed_ref_cpu.py (the references are right and the tables can tell a wrong kernel from a right one; no GPU) and
tests/test_embed_contract_gpu.py (the kernels) share.  Plain helper module: no package import, no GPU, no tests of its own.

What is restated, and how a GPU result is compared with it
----------------------------------------------------------
index maps      im2col, the uint8 form, proxy rows, tok[ids] + pos[t], gather, scatter, first-maximum argmax: written from the
                definition (which element goes where), not from the kernels' flat-index arithmetic.  Compared with torch.equal.
ordered sums    the embedding-table gradients are fp32 ADDS ONLY, in an order the kernels fix.  With adds only, no fast-math and
                finite normal inputs the result is determined bit for bit by the order (tests/reduce_emulation.py), so the
                tolerance is zero and is derived, not measured:
                    xp_vip_embed_bwd    d_pos[1+l]           0 + dx[b,M+t*L+l] over (b, t) in that order                 (+ old)
                                        d_class / d_added    0 + dx[b,m] over b                                          (+ old)
                                        d_pos[0]             0 + dx[b,m] over b, then m                                  (+ old)
                                        d_time               part[b,t] = 0 + dx[b,M+t*L+l] over l; then xp_splitk_reduce over the
                                                             B slabs, which STARTS from old (reduce_emulation.splitk_reduce)
                    xp_text_embed_bwd   d_tok[id]            dx[r0] + dx[r1] + ... over the rows of id in row order, starting
                                                             from the first occurrence's row itself (not from 0)         (+ old)
                                        d_pos[t]             0 + dx[b,t] over b                                          (+ old)
                    xp_cast_back        src + old, one add per element
                "(+ old)": with accumulate != 0 the finished sum is added to what the destination held, ONE add, last.
                xp_text_embed_bwd finds the occurrences 256 rows at a time from the first occurrence on; `text_embed_bwd` walks the
                same chunks (so that a wrong chunk boundary is expressible: `chunk`), the order of the adds is plain row order.
fp64            l2norm: y = x / |x|, inv = 1 / |x|; dx = inv (dy - y <y, dy>) on the kernel's own y and inv.  Compared with the
                project's tolerances (tests/test_embed_loss_gpu.py): 1e-5 of the tensor scale forward, 1e-5 (fp32) / 6e-3 (bf16)
                backward.  A row of zeros has inv = inf and y = NaN -- what the reference's x / x.norm() gives too.
bf16            every bf16 store of these kernels is one round-to-nearest-even of an fp32 value: `bf16_bits` does it on the bit
                pattern in integer arithmetic (no Tensor.to); a NaN becomes 0x7FC0 and is compared as a NaN (`same`), infinities stay.
The uint8 form is ((u8 / 255) - mean[c]) / std[c] in numpy fp32 in exactly that order, then one rounding to the output type.
"""
import numpy as np
import torch

from tests import reduce_emulation as RE

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = (BF16, F32)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
OTHER_MEAN, OTHER_STD = (0.25, 0.5, 0.7109375), (0.3, 0.125, 1.7)          # a second triple: three distinct values each


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=gen(seed))


# ------------------------------------------------------------------------------------------------------------ bf16 rounding
def bf16_bits(u32, mode="rne"):
    """fp32 bit patterns (numpy uint32) -> bf16 bit patterns (uint16), round to nearest even in integer arithmetic"""
    u = np.asarray(u32, dtype=np.uint32).astype(np.uint64)
    if mode == "truncate":                                           # (a wrong rounding, for tests/test_embed_ref_cpu.py)
        r = u >> np.uint64(16)
    else:
        r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = ((u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)) & ((u & np.uint64(0x007FFFFF)) != 0)
    return np.where(nan, np.uint64(0x7FC0), r).astype(np.uint16)


def f32_bits(t):
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


def from_f32_bits(u32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(u32, dtype=np.uint32)).view(np.int32)).view(torch.float32)


def to_bf16(t, mode="rne"):
    """fp32 tensor -> bfloat16 tensor through `bf16_bits`"""
    b = bf16_bits(f32_bits(t), mode)
    return torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16).view(t.shape)


def store(t, dtype):
    """what store4 leaves of the fp32 value: itself, or its one rounding to bf16"""
    return t.clone() if dtype == F32 else to_bf16(t)


def same(a, b):
    """a and b hold the same bits, except that a NaN matches any NaN (of either sign, any payload)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    it = torch.int16 if a.dtype == BF16 else torch.int32
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(it)[~na], b.contiguous().view(it)[~nb])


# fp32 bit patterns -> the bf16 pattern each must become.  0x3F80 is 1.0; the kept mantissa's last bit is bit 16.
SPECIAL = [
    (0x3F808000, 0x3F80),      # an exact tie, kept mantissa even: down
    (0x3F818000, 0x3F82),      # an exact tie, kept mantissa odd: up
    (0x3F807FFF, 0x3F80),      # one fp32 ulp below a tie
    (0x3F808001, 0x3F81),      # one fp32 ulp above a tie
    (0x3F817FFF, 0x3F81), (0x3F818001, 0x3F82),
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),      # the same ties, negative
    (0x3FFF8000, 0x4000),      # a tie that carries into the exponent: 1.99609375 + half an ulp -> 2.0
    (0x7F7F7FFF, 0x7F7F),      # the largest fp32 that stays finite
    (0x7F7F8000, 0x7F80),      # the smallest that rounds to infinity (a tie on an odd mantissa)
    (0x7F7FFFFF, 0x7F80),      # the fp32 maximum
    (0xFF7F7FFF, 0xFF7F), (0xFF7F8000, 0xFF80),
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),      # +-infinity
    (0x00000000, 0x0000), (0x80000000, 0x8000),      # +-0
    (0x7FC00000, 0x7FC0),      # a quiet NaN
    (0x3F800000, 0x3F80),      # (1.0: pads the table to a multiple of 4)
]
# fp32 subnormals of both signs.  Round-to-nearest-even keeps them (torch's CPU conversion does); a conversion that flushes gives a
# zero of the same sign.  Which of the two the MI355X does is measured by tests/test_embed_contract_gpu.py and stated in the header.
SUBNORMAL = [
    (0x00000001, 0x0000), (0x00008000, 0x0000), (0x00008001, 0x0001), (0x00018000, 0x0002), (0x00400000, 0x0040), (0x007FFFFF, 0x0080),
    (0x80000001, 0x8000), (0x80008000, 0x8000), (0x80008001, 0x8001), (0x80018000, 0x8002), (0x80400000, 0x8040), (0x807FFFFF, 0x8080),
]
assert len(SPECIAL) % 4 == 0 and len(SUBNORMAL) % 4 == 0


def table_f32(table):
    return from_f32_bits(np.array([a for a, _ in table], dtype=np.uint32))


# ------------------------------------------------------------------------------------------------------------ index maps
def im2col(frames, P, swap_grid=False):
    """patches[(bt, gy, gx), (c, py, px)] = frames[bt, c, gy*P+py, gx*P+px]; frames [BT, 3, H, W] of any type -> [BT*gh*gw, 3*P*P].
    swap_grid: a WRONG map for tests/test_embed_ref_cpu.py -- the row index is split with gh where gw belongs (out-of-frame pixels wrap)"""
    BT, C, H, W = frames.shape
    gh, gw = H // P, W // P
    if swap_grid:
        gh, gw = gw, gh
    gy = torch.arange(gh).view(gh, 1, 1, 1, 1)
    gx = torch.arange(gw).view(1, gw, 1, 1, 1)
    c = torch.arange(C).view(1, 1, C, 1, 1)
    py = torch.arange(P).view(1, 1, 1, P, 1)
    px = torch.arange(P).view(1, 1, 1, 1, P)
    y, x = (gy * P + py) % H, (gx * P + px) % W
    return torch.cat([frames[bt][c, y, x].reshape(gh * gw, C * P * P) for bt in range(BT)])


def image_norm_u8(frames_u8, mean, std):
    """uint8 [BT, 3, H, W] -> fp32: ((u8 / 255) - mean[c]) / std[c] in numpy fp32, in that order"""
    x = frames_u8.numpy().astype(np.float32) / np.float32(255.0)
    m, s = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    return torch.from_numpy(((x - m) / s).astype(np.float32))


def proxy_rows(cls, added, pos, B, M):
    """[B, M, D] fp32: row 0 = cls + pos[0], row 1+i = added[i] + pos[0]"""
    rows = [cls + pos[0]] + [added[i] + pos[0] for i in range(M - 1)]
    return torch.stack(rows)[None].repeat(B, 1, 1)


def text_embed(ids, tok, pos):
    """[B, Lt, D] fp32: tok[ids[b, t]] + pos[t]"""
    B, Lt = ids.shape
    return torch.stack([torch.stack([tok[int(ids[b, t])] + pos[t] for t in range(Lt)]) for b in range(B)])


def argmax_rows(ids, last=False):
    """position of the FIRST maximum of every row of int64 ids (last: a wrong one, for the CPU test)"""
    out = []
    for row in ids.tolist():
        best, bi = row[0], 0
        for t, v in enumerate(row):
            if v > best or (last and v == best):
                best, bi = v, t
        out.append(bi)
    return torch.tensor(out, dtype=torch.int64)


def gather_rows(x, idx):
    """x [B, S, D] -> [B, D]: x[b, idx[b]], idx None = row 0"""
    return torch.stack([x[b, 0 if idx is None else int(idx[b])] for b in range(x.shape[0])])


def scatter_rows(dout, idx, S):
    """dout [B, D] -> [B, S, D]: zeros, but row idx[b] (None = 0) of sample b is dout[b]"""
    B, D = dout.shape
    out = torch.zeros(B, S, D, dtype=dout.dtype)
    for b in range(B):
        out[b, 0 if idx is None else int(idx[b])] = dout[b]
    return out


# ------------------------------------------------------------------------------------------------------------ ordered sums
def ordered_sum(x, order="forward", from_zero=True):
    """x [n, ...] fp32 -> the sum over dim 0 as fp32 adds: 'forward' one by one from 0 (from_zero) or from x[0]; 'reversed' and
    'pairwise' are other orders of the same sum (for tests/test_embed_ref_cpu.py)"""
    assert x.dtype == F32
    if order == "pairwise":
        xs = list(x)
        while len(xs) > 1:
            xs = [xs[i] + xs[i + 1] if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
        return xs[0] + 0.0 if from_zero else xs[0].clone()
    idx = list(range(x.shape[0]))
    if order == "reversed":
        idx.reverse()
    s = torch.zeros_like(x[0]) if from_zero else x[idx[0]].clone()
    for i in idx if from_zero else idx[1:]:
        s = s + x[i]
    return s


def _plus_old(s, old, accumulate):
    return s + old if accumulate else s


def vip_embed_bwd(dx, M, T, L, old=None, order="forward"):
    """dx [B, S, D] (its stored values widened to fp32), S = M + T*L -> dict(d_class [D], d_added [M-1, D], d_pos [1+L, D],
    d_time [T, D]).  old: the four destinations' previous contents (accumulate != 0) or None"""
    dx = dx.float()
    B, S, D = dx.shape
    assert S == M + T * L
    acc = old is not None
    fr = dx[:, M:].reshape(B, T, L, D)
    grid = ordered_sum(fr.reshape(B * T, L, D), order)                                           # [L, D], (b, t) order
    prox = ordered_sum(dx[:, :M], order)                                                         # [M, D], over b
    pos0 = ordered_sum(dx[:, :M].reshape(B * M, D), order)                                       # [D], b then m
    part = ordered_sum(fr.permute(2, 0, 1, 3).contiguous(), order)                               # [B, T, D], over l
    if order == "forward":
        d_time = RE.splitk_reduce(part.reshape(B, T * D), old["d_time"].reshape(-1) if acc else None, acc).view(T, D)
    else:
        d_time = _plus_old(ordered_sum(part, order), old["d_time"] if acc else None, acc)
    d_pos = torch.cat([pos0[None], grid])
    return {"d_class": _plus_old(prox[0], old["d_class"] if acc else None, acc),
            "d_added": _plus_old(prox[1:], old["d_added"] if acc else None, acc),
            "d_pos": _plus_old(d_pos, old["d_pos"] if acc else None, acc), "d_time": d_time}


CHUNK = (256, 256)         # text_embed_bwd_tok_kernel: rows looked at per ballot round, distance between two rounds


def text_embed_bwd(ids, dx, vocab, old_tok=None, old_pos=None, order="forward", chunk=CHUNK):
    """ids [B, Lt] int64, dx [B, Lt, D] -> (d_tok [vocab, D], d_pos [npos or Lt, D]).  With old_* (accumulate != 0) the rows of ids
    that do not occur and the d_pos rows >= Lt are the old ones; without, d_tok's are zero and d_pos has Lt rows."""
    dx = dx.float()
    B, Lt, D = dx.shape
    acc = old_tok is not None
    flat, rows = ids.reshape(-1).tolist(), B * Lt
    dxr = dx.reshape(rows, D)
    d_tok = old_tok.clone() if acc else torch.zeros(vocab, D)
    seen = set()
    for r, tid in enumerate(flat):
        if tid in seen:                                     # only the first occurrence of an id works
            continue
        seen.add(tid)
        occ, base = [r], r + 1
        while base < rows:
            occ += [q for q in range(base, min(base + chunk[0], rows)) if flat[q] == tid]
            base += chunk[1]
        d_tok[tid] = _plus_old(ordered_sum(dxr[occ], order, from_zero=False), d_tok[tid], acc)
    pos = ordered_sum(dx, order)                                                                 # [Lt, D], over b
    if acc:
        d_pos = old_pos.clone()
        d_pos[:Lt] = pos + old_pos[:Lt]
    else:
        d_pos = pos
    return d_tok, d_pos


def cast_back(src, old=None):
    return src.float() + old if old is not None else src.float()


# ------------------------------------------------------------------------------------------------------------ l2norm, fp64
def l2norm_fwd64(x):
    xd = x.double()
    n = xd.norm(dim=-1, keepdim=True)
    return xd / n, (1.0 / n)[:, 0]


def l2norm_bwd64(dy, y, inv):
    """on the kernel's own inputs: the fp32 dy, y and inv it reads"""
    dy, y, inv = dy.double(), y.double(), inv.double()
    return inv[:, None] * (dy - y * (y * dy).sum(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------------------ the case tables
IM2COL_CASES = [(1, 8, 8, 8), (2, 32, 48, 16), (3, 40, 24, 8), (1, 64, 32, 32), (5, 64, 64, 16)]               # (BT, H, W, P)
IM2COL_BIG = (128, 224, 224, 16)            # 25088 x 96 eight-element vectors: beyond 8192 blocks of 256 threads
NORMS = {"clip": (CLIP_MEAN, CLIP_STD), "other": (OTHER_MEAN, OTHER_STD)}
PROXY_CASES = [(1, 1, 1, 4), (3, 49, 4, 128), (2, 10, 10, 260)]                                                # (B, S, M, D)
VIP_BWD_CASES = [(1, 1, 1, 1, 4), (3, 4, 5, 9, 128), (2, 1, 3, 8, 768), (4, 4, 4, 7, 1024), (5, 2, 7, 17, 260)]   # (B, M, T, L, D)
TEXT_CASES = [(1, 1, 4, 1), (4, 12, 128, 50), (2, 77, 1028, 30), (9, 32, 512, 40)]                             # (B, Lt, D, V)
TEXT_NPOS_EXTRA = 3                         # npos = Lt + 3 > Lt
CONSTRUCTED = (9, 32, 512, 40)
ARGMAX_CASES = [(1, 1), (65, 77)]                                                                              # (B, Lt)
GATHER_CASES = [(1, 1, 4), (3, 7, 260), (4, 12, 128)]                                                          # (B, S, D)
SCATTER_BIG = (8, 2356, 768)                # 3.6 M four-element vectors: beyond the grid cap, the production shape
L2NORM_CASES = [(1, 4), (3, 260), (4, 256), (5, 768), (9, 512), (130, 1024)]                                   # (rows, cols)
L2NORM_ZERO_ROW = (4, 256)                  # its second row is all zeros
CAST_N = [4, 12, 1028]


def frames_f32(case, seed=0):
    BT, H, W, P = case
    return randn(BT, 3, H, W, seed=1000 + seed + BT + H + 2 * W + P)


def frames_u8(case, seed=0):
    BT, H, W, P = case
    t = torch.randint(0, 256, (BT, 3, H, W), generator=gen(2000 + seed + BT + H + 2 * W + P), dtype=torch.uint8)
    t.view(-1)[:3] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    return t


def proxy_inputs(case):
    B, S, M, D = case
    g = gen(3000 + B + S + M + D)
    cls, pos = torch.randn(D, generator=g), torch.randn(3, D, generator=g)
    return cls, (torch.randn(M - 1, D, generator=g) if M > 1 else None), pos


def vip_bwd_inputs(case, dtype):
    """dx in `dtype`, and the seeded finite previous contents of the four destinations"""
    B, M, T, L, D = case
    g = gen(4000 + B + M + T + L + D)
    dx = torch.randn(B, M + T * L, D, generator=g).to(dtype)
    old = {"d_class": torch.randn(D, generator=g), "d_added": torch.randn(M - 1, D, generator=g),
           "d_pos": torch.randn(1 + L, D, generator=g), "d_time": torch.randn(T, D, generator=g)}
    return dx, old


CONSTRUCTED_R0 = 3


def constructed_ids():
    """ids of CONSTRUCTED (288 rows, vocabulary 40), built, not drawn:
        id 0    rows r0 = 3 and r0 + 255, r0 + 256, r0 + 257 -- offsets 254, 255 of the first 256-row chunk behind r0 and offset 0 of
                the second
        id 1    row 0 only            id 2    the last row only
        id 3    row 10 and row 270: its only repeat lies in the second chunk (rows 267 ..)
        id 39   absent (so are 35 .. 38); every other row cycles through 4 .. 34, each of which repeats every 31 rows: the early ones
                have repeats in both chunks"""
    B, Lt, D, V = CONSTRUCTED
    rows = B * Lt
    ids = [4 + r % 31 for r in range(rows)]
    r0 = CONSTRUCTED_R0
    for r in (r0, r0 + 255, r0 + 256, r0 + 257):
        ids[r] = 0
    ids[0], ids[rows - 1] = 1, 2
    ids[10], ids[270] = 3, 3
    return torch.tensor(ids, dtype=torch.int64).view(B, Lt)


def text_ids(case):
    B, Lt, D, V = case
    if case == CONSTRUCTED:
        return constructed_ids()
    if V == 1:
        return torch.zeros(B, Lt, dtype=torch.int64)
    g = gen(5000 + B + Lt + D + V)
    ids = torch.randint(0, V - 3, (B, Lt), generator=g)          # V-2 and V-3 never occur
    for b in range(B):
        ids[b, Lt // 2 + b:] = V - 1                              # a padding id that repeats
    return ids


def text_inputs(case, dtype):
    B, Lt, D, V = case
    g = gen(6000 + B + Lt + D + V)
    npos = Lt + TEXT_NPOS_EXTRA
    return {"ids": text_ids(case), "tok": torch.randn(V, D, generator=g), "pos": torch.randn(npos, D, generator=g),
            "dx": torch.randn(B, Lt, D, generator=g).to(dtype), "old_tok": torch.randn(V, D, generator=g),
            "old_pos": torch.randn(npos, D, generator=g), "npos": npos}


def argmax_ids(case):
    B, Lt = case
    ids = torch.randint(0, 1000, (B, Lt), generator=gen(7000 + B + Lt))
    if Lt > 1:
        ids[0, 0] = 5000                                          # the maximum first
        ids[1, Lt - 1] = 5000                                     # last
        ids[2, 10] = ids[2, 20] = ids[2, Lt - 1] = 5000           # repeated: the first wins
        ids[3, 2] = ids[3, 30] = (1 << 32) + 7                    # above 2^32: a 32-bit compare sees 7 and 0
        ids[3, 9] = ids[3, 40] = 1 << 33
        ids[B - 1, 5] = ids[B - 1, 6] = 7000                      # row 64: the second block
    return ids


def gather_inputs(case, dtype):
    B, S, D = case
    g = gen(8000 + B + S + D)
    x = torch.randn(B, S, D, generator=g).to(dtype)
    dout = torch.randn(B, D, generator=g).to(dtype)
    idx = torch.randint(0, S, (B,), generator=g)
    idx[0] = 0
    if B >= 3:
        idx[1], idx[2] = S - 1, S - 1                             # the last row, twice
    return x, dout, idx


def l2norm_inputs(case, dtype, zero_row=False):
    rows, cols = case
    g = gen(9000 + rows + cols)
    x = torch.randn(rows, cols, generator=g).to(dtype)
    if zero_row:
        x[1] = 0
    return x, torch.randn(rows, cols, generator=g)


def cast_input(n):
    """the special values, then seeded normal values up to n elements (n < the table: its first n)"""
    sp = table_f32(SPECIAL)
    return torch.cat([sp, randn(max(n - sp.numel(), 0), seed=n)])[:n].contiguous()
