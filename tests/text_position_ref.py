"""CLIPTextEmbeddings with caller-given position ids (csrc/text_embed_pos.hip: xp_text_embed_fwd_pos / xp_text_embed_bwd_pos),
restated in numpy from the definition.  Plain helper module: no package import, no GPU, no tests of its own.

forward     x[b,t] = tok[ids[b,t]] + pos[pos_ids[b % pos_B, t]]: an index map, ONE fp32 add, and -- bf16 output -- one round to
            nearest even of that fp32 value (tests/embed_ref.py::to_bf16, integer arithmetic on the bit pattern).  A position id
            outside [0, n_pos) makes the whole row NaN and reads no table row.  With one add there is nothing to reorder: a GPU
            result is compared with torch.equal (``embed_ref.same``: a NaN matches a NaN).
backward    fp32 ADDS ONLY, in row order.  table[k] = dx[r0] + dx[r1] + ... over the rows r0 < r1 < ... whose key is k, starting
            from the first occurrence's row itself (not from 0); accumulate: + old, ONE add, last.  Rows of the table no key names
            are zero (store) or the old ones (accumulate).  The keys of d_tok are ids (trusted, as xp_text_embed_bwd trusts them);
            the keys of d_pos are the position ids the rows read, and a row whose id is outside the table adds to nothing.  With
            adds only and finite inputs the order fixes every bit (tests/reduce_emulation.py): the tolerance is zero.
            The kernel finds a key's later occurrences 256 rows at a time (``CHUNK``, the ballot round of
            text_embed_bwd_tok_kernel); the order of the adds is plain row order whatever the round, so the restatement does
            not walk rounds -- the GPU cases put one key on the rows at both sides of every round boundary instead.
``*64``     the same two maps in fp64 (exact index map, fp64 sums): what tests/test_text_position_cpu.py holds the reference's own
            fp32 results against, with the bounds of one fp32 rounding (forward) and of a recursive fp32 sum (backward).
"""
import numpy as np
import torch

from tests import embed_ref as R

CHUNK = 256


def position_rows(pos_ids, B, Lt):
    """[Lt], [1, Lt] or [B, Lt] -> int64 numpy [B, Lt]: the id row (b, t) reads, pos_ids[b % pos_B, t]"""
    p = np.asarray(pos_ids.numpy() if isinstance(pos_ids, torch.Tensor) else pos_ids, dtype=np.int64)
    p = p.reshape(1, -1) if p.ndim == 1 else p
    assert p.ndim == 2 and p.shape[1] == Lt and p.shape[0] in (1, B), p.shape
    return np.stack([p[b % p.shape[0]] for b in range(B)])


def _embed(ids, pos_ids, tok, pos, ftype):
    ids = np.asarray(ids.numpy(), dtype=np.int64)
    B, Lt = ids.shape
    tok, pos = tok.numpy().astype(ftype), pos.numpy().astype(ftype)
    rows = position_rows(pos_ids, B, Lt)
    x = np.full((B, Lt, tok.shape[1]), np.nan, dtype=ftype)
    for b in range(B):
        for t in range(Lt):
            p = int(rows[b, t])
            if 0 <= p < pos.shape[0]:
                x[b, t] = tok[ids[b, t]] + pos[p]
    return torch.from_numpy(x)


def text_embed_pos(ids, pos_ids, tok, pos):
    """[B, Lt, D] fp32: one fp32 add per element; ``embed_ref.store(x, dtype)`` is what the kernel leaves of it"""
    return _embed(ids, pos_ids, tok, pos, np.float32)


def text_embed_pos64(ids, pos_ids, tok, pos):
    return _embed(ids, pos_ids, tok, pos, np.float64)


def _scatter(keys, n_keys, dxr, old, ftype, checked):
    """table [n_keys, D]: per key the sum of its rows of dxr [rows, D] in row order, from the first row itself; + old, last"""
    table = np.zeros((n_keys, dxr.shape[1]), dtype=ftype) if old is None else old.numpy().astype(ftype)
    seen = {}
    for r, k in enumerate(keys):
        if checked and not 0 <= k < n_keys:
            continue
        seen.setdefault(int(k), []).append(r)
    for k, occ in seen.items():
        s = dxr[occ[0]].copy()
        for r in occ[1:]:
            s = s + dxr[r]
        table[k] = s if old is None else s + table[k]
    return torch.from_numpy(table)


def _bwd(ids, pos_ids, dx, vocab, n_pos, old_tok, old_pos, ftype):
    B, Lt = ids.shape
    dxr = dx.float().numpy().astype(ftype).reshape(B * Lt, -1)          # (a bf16 dx widens exactly)
    d_tok = _scatter(ids.reshape(-1).tolist(), vocab, dxr, old_tok, ftype, checked=False)
    d_pos = _scatter(position_rows(pos_ids, B, Lt).reshape(-1).tolist(), n_pos, dxr, old_pos, ftype, checked=True)
    return d_tok, d_pos


def text_embed_bwd_pos(ids, pos_ids, dx, vocab, n_pos, old_tok=None, old_pos=None):
    """ids [B, Lt] int64, dx [B, Lt, D] -> (d_tok [vocab, D], d_pos [n_pos, D]) fp32, the ordered fp32 sums; old_*: accumulate"""
    return _bwd(ids, pos_ids, dx, vocab, n_pos, old_tok, old_pos, np.float32)


def text_embed_bwd_pos64(ids, pos_ids, dx, vocab, n_pos):
    return _bwd(ids, pos_ids, dx, vocab, n_pos, None, None, np.float64)


def sum_bound(keys, n_keys, dx):
    """[n_keys, D] fp64: the a-priori bound (n - 1) 2^-24 sum_i |dx_i| (to first order) of a recursive fp32 sum of a key's n rows
    against their exact sum -- any order of the adds (Higham, Accuracy and Stability of Numerical Algorithms, (4.4))"""
    B, Lt = dx.shape[:2]
    dxr = dx.double().numpy().reshape(B * Lt, -1)
    mag, cnt = np.zeros((n_keys, dxr.shape[1])), np.zeros(n_keys)
    for r, k in enumerate(keys):
        if 0 <= k < n_keys:
            mag[k] += np.abs(dxr[r])
            cnt[k] += 1
    return torch.from_numpy(np.maximum(cnt - 1, 0)[:, None] * 2.0 ** -24 * mag * (1 + 1e-6))


# ------------------------------------------------------------------------------------------------------------ GPU case inputs
def inputs(B, Lt, D, vocab, n_pos, pos_B, dtype, seed=0, accumulate=False):
    """seeded inputs of one kernel case: every position of the table but ``hole`` (an unreferenced row between referenced ones,
    when the table has three rows or more) is drawn, repeats included"""
    g = R.gen(1000 + seed)
    hole = n_pos // 2 if n_pos >= 3 else None
    pool = torch.tensor([p for p in range(n_pos) if p != hole])
    pos_ids = pool[torch.randint(0, len(pool), (pos_B, Lt), generator=g)]
    if Lt >= len(pool):
        pos_ids[0, torch.randperm(Lt, generator=g)[:len(pool)]] = pool          # every other row of the table is named at least once
    out = dict(ids=torch.randint(0, vocab, (B, Lt), generator=g), pos_ids=pos_ids, hole=hole,
               tok=torch.randn(vocab, D, generator=g), pos=torch.randn(n_pos, D, generator=g),
               dx=torch.randn(B, Lt, D, generator=g).to(dtype))
    if accumulate:
        out.update(old_tok=torch.randn(vocab, D, generator=g), old_pos=torch.randn(n_pos, D, generator=g))
    return out
