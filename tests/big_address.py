"""Operands beyond 2 GiB / 4 GiB for the -m gpu tests (plain helper module in the style of tests/guarded.py, no tests of its own).

``Guarded.check`` of tests/guarded.py builds a boolean mask and an indexed copy of the whole buffer: at 4 GiB that is 10 GiB of
temporaries.  Here nothing of an operand's size is ever built twice: ``Pitched`` fills a [rows, ld] matrix on the device (padding =
PAD_VALUE, seeded randn in the [rows, cols] window only, drawn in row chunks) and proves that it is unchanged by drawing the same
numbers again; ``BigGuarded`` is an output of the same shape filled with the 0x7FA5 pattern whose check walks the buffer in chunks
of 64 Mi elements (counted with count_nonzero: summing a boolean tensor builds an int64 copy of it, 2 GiB per 256 Mi elements);
``boundary_rows`` names the rows every case must compare: both ends of the operand and both sides of every power-of-two byte
offset (2^31, 2^32, 2^33) the operand crosses, where a 32-bit offset wraps or changes sign."""
import torch

from tests.guarded import _SENT

DEVICE = "cuda"
PAD_VALUE = 1000.0                    # input elements outside the operands' extents (tests/test_gemm_plans_gpu.py)
CHUNK = 64 << 20                      # elements: the most any check touches at once (a comparison's result: one byte each)
FILL = 32 << 20                       # elements of randn drawn at once (fp32, then rounded to the operand's type)


def _row_chunks(rows, row_elems, limit):
    step = max(1, limit // max(1, row_elems))
    return [(r, min(rows, r + step)) for r in range(0, rows, step)]


class Pitched:
    """[rows, ld] on the device: ``scale * randn`` (seeded) in columns [0, cols), PAD_VALUE in the padding; never on the host.
    ``grid``: the values are rounded to multiples of it (sums of products of such values are exact in fp32 far longer).
    ``values`` (a small [rows, cols] tensor, e.g. an existing case's own seeded inputs) replaces the drawn numbers."""

    def __init__(self, rows, cols, ld, dtype, seed=0, scale=1.0, grid=None, values=None):
        assert ld >= cols and (values is None or tuple(values.shape) == (rows, cols))
        self.rows, self.cols, self.ld, self.dtype, self.seed, self.scale, self.grid = rows, cols, ld, dtype, seed, scale, grid
        self.values = None if values is None else values.to(device=DEVICE, dtype=dtype).clone()
        self.mat = torch.empty((rows, ld), dtype=dtype, device=DEVICE)
        if ld > cols:
            self.mat.fill_(PAD_VALUE)
        for r0, r1, vals in self._draw():
            self.mat[r0:r1, :cols] = vals

    def _draw(self):
        if self.values is not None:
            yield 0, self.rows, self.values
            return
        g = torch.Generator(device=DEVICE).manual_seed(self.seed)
        for r0, r1 in _row_chunks(self.rows, self.cols, FILL):
            v = torch.randn((r1 - r0, self.cols), generator=g, device=DEVICE) * self.scale
            if self.grid:
                v = torch.round(v / self.grid) * self.grid
            yield r0, r1, v.to(self.dtype)

    @property
    def nbytes(self):
        return self.rows * self.ld * self.mat.element_size()

    def window(self, rows):
        """[len(rows), cols]: the values of the given rows (an index tensor)"""
        return self.mat[rows, :self.cols]

    def assert_unchanged(self, tag):
        """the window holds the numbers of the seed, the padding PAD_VALUE -- compared chunk by chunk on the device"""
        for r0, r1, vals in self._draw():
            assert torch.equal(self.mat[r0:r1, :self.cols], vals), f"{tag}: input rows {r0}..{r1} changed"
        if self.ld > self.cols:
            for r0, r1 in _row_chunks(self.rows, self.ld, CHUNK):
                bad = int(torch.count_nonzero(self.mat[r0:r1, self.cols:] != PAD_VALUE))
                assert bad == 0, f"{tag}: {bad} padding elements of input rows {r0}..{r1} changed"


class BigGuarded:
    """a [rows, ld] output inside a flat buffer that holds the sentinel bit pattern (0x7FA5 / 0x7FA5A5A5: a NaN) in front of it,
    behind it and in every element the kernel must not write"""

    def __init__(self, rows, ld, dtype, lead=64):
        self.itype, self.sent = _SENT[dtype]
        self.lead, self.rows, self.ld = lead, rows, ld
        self.flat = torch.empty(lead + rows * ld + lead, dtype=dtype, device=DEVICE)
        self.flat.view(self.itype).fill_(self.sent)
        self.mat = self.flat[lead:lead + rows * ld].view(rows, ld)

    def outside_window(self, written, ncols):
        """the number of elements outside columns [0, ncols) of the written rows (an int: the first rows; or a bool [rows] mask) that
        no longer hold the pattern; walks the buffer in chunks of at most CHUNK elements"""
        bits = self.flat.view(self.itype)
        end = self.lead + self.rows * self.ld
        bad = int(torch.count_nonzero(bits[:self.lead] != self.sent)) + int(torch.count_nonzero(bits[end:] != self.sent))
        body = bits[self.lead:end].view(self.rows, self.ld)
        if isinstance(written, int):
            n = written
            written = torch.zeros(self.rows, dtype=torch.bool, device=DEVICE)
            written[:n] = True
        for r0, r1 in _row_chunks(self.rows, self.ld, CHUNK):
            blk = body[r0:r1]
            if ncols < self.ld:
                bad += int(torch.count_nonzero(blk[:, ncols:] != self.sent))
            if ncols > 0:
                bad += int(torch.count_nonzero(blk[~written[r0:r1], :ncols] != self.sent))
        return bad

    def check(self, tag, written, ncols):
        bad = self.outside_window(written, ncols)
        assert bad == 0, f"{tag}: {bad} elements written outside the output window"


def boundary_rows(rows, ld, esz, tile, seed=0, random_rows=256):
    """Sorted row indices (int64, on the device) every case compares: the first and the last ``tile`` rows; the ``tile`` rows on each
    side of byte offsets 2^31 and 2^32 of a [rows, ld] operand of ``esz``-byte elements, and of 2^33 where the operand reaches it;
    ``random_rows`` seeded random rows."""
    pick = set(range(min(tile, rows))) | set(range(max(0, rows - tile), rows))
    for p in (31, 32, 33):
        if rows * ld * esz > 1 << p:
            r = (1 << p) // (ld * esz)                  # the row that holds (or begins at) the boundary byte
            pick |= set(range(max(0, r - tile), min(rows, r + tile)))
    g = torch.Generator().manual_seed(seed)
    pick |= set(torch.randint(0, rows, (random_rows,), generator=g).tolist())
    return torch.tensor(sorted(pick), dtype=torch.int64, device=DEVICE)


def crossed(rows, ld, esz):
    """the power-of-two byte offsets a [rows, ld] operand crosses"""
    return [p for p in (31, 32, 33) if rows * ld * esz > 1 << p]
