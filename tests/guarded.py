"""Guard buffers for the -m gpu tests (plain helper module, no tests of its own).

``Guarded``: an output matrix inside a flat buffer that holds a NaN bit pattern in front of it, behind it and in every element the
kernel must not write.  ``GuardedWorkspaces``: replaces ``hip_ops.workspace`` so that every scratch request of the library gets a
fresh buffer of EXACTLY the requested size between two guards, all of it poisoned -- the ordinary allocator never hands out fewer
than 1 MiB and only grows, so without this no kernel ever runs with the size its ``*_workspace_bytes`` function reports, an overrun
lands in slack, and a scratch word read before it is written sees the previous user's (run to run identical) bits."""
import torch

_SENT = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}      # NaN bit patterns


class Guarded:
    """a [rows, cols] matrix inside a flat buffer that holds a sentinel bit pattern in front of it, after it and in every
    element the kernel must not write"""

    def __init__(self, rows, cols, dtype, lead=64, tail_rows=2):
        self.itype, self.sent = _SENT[dtype]
        self.lead, self.rows, self.cols = lead, rows, cols
        self.flat = torch.empty(lead + (rows + tail_rows) * cols + lead, dtype=dtype, device="cuda")
        self.flat.view(self.itype).fill_(self.sent)
        self.mat = self.flat[lead:lead + rows * cols].view(rows, cols)

    def check(self, tag, rows, ncols):
        """nothing outside columns [0, ncols) of `rows` (a row-index tensor, or an int: the first rows) was written"""
        written = torch.zeros(self.flat.numel(), dtype=torch.bool, device="cuda")
        w = written[self.lead:self.lead + self.rows * self.cols].view(self.rows, self.cols)
        if isinstance(rows, int):
            w[:rows, :ncols] = True
        else:
            w[rows, :ncols] = True
        bad = (self.flat.view(self.itype)[~written] != self.sent).sum().item()
        assert bad == 0, f"{tag}: {bad} elements written outside the output window"


def _guarded_defer(nrows, N):
    """a DeferredReduce whose partial-row slot sits in a Guarded buffer"""
    from xpretrain_amd import hip_ops as H

    class Defer(H.DeferredReduce):
        def slot(self, nbytes, name):
            assert nbytes == nrows * N * 4
            self.guard = Guarded(nrows, N, torch.float32)
            return self.guard.mat
    return Defer(torch.device("cuda"))


class GuardedWorkspaces:
    """Context manager: while active, ``xpretrain_amd.hip_ops.workspace`` -- the one function every scratch buffer of the project
    comes from, inside hip_ops and as ``H.workspace`` in functional.py -- returns a fresh uint8 view of exactly ``nbytes`` elements
    (so ``numel() == nbytes`` reaches the library's ``workspace_bytes`` checks), 4096-byte aligned, inside a private buffer with a
    64 KiB guard in front and a 1 MiB guard behind.  The whole buffer, body included, is filled on the current stream with the
    16-bit pattern 0x7FA5: a NaN as bf16 and as fp32, a large positive int32 (a stale counter reads "all problems taken", never a
    negative index).  A request of 0 bytes gets a 256-byte body (a zero-element tensor has a null ``data_ptr()``).

    Every buffer stays alive until the manager is dropped -- the weight-gradient GEMMs run on the library's side stream, so nothing
    may go back to the caching allocator before ``check()`` has synchronised.  ``check()``: every guard still holds the pattern."""
    PATTERN, FRONT, BACK, ALIGN = 0x7FA5, 64 << 10, 1 << 20, 4096

    def __init__(self):
        self.records = []          # (tag, nbytes, stream)
        self._bufs = []            # (tag, nbytes, raw buffer, offset of the body, body bytes)
        self._saved = None

    # ---- the replacement of hip_ops.workspace
    def workspace(self, nbytes, device, tag="ws"):
        nbytes = int(nbytes)
        body = nbytes if nbytes > 0 else 256
        raw = torch.empty(self.FRONT + body + (body & 1) + self.BACK + self.ALIGN, dtype=torch.uint8, device=device)
        raw.view(torch.int16).fill_(self.PATTERN)            # (on the current stream, in front of the kernels that use the buffer)
        off = self.FRONT + (-(raw.data_ptr() + self.FRONT)) % self.ALIGN
        view = raw[off:off + body]
        assert view.data_ptr() % self.ALIGN == 0 and view.numel() == body
        self.records.append((tag, nbytes, torch.cuda.current_stream().cuda_stream))
        self._bufs.append((tag, nbytes, raw, off, body))
        return view

    def __enter__(self):
        from xpretrain_amd import hip_ops as H
        assert self._saved is None
        self._saved = H.workspace
        H.workspace = self.workspace
        return self

    def __exit__(self, *exc):
        from xpretrain_amd import hip_ops as H
        H.workspace = self._saved
        self._saved = None
        return False

    # ---- after the run
    def _pattern_holds(self, tag, what, raw, lo, hi, base):
        """bytes [lo, hi) of `raw` still hold the pattern (little-endian: 0xA5 at even offsets of the buffer, 0x7F at odd ones)"""
        where = f"workspace {tag!r}: {what} changed"
        if lo < hi and lo & 1:
            assert int(raw[lo]) == self.PATTERN >> 8, f"{where} at byte offset {lo - base} relative to the body"
            lo += 1
        if lo < hi and hi & 1:
            assert int(raw[hi - 1]) == self.PATTERN & 0xFF, f"{where} at byte offset {hi - 1 - base} relative to the body"
            hi -= 1
        if lo >= hi:
            return
        bad = (raw[lo:hi].view(torch.int16) != self.PATTERN).nonzero()
        assert bad.numel() == 0, f"{where}, first in the 16-bit word at byte offset {lo + 2 * int(bad[0]) - base} relative to the body " \
                                 f"({bad.numel()} words)"

    def check(self):
        """synchronise, then: every guard (front, and everything behind the body) still holds the pattern"""
        torch.cuda.synchronize()
        for tag, nbytes, raw, off, body in self._bufs:
            self._pattern_holds(tag, "the guard in front of the body", raw, 0, off, off)
            end = off + body
            self._pattern_holds(tag, f"the guard behind the {nbytes}-byte body", raw, end, raw.numel(), off)

    def bodies(self, tag):
        """the body views handed out for `tag`, in request order"""
        return [raw[off:off + body] for t, _, raw, off, body in self._bufs if t == tag]

    def check_body_beyond(self, tag, used_bytes):
        """(after check()) the bytes of every `tag` body at or beyond `used_bytes` still hold the pattern: the call used no more than
        the plan of its direction says"""
        for t, nbytes, raw, off, body in self._bufs:
            if t == tag and used_bytes < body:
                self._pattern_holds(tag, f"the body beyond the plan's {used_bytes} bytes", raw, off + used_bytes, off + body, off)
