"""The stream ledger (plain helper module, no tests of its own): which launch went to which stream with which pointers, which order
edges exist between the streams, and when each allocator block was allocated and freed -- recorded exactly, then checked exactly.

A bit-equality test of a cross-stream switch passes whenever timing is kind.  The ordering protocol itself is host-side information
and deterministic, so this module records it (``Recorder``, on the GPU) and checks it (``check`` / ``verdict``, plain Python: the
checker half of this file imports neither the package nor torch, and the CPU tests feed it synthetic ledgers).

THE LEDGER is a list of dict events in ONE clock: the order of the caching allocator's own trace
(``torch.cuda.memory._record_memory_history`` / ``_snapshot()["device_traces"]``).  Everything the host side logs -- a launch, an
order edge, a ``record_stream`` -- takes a marker in that trace when it is logged: a ``torch.cuda.caching_allocator_alloc`` /
``_delete`` of 8 bytes on a marker stream used for nothing else, under one lock, so the i-th alloc on the marker stream IS host
event i and the marker pool disturbs no other stream's blocks.  No second clock (time stamps, Python call order against trace
order) is used anywhere.  Event kinds (``k``):

  alloc         addr, size, stream            free          addr, frame (free_requested: the block goes back to its stream's pool)
  free_done     addr (free_completed)         launch        seq, entry, stream, ptrs [[label, addr] ...], rows, ext, side
  wait_stream   stream, on                    record / wait_event / sync_event      ev (, stream)
  sync_stream   stream                        sync_device
  record_stream addr, stream                  autograd_in / autograd_out            addrs, stream
  backward_end  stream, streams

``ptrs`` holds every non-null device pointer of the call under a label: the parameter's name, ``param.field`` for the pointer
fields of a struct passed by reference (found by walking the ctypes ``_fields_``), ``param[].field`` for a host array of structs,
``grads_host[]`` for a host array of device pointers, and ``table[].p / .m / .v / .shadow`` for the optimizer's device-resident
table, whose tensors come from the host-side plan that built it.  ``rows`` / ``ext``: for xp_encoder_layer_fwd, XpLayerDims.rows
and per label (rows per unit, bytes per unit) from the layer plan's piece table, so that label's extent is rows // unit * bytes.

THE MODEL (``check``): vector clocks per stream -- a launch ticks its stream, an event carries a copy, a wait takes the maximum; a
host-side synchronisation raises a host clock that every later launch inherits.  Host-blocking reads (.item(), .cpu(), torch.equal)
are NOT modelled: that is the conservative side, and the runs put an explicit torch.cuda.synchronize() where they need one.
Edges nobody can observe from Python are held in ONE table, ``MODEL_EDGES``, each with its source.

  R1 lifetime   the allocator hands a freed block back at once, but only to its allocation stream: at ``free`` every launch that
                touched the block on ANOTHER stream must be ordered before the allocation stream's position at that moment, or the
                block carries a record_stream for that launch's stream.
  R2 order      every pair of launches on different streams that touch one block with no order either way, grouped into classes
                ((entry, label), (entry, label)); ``verdict`` holds the set of classes EQUAL to the committed ``CONCURRENT`` table and
                checks each reason: "both read" against the written labels of the C header, "disjoint halves" from the two calls'
                own pointers and extents.
  R3 unseen     every non-null pointer resolves to a live block (csrc/ allocates no device memory); a launch on a stream the
                ledger has never seen fails too.
"""
import bisect
import collections
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xpretrain_hip.h")

# ------------------------------------------------------------------------------------------------------------ the C header
_FIELD = re.compile(r"(const\s+)?(\w+)\b((?:\s*\*(?:\s*const\b)?)*)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?")
_PY_KEYWORDS = ("in",)                    # _lib.py gives a field named with a Python keyword a trailing underscore
DEVICE_TABLES = {"XpAdamTensor": ("p", "m", "v", "shadow")}      # arrays in device memory: operands from the host-side plan
DEVICE_STRUCTS = ("XpStepVerdict",)                               # a struct in device memory, passed by its device address


def _decl(text):
    m = _FIELD.fullmatch(text.strip())
    if not m:
        raise RuntimeError(f"stream_ledger: cannot read the declaration {text.strip()!r}")
    const, base, stars, name, n = m.groups()
    return bool(const), base, stars.count("*"), name + "_" * (name in _PY_KEYWORDS), int(n) if n else 0


def read_abi(text):
    """``(structs, entries)`` of the header: structs name -> [(field, const, base, stars, count)], entries name -> [(param, const,
    base, stars)] for every entry point whose last parameter is ``void* stream``"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for decl in m[1].split(";"):
            if not decl.strip():
                continue
            first, *more = decl.split(",")
            const, base, stars, name, n = _decl(first)
            fields.append((name, const, base, stars, n))
            for d in more:
                _, _, _, name2, n2 = _decl(base + " " + d.strip())
                fields.append((name2, const, base, stars, n2))
        structs[m[2]] = fields
    body = re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;|enum\s*\w*\s*\{[^{}]*\}\s*;|^\s*#.*$", " ", text, flags=re.M)
    entries = {}
    for m in re.finditer(r"\b(xp_\w+)\s*\(([^()]*)\)\s*;", body):
        params = [] if m[2].strip() == "void" else [_decl(p)[:4] for p in m[2].split(",")]
        params = [(name, const, base, stars) for const, base, stars, name in params]
        if params and params[-1][0] == "stream" and params[-1][2:] == ("void", 1):
            entries[m[1]] = params
    return structs, entries


def _struct_labels(structs, base, prefix):
    """(label, written) of every pointer field of struct ``base``; arrays of pointers are ``field[]``; *_host fields are skipped"""
    out = []
    for name, const, fbase, stars, n in structs[base]:
        if "host" in name:
            continue
        if stars:
            out.append((f"{prefix}.{name}" + ("[]" if n else ""), not const))
        elif fbase in structs:
            out += _struct_labels(structs, fbase, f"{prefix}.{name}")
    return out


def entry_labels(structs, entries, entry):
    """every label a launch record of ``entry`` can carry -> whether the header lets the kernel write through it (no ``const``)"""
    labels = {}
    for name, const, base, stars in entries[entry][:-1]:
        if not stars:
            continue
        host = "host" in name
        if base in DEVICE_TABLES:
            labels[name] = False
            labels.update({f"{name}[].{f}": True for f in DEVICE_TABLES[base]})
        elif base in DEVICE_STRUCTS:
            labels[name] = not const
        elif base in structs:
            labels.update(_struct_labels(structs, base, name + "[]" if host else name))
        elif stars == 2:
            labels[name + "[]"] = False             # const void* const*: a host array of device pointers that are read
        elif not host:
            labels[name] = not const
    return labels


with open(HEADER_PATH) as _f:
    STRUCTS, ENTRIES = read_abi(_f.read())
LABELS = {e: entry_labels(STRUCTS, ENTRIES, e) for e in ENTRIES}
WRITTEN = {e: frozenset(l for l, w in LABELS[e].items() if w) for e in ENTRIES}       # the per-entry table of written fields

# ------------------------------------------------------------------------------------------------------------ the two tables
# Order edges that exist but that no Python wrapper can observe, each with its source.  ``when``: a predicate over the launch
# record (its ``side`` field is set by the recorder exactly when the library's condition holds; the CPU tests hold the condition).
_WGRAD = dict(
    kind="side_stream",
    when="xp_side_stream() != NULL and the call's WgradOrder has a side: XpLayerDims.rows >= 4096 (dense: and XP_ATTN_PROXY)",
    mark="xpretrain_amd/csrc/layer.hip WgradOrder::mark: hipEventRecord(ev[i], main); hipStreamWaitEvent(side, ev[i]) -- the side "
         "stream is ordered behind everything the caller's stream has enqueued, in front of each weight-gradient GEMM",
    join="xpretrain_amd/csrc/layer.hip WgradOrder::join (finish_bwd): hipEventRecord(done, side); hipStreamWaitEvent(main, done) -- "
         "the caller's stream is ordered behind the side stream before the call returns")
MODEL_EDGES = {
    "xp_encoder_layer_bwd": dict(_WGRAD, where="csrc/layer.hip: xp_encoder_layer_bwd builds `const WgradOrder wg{...}`, wg.mark(0..3)"),
    "xp_encoder_layer_bwd_listed": dict(_WGRAD, where="csrc/layer.hip: the same body as xp_encoder_layer_bwd (dx3_support != NULL)"),
    "xp_encoder_layer_pooled_bwd": dict(_WGRAD, where="csrc/layer.hip: xp_encoder_layer_pooled_bwd builds `const WgradOrder wg{...}`"),
    "autograd_in": dict(
        kind="autograd",
        where="torch/csrc/autograd/input_buffer.cpp InputBuffer::add: a gradient consumed by a node on a stream other than its "
              "producer's -- the consumer stream waits for an event recorded on the producer stream behind the producing node, and "
              "the gradient's block is recorded on the consumer stream (c10 CachingAllocator recordStream).  Modelled from the "
              "producing node's own end (autograd_out of the same address) where it is a custom Function's, else from the "
              "producer stream's position when the block was allocated: never later than the real event"),
    "backward_end": dict(
        kind="autograd",
        where="torch/csrc/autograd/engine.cpp GraphTask::exec_post_processing: the stream that called backward() waits for every "
              "stream a node of the graph task ran on (leaf_streams), before backward() returns"),
}

_FWD = "xp_encoder_layer_fwd"
# the saved pieces of functional._LayerPlan, the [., D] streams and the fp32 side rows: what the two forward chains both address
# (labels that can share a block, group by group: the arena's pieces; a layer's x3 is the next layer's x; its side_out the next
# layer's side_in; side_x2 is a tensor of its own)
FWD_BLOCK_GROUPS = (("h1", "qkv", "attn_o", "x2", "h2", "pre", "act", "mean1", "rstd1", "mean2", "rstd2", "stats"), ("x", "x3"),
                    ("side_in", "side_out"), ("side_x2",))
FWD_PARAM_LABELS = tuple("args." + n for n in ("Wqkv", "Wo", "W1", "W2", "ln1_w", "ln1_b", "bqkv", "bo", "ln2_w", "ln2_b", "b1", "b2"))


def cls(a, b):
    """the class of an unordered pair of (entry, label) touches"""
    return tuple(sorted((tuple(a), tuple(b))))


BOTH_READ, DISJOINT = "both read", "disjoint halves"
# Every class of launch pairs on different streams that touch one allocator block with no order either way, with its reason.
# The video tower's forward as two half-batch chains (functional.ForwardSplit) is the one place where the step runs the same entry
# point on two streams over the same buffers: chain 0 on the caller's stream over rows [0, rows/2), chain 1 on the second stream over
# rows [rows/2, rows) of the SAME full-batch x, x3, arena and side rows (functional._layer_fwd_native).  Block granularity then pairs
# every row-proportional label of one chain with every one of the other (all pieces of a layer live in one arena block; a layer's
# x3 is the next layer's x and its side_out the next side_in): all of them are "disjoint halves", proved per pair from the two
# calls' pointers and XpLayerDims.rows x the piece's row bytes.  The weights and fp32 parameters are read by both chains.
CONCURRENT = {}
for _group in FWD_BLOCK_GROUPS:
    for _i, _a in enumerate(_group):
        for _b in _group[_i:]:
            CONCURRENT[cls((_FWD, "args." + _a), (_FWD, "args." + _b))] = DISJOINT
for _a in FWD_PARAM_LABELS:
    CONCURRENT[cls((_FWD, _a), (_FWD, _a))] = BOTH_READ


def applicable(split):
    """the part of CONCURRENT a run is held to -- equality, both ways: every class of the table comes from the two forward chains,
    so a run whose video tower splits must show all of it and any other run none"""
    return dict(CONCURRENT) if split else {}


# ------------------------------------------------------------------------------------------------------------ the checker
class _Block:
    __slots__ = ("addr", "size", "stream", "touches", "recorded", "born", "gen")

    def __init__(self, addr, size, stream, born, gen):
        self.addr, self.size, self.stream, self.born, self.gen = addr, size, stream, born, gen
        self.touches, self.recorded = [], set()


def _merge(into, other):
    for s, t in other.items():
        if into.get(s, 0) < t:
            into[s] = t


def check(events, initial_blocks=(), known_streams=(0,)):
    """Replay a ledger.  Returns a report dict: ``violations`` (R1), ``classes`` (R2: class -> count) with ``unproved`` (classes that
    have a pair whose extents are unknown or overlap), ``unresolved`` and ``unseen_streams`` (R3), and the counts."""
    clocks = collections.defaultdict(dict)        # stream -> vector clock {stream: tick}
    host = {}                                     # what the host has synchronised with
    event_clock, node_end = {}, {}
    seen = set(known_streams)
    starts, blocks, gen = [], {}, 0
    launches = {}
    rep = dict(violations=[], classes=collections.Counter(), unproved=set(), examples={}, unresolved=[], unseen_streams=[],
               n_launches=0, n_blocks=0, n_frees=0, streams=collections.Counter(), edges=collections.Counter())

    def now(s):
        c = clocks[s]
        _merge(c, host)
        return c

    def add_block(addr, size, stream):
        nonlocal gen
        gen += 1
        if addr in blocks:                        # (an alloc of an address whose free the trace did not hold)
            drop_block(addr)
        blocks[addr] = _Block(addr, size, stream, dict(now(stream)), gen)
        bisect.insort(starts, addr)
        rep["n_blocks"] += 1

    def drop_block(addr):
        del blocks[addr]
        starts.pop(bisect.bisect_left(starts, addr))

    def find(addr):
        i = bisect.bisect_right(starts, addr) - 1
        if i >= 0:
            b = blocks[starts[i]]
            if addr < b.addr + max(b.size, 1):
                return b
        return None

    def before(l, clock):
        return clock.get(l["stream_tick"][0], 0) >= l["stream_tick"][1]

    def extent(l, label):
        e = (l.get("ext") or {}).get(label)
        return None if e is None or l.get("rows") is None else l["rows"] // e[0] * e[1]

    for addr, size, stream in initial_blocks:
        add_block(addr, size, stream)
        seen.add(stream)
    for e in events:
        k = e["k"]
        rep["edges"][k] += 1
        if k == "alloc":
            seen.add(e["stream"])
            add_block(e["addr"], e["size"], e["stream"])
        elif k == "free":
            b = blocks.get(e["addr"])
            if b is None:
                continue
            rep["n_frees"] += 1
            here = now(b.stream)
            for l, label in b.touches:
                if l["stream"] != b.stream and l["stream"] not in b.recorded and not before(l, here):
                    mine = [(m["entry"], lab) for m, lab in b.touches if m["stream"] == b.stream]
                    rep["violations"].append(dict(
                        rule="R1", block=[b.addr, b.size], alloc_stream=b.stream, frame=e.get("frame"),
                        launch=dict(seq=l["seq"], entry=l["entry"], label=label, stream=l["stream"]),
                        last_on_alloc_stream=list(mine[-1]) if mine else None))
            drop_block(e["addr"])
        elif k == "free_done":
            pass
        elif k == "launch":
            s = e["stream"]
            if s not in seen:
                rep["unseen_streams"].append(dict(seq=e["seq"], entry=e["entry"], stream=s))
            rep["n_launches"] += 1
            rep["streams"][s] += 1
            side = e.get("side")
            c = now(s)
            parts = [(s, c)]
            if side is not None:                  # MODEL_EDGES: mark, the weight-gradient GEMMs on the side stream, join
                cs = now(side)
                seen.add(side)
                if e.get("mark", True):           # (``mark`` / ``join`` False: only a synthetic ledger with a seeded defect says so)
                    _merge(cs, c)
                parts.append((side, cs))
            for st, ck in parts:
                ck[st] = ck.get(st, 0) + 1
                l = dict(seq=e["seq"], entry=e["entry"], stream=st, stream_tick=(st, ck[st]), clock=dict(ck), rows=e.get("rows"),
                         ext=e.get("ext"), ptrs=e["ptrs"])
                launches[(e["seq"], st)] = l
                for label, addr in e["ptrs"]:
                    b = find(addr)
                    if b is None:
                        if st == s:
                            rep["unresolved"].append(dict(seq=e["seq"], entry=e["entry"], label=label, addr=addr))
                        continue
                    for m, mlabel in b.touches:
                        # (m came first in the ledger: it cannot be behind l; the two halves of ONE call are the library's own)
                        if m["stream"] != st and m["seq"] != e["seq"] and not before(m, ck):
                            key = cls((m["entry"], mlabel), (e["entry"], label))
                            rep["classes"][key] += 1
                            x0, x1 = extent(m, mlabel), extent(l, label)
                            a0 = dict(m["ptrs"]).get(mlabel) if x0 is not None else None
                            if x0 is None or x1 is None or not (a0 + x0 <= addr or addr + x1 <= a0):
                                rep["unproved"].add(key)
                            rep["examples"].setdefault(key, [m["seq"], e["seq"]])
                    b.touches.append((l, label))
            if side is not None and e.get("join", True):
                _merge(c, clocks[side])
        elif k == "wait_stream":
            seen.update((e["stream"], e["on"]))
            _merge(now(e["stream"]), now(e["on"]))
        elif k == "record":
            seen.add(e["stream"])
            event_clock[e["ev"]] = dict(now(e["stream"]))
        elif k == "wait_event":
            seen.add(e["stream"])
            _merge(now(e["stream"]), event_clock.get(e["ev"], {}))
        elif k == "sync_event":
            _merge(host, event_clock.get(e["ev"], {}))
        elif k == "sync_stream":
            seen.add(e["stream"])
            _merge(host, now(e["stream"]))
        elif k == "sync_device":
            for s in list(clocks):
                _merge(host, clocks[s])
        elif k == "record_stream":
            seen.add(e["stream"])
            b = find(e["addr"])
            if b is not None:
                b.recorded.add(e["stream"])
        elif k == "autograd_out":
            for addr in e["addrs"]:
                node_end[addr] = (e["stream"], dict(now(e["stream"])))
        elif k == "autograd_in":
            s = e["stream"]
            seen.add(s)
            for addr in e["addrs"]:
                b = find(addr)
                if b is None:
                    continue
                end = node_end.get(addr)
                if end is not None and end[0] != s:
                    _merge(now(s), end[1])
                if b.stream != s:
                    b.recorded.add(s)
                    if end is None:
                        _merge(now(s), b.born)
        elif k == "backward_end":
            for s in e["streams"]:
                _merge(now(e["stream"]), now(s))
        else:
            raise ValueError(f"stream_ledger: unknown ledger event {k!r}")
    return rep


def verdict(rep, concurrent=None, written=None):
    """What is wrong with a report, as a list of strings (empty: R1, R2 and R3 hold)."""
    concurrent = CONCURRENT if concurrent is None else concurrent
    written = WRITTEN if written is None else written
    bad = []
    for v in rep["violations"]:
        l = v["launch"]
        bad.append(f"R1: block {v['block'][0]:#x} of stream {v['alloc_stream']:#x} freed at {v['frame']} while launch #{l['seq']} "
                   f"{l['entry']}:{l['label']} on stream {l['stream']:#x} is unordered (last on the allocation stream: "
                   f"{v['last_on_alloc_stream']})")
    for key in sorted(set(rep["classes"]) - set(concurrent)):
        bad.append(f"R2: unlisted concurrent class {key} ({rep['classes'][key]} pairs, e.g. launches {rep['examples'][key]})")
    for key in sorted(set(concurrent) - set(rep["classes"])):
        bad.append(f"R2: listed class {key} never occurs")
    for key in sorted(set(concurrent) & set(rep["classes"])):
        reason = concurrent[key]
        if reason == BOTH_READ:
            w = [(e, l) for e, l in key if l in written.get(e, ())]
            if w:
                bad.append(f"R2: class {key} is listed as {BOTH_READ!r} but {w} is written")
        elif reason == DISJOINT:
            if key in rep["unproved"]:
                bad.append(f"R2: class {key} is listed as {DISJOINT!r} but a pair's extents overlap or are unknown")
        else:
            bad.append(f"R2: class {key} has a reason no check exists for: {reason!r}")
    for u in rep["unresolved"]:
        bad.append(f"R3: launch #{u['seq']} {u['entry']}:{u['label']} = {u['addr']:#x} lies in no live block")
    for u in rep["unseen_streams"]:
        bad.append(f"R3: launch #{u['seq']} {u['entry']} on stream {u['stream']:#x}, which the ledger has never seen")
    return bad


def summary(rep):
    """the JSON-able summary of a report (gpu_util.dump)"""
    return dict(streams={hex(s): n for s, n in rep["streams"].items()}, launches=rep["n_launches"], blocks=rep["n_blocks"],
                frees=rep["n_frees"], events=dict(rep["edges"]),
                concurrent_classes=[[list(a), list(b), n] for (a, b), n in sorted(rep["classes"].items())],
                unproved=[[list(a), list(b)] for a, b in sorted(rep["unproved"])],
                violations=rep["violations"], unresolved=rep["unresolved"], unseen_streams=rep["unseen_streams"])


# ------------------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    """Records one run's ledger on the GPU; test-only, nothing in the package knows of it.

    ``start()`` switches the allocator's history on (do it BEFORE the model is built, so that every block the run touches is either
    in the trace or in the snapshot taken at that moment), installs a proxy as ``xpretrain_amd._lib._lib`` -- ``L.lib()`` then returns
    it, and every entry point of ``ENTRIES`` is logged with its stream and pointers before it is called -- and wraps the Python
    stream API: Stream.wait_stream / wait_event / record_event / synchronize / query, Event.record / wait / synchronize / query,
    torch.cuda.synchronize, Tensor.record_stream, and for the two autograd edges of MODEL_EDGES Tensor.backward and
    autograd.function.BackwardCFunction.apply.  (A query() that returns True is a synchronisation the host has observed.)  Only the
    outermost wrapped call logs: wait_stream is one edge, not the event it is made of.  ``stop()`` removes all of it and returns
    ``(events, initial_blocks)`` for ``check``; ``self.sources`` says which allocator events the trace held."""

    def __init__(self):
        import threading
        self.host, self.optimizers, self.sources = [], [], {}
        self._lock, self._tl = threading.RLock(), threading.local()
        self._undo, self._node_streams, self._in_backward = [], set(), 0
        self._side = None

    def watch(self, optimizer):
        """the optimizer whose plan names the tensors behind its device-resident tables"""
        self.optimizers.append(optimizer)

    # ---- logging: the event, then its marker in the allocator's trace
    def _log(self, ev):
        import torch
        with self._lock:
            if ev["k"] == "launch":
                ev["seq"] = len(self.host)
            self.host.append(ev)
            torch.cuda.caching_allocator_delete(torch.cuda.caching_allocator_alloc(8, self.device, self.marker))

    @staticmethod
    def _cur():
        import torch
        return torch.cuda.current_stream().cuda_stream

    def _patch(self, owner, name, make_event):
        """wrap owner.name: after the real call, the outermost wrapped call logs make_event(result, *args, **kwargs) if not None"""
        had = name in vars(owner)
        real = getattr(owner, name)
        tl, rec = self._tl, self

        def wrapper(*a, **kw):
            depth = getattr(tl, "depth", 0)
            tl.depth = depth + 1
            try:
                out = real(*a, **kw)
            finally:
                tl.depth = depth
            if depth == 0:
                ev = make_event(out, *a, **kw)
                if ev is not None:
                    rec._log(ev)
            return out
        setattr(owner, name, wrapper)
        self._undo.append((owner, name, real, had))

    def start(self):
        import torch
        import torch.autograd.function as AF
        from xpretrain_amd import _lib as L
        torch.cuda.synchronize()
        self.device = torch.cuda.current_device()
        self.marker_stream = torch.cuda.Stream()
        self.marker = self.marker_stream.cuda_stream
        torch.cuda.memory._record_memory_history(enabled="all", context="all", stacks="python", clear_history=True)
        self.initial_blocks = []
        for seg in torch.cuda.memory._snapshot()["segments"]:
            if seg.get("device", self.device) != self.device:
                continue
            at = seg["address"]
            for b in seg["blocks"]:
                addr = b.get("address", at)
                at = addr + b["size"]
                if b["state"] != "inactive":
                    self.initial_blocks.append((addr, b["size"], seg["stream"]))
        S, E, cur = torch.cuda.Stream, torch.cuda.Event, self._cur
        h = lambda st: cur() if st is None else st.cuda_stream
        self._patch(S, "wait_stream", lambda out, self_, other: dict(k="wait_stream", stream=self_.cuda_stream, on=other.cuda_stream))
        self._patch(S, "wait_event", lambda out, self_, ev: dict(k="wait_event", ev=id(ev), stream=self_.cuda_stream))
        self._patch(S, "record_event", lambda out, self_, event=None: dict(k="record", ev=id(out), stream=self_.cuda_stream))
        self._patch(S, "synchronize", lambda out, self_: dict(k="sync_stream", stream=self_.cuda_stream))
        self._patch(S, "query", lambda out, self_: dict(k="sync_stream", stream=self_.cuda_stream) if out else None)
        self._patch(E, "record", lambda out, self_, stream=None: dict(k="record", ev=id(self_), stream=h(stream)))
        self._patch(E, "wait", lambda out, self_, stream=None: dict(k="wait_event", ev=id(self_), stream=h(stream)))
        self._patch(E, "synchronize", lambda out, self_: dict(k="sync_event", ev=id(self_)))
        self._patch(E, "query", lambda out, self_: dict(k="sync_event", ev=id(self_)) if out else None)
        self._patch(torch.cuda, "synchronize", lambda out, *a, **kw: dict(k="sync_device"))
        self._patch(torch.Tensor, "record_stream",
                    lambda out, self_, stream: dict(k="record_stream", addr=self_.data_ptr(), stream=stream.cuda_stream))
        # the two autograd edges of MODEL_EDGES
        rec, real_apply, real_backward = self, AF.BackwardCFunction.apply, torch.Tensor.backward
        addrs = lambda ts: [t.data_ptr() for t in ts if isinstance(t, torch.Tensor) and t.is_cuda and t.numel()]

        def apply(ctx, *grads):
            s = cur()
            rec._node_streams.add(s)
            rec._log(dict(k="autograd_in", addrs=addrs(grads), stream=s))
            out = real_apply(ctx, *grads)
            rec._log(dict(k="autograd_out", addrs=addrs(out if isinstance(out, tuple) else (out,)), stream=cur()))
            return out

        def backward(t, *a, **kw):
            outer = rec._in_backward == 0
            if outer:
                rec._node_streams = set()
            rec._in_backward += 1
            try:
                return real_backward(t, *a, **kw)
            finally:
                rec._in_backward -= 1
                if outer:
                    rec._log(dict(k="backward_end", stream=cur(), streams=sorted(rec._node_streams)))
        AF.BackwardCFunction.apply = apply
        self._undo.append((AF.BackwardCFunction, "apply", real_apply, True))
        torch.Tensor.backward = backward
        self._undo.append((torch.Tensor, "backward", real_backward, True))
        # the launches
        self._L, self._real = L, L.lib()
        self._saved_lib = L._lib
        L._lib = _LibProxy(self, self._real)
        return self

    def stop(self):
        import torch
        self._L._lib = self._saved_lib
        for owner, name, real, had in reversed(self._undo):
            if had:
                setattr(owner, name, real)
            else:
                delattr(owner, name)
        self._undo = []
        trace = torch.cuda.memory._snapshot()["device_traces"][self.device]
        torch.cuda.memory._record_memory_history(enabled=None)
        actions = collections.Counter(te["action"] for te in trace)
        # ONE source for a block's end: free_requested where the build reports it, else free_completed
        free_action = "free_requested" if actions["free_requested"] else "free_completed"
        self.sources = dict(actions=dict(actions), free_from=free_action, clock="marker allocations on stream %#x" % self.marker)
        events, i = [], 0
        for te in trace:
            a = te["action"]
            if te.get("stream") == self.marker:
                if a == "alloc":
                    if i >= len(self.host):
                        raise RuntimeError("stream_ledger: more markers in the allocator's trace than host events")
                    events.append(self.host[i])
                    i += 1
                continue
            if a == "alloc":
                events.append(dict(k="alloc", addr=te["addr"], size=te["size"], stream=te["stream"]))
            elif a == free_action:
                events.append(dict(k="free", addr=te["addr"], frame=_frame(te.get("frames"))))
            elif a == "free_completed":
                events.append(dict(k="free_done", addr=te["addr"]))
        if i != len(self.host):
            raise RuntimeError(f"stream_ledger: {len(self.host)} host events but {i} markers in the allocator's trace")
        return events, self.initial_blocks

    # ---- one launch record
    def _launch(self, entry, args):
        import ctypes as C
        params = ENTRIES[entry]
        if len(args) != len(params):
            raise TypeError(f"stream_ledger: {entry} takes {len(params)} arguments, got {len(args)}")
        by_name = {p[0]: v for p, v in zip(params, args)}
        ptrs, ev = [], dict(k="launch", seq=None, entry=entry, rows=None, ext=None, side=None)

        def addr(v):
            if v is None:
                return 0
            if isinstance(v, int):
                return v
            if isinstance(v, C.c_void_p):
                return v.value or 0
            if isinstance(v, C._Pointer):
                return C.cast(v, C.c_void_p).value or 0
            if hasattr(v, "_obj"):
                return C.addressof(v._obj)
            raise TypeError(f"stream_ledger: {entry}: cannot read the pointer argument {v!r}")

        def add(label, a):
            if a:
                ptrs.append([label, int(a)])

        def walk(obj, prefix):
            for fname, ftype in obj._fields_:
                if "host" in fname:
                    continue
                val = getattr(obj, fname)
                if ftype is C.c_void_p:
                    add(f"{prefix}.{fname}", val)
                elif isinstance(ftype, type) and issubclass(ftype, C.Structure):
                    walk(val, f"{prefix}.{fname}")
                elif isinstance(ftype, type) and issubclass(ftype, C.Array) and ftype._type_ is C.c_void_p:
                    for x in val:
                        add(f"{prefix}.{fname}[]", x)

        def count_of(i):
            n = args[i + 1]
            return int(getattr(n, "value", n))

        for i, ((name, const, base, stars), v) in enumerate(zip(params, args)):
            if not stars:
                continue
            host = "host" in name
            if i == len(params) - 1:
                ev["stream"] = addr(v)
            elif base in DEVICE_TABLES:
                add(name, addr(v))
                ptrs.extend(self._table_operands(name, addr(v)))
            elif base in DEVICE_STRUCTS:
                add(name, addr(v))
            elif base in STRUCTS:
                obj = getattr(v, "_obj", None) if not isinstance(v, (C.Array, C.Structure)) else v
                if obj is None and isinstance(v, C._Pointer) and v:
                    obj = v.contents
                if obj is None:
                    continue
                if host:
                    elems = [obj[j] for j in range(count_of(i))] if isinstance(obj, C.Array) else [obj]
                    for el in elems:
                        walk(el, name + "[]")
                else:
                    walk(obj, name)
                    if entry == _FWD:
                        ev["rows"], ev["ext"] = int(obj.dims.rows), self._fwd_extents(obj)
                    if MODEL_EDGES.get(entry, {}).get("kind") == "side_stream":
                        ev["side"] = self._side_stream(entry, obj)
            elif stars == 2:
                n = by_name.get("n_tensors")
                for j in range(int(getattr(n, "value", n))):
                    add(name + "[]", v[j])
            elif not host:
                add(name, addr(v))
        ev["ptrs"] = ptrs
        return ev

    def _table_operands(self, name, table_addr):
        from xpretrain_amd import functional as XF
        for opt in self.optimizers:
            plan = opt._plan
            for la in (plan["launches"] if plan else ()):
                if la["table"].data_ptr() == table_addr:
                    shadows, _ = XF.WEIGHTS.shadow_bindings([p for l2 in plan["launches"] for _, p, _ in l2["part"]])
                    sm, sv = opt._STATE
                    out = []
                    for _, p, st in la["part"]:
                        out += [[f"{name}[].p", p.data_ptr()], [f"{name}[].m", st[sm].data_ptr()], [f"{name}[].v", st[sv].data_ptr()]]
                        if id(p) in shadows:
                            out.append([f"{name}[].shadow", shadows[id(p)][0]])
                    return out
        return [[f"{name}[] (no watched optimizer's plan built this table)", 1]]       # resolves to no block: R3 reports it

    def _fwd_extents(self, a):
        from xpretrain_amd import functional as XF
        for plan in XF._PLANS.values():
            if bytes(plan.dims) == bytes(a.dims) and any(n == "qkv" for n, _, _ in plan.fill):
                ext = {f"args.{n}": [1, bpr] for n, _, bpr in plan.fill}
                ext.update({"args.x": [1, plan.rD], "args.x3": [1, plan.rD]})
                ext.update({f"args.{n}": [plan.side_S, plan.side_M * plan.side_row] for n in ("side_in", "side_out", "side_x2")})
                return ext
        return None

    def _side_stream(self, entry, a):
        """the library's side stream where MODEL_EDGES' condition holds for this call, else None"""
        pooled = "pooled" in entry
        if a.dims.rows < 4096 or (not pooled and a.dims.attn_mode != self._L.XP_ATTN_PROXY):
            return None
        if self._side is None:
            self._side = self._real.xp_side_stream() or 0
        return self._side or None


class _LibProxy:
    """stands in for the loaded library: an entry point of ENTRIES logs its launch record, then calls the real one"""

    def __init__(self, rec, real):
        self.__dict__.update(_rec=rec, _real=real)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ENTRIES:
            return fn
        rec = self._rec

        def call(*args):
            rec._log(rec._launch(name, args))
            return fn(*args)
        self.__dict__[name] = call
        return call


def _frame(frames):
    """the innermost Python frame of the project (else the innermost of all) as 'file:line name'"""
    frames = [f for f in (frames or ()) if str(f.get("filename", "")).endswith(".py")]
    own = [f for f in frames if "xpretrain_amd" in f["filename"] or os.sep + "tests" + os.sep in f["filename"]]
    f = (own or frames or [None])[0]
    return None if f is None else f"{os.path.basename(f['filename'])}:{f['line']} {f['name']}"
