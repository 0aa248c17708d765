"""CPU: the checker of tests/stream_ledger.py on synthetic ledgers -- the clean protocols give no report, every seeded defect is
reported with the right pair named -- and its committed tables name only entry points and fields of the C ABI."""
import os

import pytest

from tests import stream_ledger as SL

MAIN, SECOND, WGRAD, LATE, UNSEEN = 0, 0x20, 0x30, 0x40, 0x99
FWD, BWD, ADAMW = "xp_encoder_layer_fwd", "xp_encoder_layer_bwd", "xp_adamw_step"
# the tiny video layer of tests/step_matrix.py: 64 rows of D = 128, Dff = 256, 2 heads, M = 4 of S = 16 rows of a sample are side rows
ROWS, D, DFF, HEADS, S_, M_ = 64, 128, 256, 2, 16, 4
PIECES = (("h1", 2 * D), ("qkv", 6 * D), ("attn_o", 2 * D), ("x2", 2 * D), ("h2", 2 * D), ("pre", 2 * DFF), ("act", 2 * DFF), ("mean1", 4),
          ("rstd1", 4), ("mean2", 4), ("rstd2", 4), ("stats", HEADS * 8))          # functional._LayerPlan's piece table: bytes per row
PARAMS = ("Wqkv", "Wo", "W1", "W2", "ln1_w", "ln1_b", "bqkv", "bo", "ln2_w", "ln2_b", "b1", "b2")


class Ledger:
    """a synthetic ledger, written in program order"""

    def __init__(self):
        self.events, self.next = [], 0x10000

    def alloc(self, size, stream=MAIN):
        addr, self.next = self.next, self.next + ((size + 511) & ~511) + 512
        self.events.append(dict(k="alloc", addr=addr, size=size, stream=stream))
        return addr

    def free(self, addr, frame="step.py:1 run"):
        self.events.append(dict(k="free", addr=addr, frame=frame))

    def launch(self, entry, stream, ptrs, **more):
        seq = len(self.events)
        self.events.append(dict(k="launch", seq=seq, entry=entry, stream=stream, ptrs=[[l, a] for l, a in ptrs.items()], **more))
        return seq

    def edge(self, k, **fields):
        self.events.append(dict(k=k, **fields))


def _layer_buffers(led):
    arena_off, o = {}, 0
    for name, bpr in PIECES:
        arena_off[name] = o
        o += (ROWS * bpr + 255) & ~255
    return dict(arena=led.alloc(o), off=arena_off, x3=led.alloc(ROWS * 2 * D), side_out=led.alloc(ROWS // S_ * M_ * 4 * D),
                side_x2=led.alloc(ROWS // S_ * M_ * 4 * D))


def _fwd(led, stream, r0, rows, x, side_in, buf, weights, ws):
    """one chain's xp_encoder_layer_fwd over rows [r0, r0 + rows), addressed as functional._layer_args / _side_args do"""
    ptrs = {"args." + n: a for n, a in weights.items()}
    ext = {"args.x": [1, 2 * D], "args.x3": [1, 2 * D]}
    for name, bpr in PIECES:
        ptrs["args." + name] = buf["arena"] + buf["off"][name] + r0 * bpr
        ext["args." + name] = [1, bpr]
    ptrs["args.x"], ptrs["args.x3"] = x + r0 * 2 * D, buf["x3"] + r0 * 2 * D
    side0 = r0 // S_ * M_ * 4 * D
    for n, a in (("side_in", side_in), ("side_out", buf["side_out"]), ("side_x2", buf["side_x2"])):
        ptrs["args." + n], ext["args." + n] = a + side0, [S_, M_ * 4 * D]
    ptrs["args.workspace"] = ws
    return led.launch(FWD, stream, ptrs, rows=rows, ext=ext)


def two_chain_forward(free_early=False, shared_workspace=False, layers=2):
    """ForwardSplit: fork, ``layers`` layer calls per chain over the halves of the same buffers, join, then the buffers go"""
    led = Ledger()
    x, side = led.alloc(ROWS * 2 * D), led.alloc(ROWS // S_ * M_ * 4 * D)
    ws = {MAIN: led.alloc(1 << 20), SECOND: led.alloc(1 << 20)}
    if shared_workspace:
        ws[SECOND] = ws[MAIN]
    led.edge("wait_stream", stream=SECOND, on=MAIN)
    held, seqs = [x, side], []
    for _ in range(layers):
        weights = {n: led.alloc(4096) for n in PARAMS}
        buf = _layer_buffers(led)
        for stream, r0 in ((MAIN, 0), (SECOND, ROWS // 2)):
            seqs.append(_fwd(led, stream, r0, ROWS // 2, x, side, buf, weights, ws[stream]))
        if free_early and len(held) == 2:
            led.free(x, "functional.py:1 forward")         # the first layer's input dies when the next layer returns: no hold()
        x, side = buf["x3"], buf["side_out"]
        held += [buf["arena"], buf["x3"], buf["side_out"], buf["side_x2"]]
    led.edge("wait_stream", stream=MAIN, on=SECOND)
    for a in held[1 if free_early else 0:]:
        led.free(a)
    return led, seqs


def late_update(record=True, wait_on=(MAIN, SECOND)):
    """multi_tensor.step with a late launch on a stream of its own, zero_grad(set_to_none=True), then the next forward's layer K as
    two chains, each of which waits for the update's event"""
    led = Ledger()
    p, m, v, shadow, grad, table, cmap = (led.alloc(4096) for _ in range(7))
    led.edge("wait_stream", stream=LATE, on=MAIN)
    if record:
        led.edge("record_stream", addr=grad, stream=LATE)
    late = led.launch(ADAMW, LATE, {"table": table, "chunk_map": cmap, "grads_host[]": grad, "table[].p": p, "table[].m": m,
                                    "table[].v": v, "table[].shadow": shadow})
    led.edge("record", ev=1, stream=LATE)
    led.free(grad, "optimizer.py:1 zero_grad")
    led.edge("wait_stream", stream=SECOND, on=MAIN)
    for st in wait_on:
        led.edge("wait_event", ev=1, stream=st)
    weights = {n: led.alloc(4096) for n in PARAMS if n != "Wqkv"}
    weights["Wqkv"] = shadow                                # the compute-dtype copy the late launch rewrites
    x, side, buf = led.alloc(ROWS * 2 * D), led.alloc(ROWS // S_ * M_ * 4 * D), _layer_buffers(led)
    ws = {MAIN: led.alloc(1 << 20), SECOND: led.alloc(1 << 20)}
    seqs = [_fwd(led, st, r0, ROWS // 2, x, side, buf, weights, ws[st]) for st, r0 in ((MAIN, 0), (SECOND, ROWS // 2))]
    led.edge("wait_stream", stream=MAIN, on=SECOND)
    return led, late, seqs


def side_stream_backward(join=True):
    """two native layer backwards whose weight-gradient GEMMs run on the library's stream, sharing the caller's workspace; then the
    workspace goes back to the allocator"""
    led = Ledger()
    ws, dx, dw = led.alloc(1 << 20), led.alloc(ROWS * 2 * D), led.alloc(4096)
    seqs = [led.launch(BWD, MAIN, {"args.workspace": ws, "args.dx": dx, "args.dwqkv": dw}, side=WGRAD, **({} if join else {"join": False}))
            for _ in range(2)]
    led.free(ws, "hip_ops.py:1 workspace")
    return led, seqs


def _classes(rep):
    return set(rep["classes"])


def _unproved(rep):
    """among the classes listed as disjoint halves (a class of reads needs no extents)"""
    return {k for k in rep["unproved"] if SL.CONCURRENT.get(k) == SL.DISJOINT}


def test_clean_two_chain_layer_late_update_and_side_stream_backward_give_no_report():
    led, _ = two_chain_forward()
    rep = SL.check(led.events)
    assert SL.verdict(rep) == [] and _classes(rep) == set(SL.CONCURRENT) and not _unproved(rep)
    assert rep["n_launches"] == 4 and rep["streams"] == {MAIN: 2, SECOND: 2}
    for led in (late_update()[0], side_stream_backward()[0]):
        rep = SL.check(led.events)
        only_chains = {k: r for k, r in SL.CONCURRENT.items() if k in rep["classes"]}
        assert SL.verdict(rep, concurrent=only_chains) == [] and not rep["violations"] and not rep["unresolved"]
    assert not SL.check(side_stream_backward()[0].events)["classes"]
    # a listed class that never occurs is a failure too; a run without the two chains is held to the part of the table that applies
    rep = SL.check(side_stream_backward()[0].events)
    assert len(SL.verdict(rep)) == len(SL.CONCURRENT) and SL.verdict(rep, concurrent=SL.applicable(split=False)) == []
    assert SL.applicable(split=True) == SL.CONCURRENT and SL.applicable(split=False) == {}


def test_a_buffer_freed_on_the_callers_stream_while_the_second_chain_is_unordered_is_r1():
    led, seqs = two_chain_forward(free_early=True)
    rep = SL.check(led.events)
    assert [(v["launch"]["seq"], v["launch"]["entry"], v["launch"]["label"], v["launch"]["stream"]) for v in rep["violations"]] == \
        [(seqs[1], FWD, "args.x", SECOND)]
    v = rep["violations"][0]
    assert v["alloc_stream"] == MAIN and v["frame"] == "functional.py:1 forward" and v["last_on_alloc_stream"] == [FWD, "args.x"]
    assert any(line.startswith("R1:") and "args.x" in line for line in SL.verdict(rep))


def test_a_late_launch_without_record_stream_on_a_freed_gradient_is_r1():
    led, late, _ = late_update(record=False)
    rep = SL.check(led.events)
    assert [(v["launch"]["seq"], v["launch"]["entry"], v["launch"]["label"], v["frame"]) for v in rep["violations"]] == \
        [(late, ADAMW, "grads_host[]", "optimizer.py:1 zero_grad")]


def test_a_dropped_wait_in_front_of_layer_k_on_the_second_chain_only_is_r2():
    led, late, seqs = late_update(wait_on=(MAIN,))
    rep = SL.check(led.events)
    key = SL.cls((ADAMW, "table[].shadow"), (FWD, "args.Wqkv"))
    assert _classes(rep) - set(SL.CONCURRENT) == {key} and rep["classes"][key] == 1
    assert rep["examples"][key] == [late, seqs[1]]          # the late launch and the SECOND chain's layer call; the first chain waited
    assert any(line.startswith("R2: unlisted") and "table[].shadow" in line for line in SL.verdict(rep))
    # (dropped on both chains: both layer calls pair with the late launch)
    rep = SL.check(late_update(wait_on=())[0].events)
    assert rep["classes"][key] == 2


def test_a_workspace_shared_by_two_streams_is_r2():
    led, seqs = two_chain_forward(shared_workspace=True, layers=1)
    rep = SL.check(led.events)
    key = SL.cls((FWD, "args.workspace"), (FWD, "args.workspace"))
    assert _classes(rep) - set(SL.CONCURRENT) == {key} and rep["examples"][key] == seqs
    assert key in rep["unproved"]                           # (no extent: a workspace is not row-proportional)


def test_a_removed_join_edge_is_reported():
    led, seqs = side_stream_backward(join=False)
    rep = SL.check(led.events)
    # the next call on the caller's stream touches the workspace the side stream may still read, and the free is unordered too
    key = SL.cls((BWD, "args.workspace"), (BWD, "args.workspace"))
    assert key in rep["classes"] and rep["examples"][key] == seqs
    assert [(v["launch"]["seq"], v["launch"]["stream"], v["launch"]["label"]) for v in rep["violations"]] == \
        [(seqs[0], WGRAD, "args.workspace"), (seqs[1], WGRAD, "args.workspace")]


def test_overlapping_halves_are_not_proved_disjoint():
    led, _ = two_chain_forward(layers=1)
    for e in led.events:
        if e["k"] == "launch" and e["stream"] == SECOND:
            e["ptrs"] = [[l, a - 2 * D if l == "args.x3" else a] for l, a in e["ptrs"]]       # one row too low
    rep = SL.check(led.events)
    key = SL.cls((FWD, "args.x3"), (FWD, "args.x3"))
    assert _unproved(rep) == {key}
    assert any("extents overlap" in line for line in SL.verdict(rep))


def test_a_written_field_cannot_be_listed_as_both_read():
    led, _ = two_chain_forward()
    rep = SL.check(led.events)
    key = SL.cls((FWD, "args.x3"), (FWD, "args.x3"))
    assert any("is written" in line for line in SL.verdict(rep, concurrent={**SL.CONCURRENT, key: SL.BOTH_READ}))
    assert any("no check exists" in line for line in SL.verdict(rep, concurrent={**SL.CONCURRENT, key: "trust me"}))


def test_r3_a_pointer_into_no_block_a_freed_block_and_an_unseen_stream():
    led = Ledger()
    a = led.alloc(4096)
    led.launch("xp_cast", MAIN, {"src": a, "dst": a + 8192})
    led.free(a)
    led.launch("xp_cast", MAIN, {"src": a})
    led.launch("xp_cast", UNSEEN, {})
    rep = SL.check(led.events)
    assert [(u["label"], u["addr"]) for u in rep["unresolved"]] == [("dst", a + 8192), ("src", a)]
    assert [u["stream"] for u in rep["unseen_streams"]] == [UNSEEN]
    assert sum(line.startswith("R3:") for line in SL.verdict(rep, concurrent={})) == 3
    # a block from before the recording began resolves, and a host-side synchronisation orders everything behind it
    led = Ledger()
    led.launch("xp_cast", SECOND, {"src": 0x5000})
    led.edge("sync_device")
    led.launch("xp_cast", MAIN, {"dst": 0x5000})
    rep = SL.check(led.events, initial_blocks=[(0x5000, 512, MAIN)], known_streams=(MAIN, SECOND))
    assert SL.verdict(rep, concurrent={}) == []


def test_the_autograd_edges_order_a_consumer_behind_its_producer_and_the_caller_behind_the_graph():
    def run(with_edges):
        led = Ledger()
        g, dx = led.alloc(4096), led.alloc(4096, SECOND)
        led.launch("xp_contrastive_loss", MAIN, {"d_txt": g})
        if with_edges:
            led.edge("autograd_out", addrs=[g], stream=MAIN)
            led.edge("autograd_in", addrs=[g], stream=SECOND)
        led.launch("xp_l2norm_bwd", SECOND, {"dy": g, "dx": dx})
        led.free(g, "autograd")
        if with_edges:
            led.edge("backward_end", stream=MAIN, streams=[MAIN, SECOND])
        led.launch(ADAMW, MAIN, {"grads_host[]": dx})
        return SL.check(led.events, known_streams=(MAIN, SECOND))
    rep = run(True)
    assert SL.verdict(rep, concurrent={}) == []
    rep = run(False)
    assert len(rep["violations"]) == 1 and len(rep["classes"]) == 2


def test_the_tables_name_only_entry_points_and_fields_of_the_abi():
    from xpretrain_amd import _lib as L
    import ctypes as C
    with_stream = {n for n, (_, args) in L.SIGNATURES.items() if args and args[-1] is C.c_void_p}
    assert set(SL.ENTRIES) <= with_stream and len(SL.ENTRIES) > 50
    for n, params in SL.ENTRIES.items():
        assert len(params) == len(L.SIGNATURES[n][1]) and params[-1][0] == "stream", n
        for (name, const, base, stars), ctype in zip(params, L.SIGNATURES[n][1]):
            assert bool(stars) == (ctype is C.c_void_p or hasattr(ctype, "contents")), (n, name)
    # every other signature ends in something that is not a stream
    text = open(SL.HEADER_PATH).read()
    for n in with_stream - set(SL.ENTRIES):
        assert not text[text.index(n + "("):].split(")", 1)[0].rstrip().endswith("stream"), n
    # the struct labels are the ctypes fields
    for struct, fields in SL.STRUCTS.items():
        assert [f[0] for f in fields] == [f[0] for f in getattr(L, struct)._fields_], struct
    assert set(SL.DEVICE_TABLES) == set(L._DEVICE_TABLES) and all(s in SL.STRUCTS for s in SL.DEVICE_STRUCTS)
    for key, reason in SL.CONCURRENT.items():
        assert key == SL.cls(*key) and reason in (SL.BOTH_READ, SL.DISJOINT)
        for entry, label in key:
            assert entry in SL.ENTRIES and label in SL.LABELS[entry], (entry, label)
            assert (label in SL.WRITTEN[entry]) <= (reason == SL.DISJOINT), (entry, label)
    # what the header's const says about the layer forward is what the kernels do: inputs and parameters read, the rest written
    assert SL.WRITTEN[FWD] == {"args." + n for n in [p[0] for p in PIECES] + ["x3", "side_out", "side_x2", "workspace"]}
    assert not any(SL.LABELS[FWD]["args." + n] for n in PARAMS + ("x", "side_in", "pad_mask"))
    assert SL.WRITTEN[ADAMW] == {"table[].p", "table[].m", "table[].v", "table[].shadow", "grad_norm_out"}
    # the edge table: the three backward entry points, each with the lines of csrc/layer.hip it stands for; the autograd edges
    layer = open(os.path.join(os.path.dirname(SL.HEADER_PATH), "..", "xpretrain_amd", "csrc", "layer.hip")).read()
    side = {n for n, e in SL.MODEL_EDGES.items() if e["kind"] == "side_stream"}
    assert side == {"xp_encoder_layer_bwd", "xp_encoder_layer_bwd_listed", "xp_encoder_layer_pooled_bwd"} <= set(SL.ENTRIES)
    for n in side:
        assert all(SL.MODEL_EDGES[n][k] for k in ("when", "where", "mark", "join"))
    for text in ("struct WgradOrder", "int mark(int i) const", "int join() const", "hipStreamWaitEvent(side->side, side->ev[i], 0)",
                 "hipStreamWaitEvent(main, side->done, 0)", "rows >= 4096", "return wg.join();"):
        assert text in layer, text
    assert {n for n, e in SL.MODEL_EDGES.items() if e["kind"] == "autograd"} == {"autograd_in", "backward_end"}


@pytest.mark.parametrize("text, want", [
    ("int xp_a(const float* x, float* y, int64_t n, void* stream);", {"x": False, "y": True}),
    ("typedef struct { const void* in; void* out; const int32_t* t[3]; const int32_t* t_host; } XpS;\n"
     "int xp_b(const XpS* a, const XpS* list_host, int32_t n, const void* const* grads_host, int32_t n_tensors, void* stream);\n"
     "size_t xp_b_bytes(const XpS* a);",
     {"a.in_": False, "a.out": True, "a.t[]": False, "list_host[].in_": False, "list_host[].out": True, "list_host[].t[]": False,
      "grads_host[]": False}),
])
def test_the_header_reader(text, want):
    structs, entries = SL.read_abi(text)
    assert len(entries) == 1
    (name,) = entries
    assert SL.entry_labels(structs, entries, name) == want
