"""CPU: the pointer-alignment rule of the C ABI (include/xpretrain_hip.h, "Pointer alignment"), held from four sides without a GPU:

  completeness   every pointer-typed parameter of every bound entry, and every pointer field of every ABI struct, is a row of
                 tests/alignment_cases.py or is listed there as exempt; no row names a pointer that does not exist
  refusals       every ``need N`` row: the entry, called with otherwise valid arguments and the operand one element (and, for N = 16,
                 8 bytes) off an aligned synthetic address, returns XP_ERR_ARG and names entry, operand and N.  Nothing is
                 dereferenced: the refusal comes before the first HIP call.  The same call with every operand aligned gets past
                 the argument checks (it ends in XP_ERR_LAUNCH on a machine without a device), so a missing check shows as that
                 other error, not as a pass
  header         the ``align[entry]`` comments of the header state what the table states
  gradient sinks functional._claim_sink declines a sink that is not 16-byte aligned (a reducer bucket with the one-element
                 logit_scale in front of the layer groups) and the pack-copy path gives the same gradients

The calls with synthetic addresses are made only where there is no device (with one, an accepted call would launch on them);
tests/test_alignment_gpu.py makes the refusals over real buffers."""
import ctypes as C
import os
import socket

import pytest
import torch

from tests import alignment_cases as A
from xpretrain_amd import _lib as L

PROTOS, STRUCTS = A.prototypes(), A.struct_fields()
NEED_ROWS = A.need_rows()
BASE = 0x7000_0000_0000          # synthetic device addresses: 16 MiB apart, 4096-byte aligned


def _is_pointer(ctype):
    return ctype is C.c_void_p or ctype is C.c_char_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


# ------------------------------------------------------------------------------------------------------------------ completeness
def test_the_text_reader_sees_the_bound_signatures():
    """tests/alignment_cases.py reads parameter NAMES from the header; names, order and pointer-ness agree with what _lib binds"""
    assert set(PROTOS) == set(L.SIGNATURES)
    for entry, (_, argtypes) in L.SIGNATURES.items():
        assert [p[2] for p in PROTOS[entry]] == [_is_pointer(t) for t in argtypes], entry
    for sname, fields in STRUCTS.items():
        bound = getattr(L, sname)._fields_
        assert [f[1] + "_" * (f[1] == "in") for f in fields] == [n for n, _ in bound], sname


def test_every_pointer_parameter_is_a_row_or_exempt():
    for entry in L.SIGNATURES:
        ops = [o for o, _ in A.operands(entry, PROTOS, STRUCTS)]          # (raises for a struct pointer nobody classified)
        assert len(ops) == len(set(ops)), entry
        assert sorted(ops) == sorted(A.ROWS.get(entry, {})), (entry, sorted(set(ops) ^ set(A.ROWS.get(entry, {}))))
        if ops:
            assert entry in A.CALLS, f"{entry} takes device pointers and has no call in CALLS"
        for cls in A.ROWS.get(entry, {}).values():
            assert cls in ("any", "need 4", "need 8", "need 16", "need 8/16"), (entry, cls)
    assert set(A.ROWS) <= set(L.SIGNATURES) and set(A.CALLS) == set(A.ROWS)
    anys = {e for e, r in A.ROWS.items() if "any" in r.values()}
    assert anys == set(A.ANY_HELD_TO), anys ^ set(A.ANY_HELD_TO)


def test_every_pointer_field_of_every_struct_is_a_row_or_exempt():
    covered = set()
    for (entry, param), (sname, prefix) in A.HOST_STRUCTS.items():
        covered.add(sname)
    covered.update(A.DEVICE_TABLE_FIELDS.values())
    for sname, fields in STRUCTS.items():
        ptr_fields = [f for f in fields if f[2]]
        nested = [f for f in fields if f[0] in STRUCTS and not f[2]]
        if ptr_fields:
            users = [k for k, v in A.HOST_STRUCTS.items() if v[0] == sname] + [e for e in A.OPTIM_ENTRIES if sname in A.DEVICE_TABLE_FIELDS.values()]
            parents = [s for s, fs in STRUCTS.items() if any(f[0] == sname and not f[2] for f in fs)]
            assert users or any(p in covered for p in parents), f"{sname} has pointer fields and no entry's rows cover them"
        for f in nested:
            assert f[0] in STRUCTS
    for (sname, fname), why in A.EXEMPT_FIELDS.items():
        assert any(f[1] == fname and f[2] for f in STRUCTS[sname]) and why


def test_no_row_names_a_pointer_that_does_not_exist():
    for (entry, param), why in A.EXEMPT.items():
        assert any(p[1] == param and p[2] for p in PROTOS[entry]) and why, (entry, param)
    for (entry, param), (sname, _) in A.HOST_STRUCTS.items():
        assert any(p[1] == param and p[2] and sname in p[0] for p in PROTOS[entry]), (entry, param)
    for name, why in A.EXEMPT_NAMES.items():
        assert any(p[1] == name and p[2] for ps in PROTOS.values() for p in ps) and why
    for entry, spec in A.CALLS.items():
        ops = set(A.ROWS[entry])
        assert set(spec.get("null", ())) <= ops and set(spec.get("esz", ())) <= ops, entry
        scalars = {p[1] for p in PROTOS[entry] if not p[2]}
        given = {k for k in spec if k not in A._META and not isinstance(spec[k], dict)}
        assert scalars - {"dtype"} == given - {"dtype"} and ("dtype" in scalars) == ("dtype" in given or "dtypes" in spec), (entry, scalars ^ given)


def test_removing_a_row_fails_the_completeness_test(monkeypatch):
    rows = {e: dict(r) for e, r in A.ROWS.items()}
    del rows["xp_cast_back"]["dst"]
    monkeypatch.setattr(A, "ROWS", rows)
    with pytest.raises(AssertionError, match="xp_cast_back"):
        test_every_pointer_parameter_is_a_row_or_exempt()


def test_every_need_row_has_an_offset_that_must_be_refused():
    for entry, operand, dtype, n, offsets in NEED_ROWS:
        assert offsets and all(o % n for o in offsets), (entry, operand, n, offsets)
        assert n != 16 or 8 in offsets, (entry, operand)


# ------------------------------------------------------------------------------------------------------------------ the header
def test_the_header_states_the_table():
    stated = A.header_classes()
    assert set(stated) == set(A.ROWS), set(stated) ^ set(A.ROWS)
    for entry, rows in A.ROWS.items():
        said = dict(stated[entry])
        default = said.pop("*", None)
        assert set(said) <= set(rows), (entry, set(said) - set(rows))
        for operand, cls in rows.items():
            assert said.get(operand, default) == cls, (entry, operand, said.get(operand, default), cls)
        assert default is None or any(o not in said for o in rows), f"{entry}: 'all {default}' names nothing"
    with open(A.HEADER) as f:
        text = f.read()
    assert "Pointer alignment." in text and "is not N-byte aligned" in text


# ------------------------------------------------------------------------------------------------------------------ refusals
def _addresses(entry):
    ops = list(A.ROWS[entry])
    return {o: BASE + (i + 1) * (16 << 20) for i, o in enumerate(ops)}


def _call(entry, dtype, shifted=None, offset=0):
    at = _addresses(entry)
    if shifted is not None:
        at[shifted] += offset
    args, keep = A.build_call(entry, dtype, at.__getitem__, extra=() if shifted is None else (shifted,))
    rc = getattr(L.lib(), entry)(*args)
    return rc, L.lib().xp_last_error().decode()


needs_no_device = pytest.mark.skipif(torch.cuda.device_count() > 0, reason="synthetic addresses: made only where nothing can launch "
                                     "(tests/test_alignment_gpu.py makes these refusals over real buffers)")


@needs_no_device
@pytest.mark.parametrize("entry", [e for e, c in A.CALLS.items() if not c.get("base_unchecked")])
def test_the_aligned_call_passes_every_argument_check(entry):
    """the table's call is otherwise valid: with every operand aligned it is not refused (no device: it ends where it would launch)"""
    for dtype in A.call_dtypes(entry):
        rc, msg = _call(entry, dtype)
        if A.CALLS[entry].get("setter"):
            assert rc == 0, msg
            getattr(L.lib(), entry)(None)
        else:
            assert rc == L.XP_ERR_LAUNCH, (entry, dtype, rc, msg)
            assert "aligned" not in msg


@needs_no_device
@pytest.mark.parametrize("entry", sorted({r[0] for r in NEED_ROWS}))
def test_a_misaligned_base_is_refused_before_any_launch(entry):
    rows = [r for r in NEED_ROWS if r[0] == entry]
    assert rows
    floor_done = set()                  # (an accepted call walks into the HIP runtime, which is slow without a device: the floor of
    for _, operand, dtype, n, offsets in rows:      #  every class below 16 and of one need-16 operand per entry and storage type)
        for off in offsets:
            rc, msg = _call(entry, dtype, operand, off)
            where = (entry, operand, dtype, n, off, rc, msg)
            assert rc == L.XP_ERR_ARG, where
            assert msg.startswith(entry + ":") and f" {operand}=" in msg and f"is not {n}-byte aligned" in msg, where
        spec = A.CALLS[entry]
        if operand not in spec.get("null", ()) and not spec.get("base_unchecked") and (n < 16 or (dtype, n) not in floor_done):
            floor_done.add((dtype, n))                                  # the floor itself is served: aligned to N and not to 2N
            rc, msg = _call(entry, dtype, operand, n)                   # (an operand the base call leaves NULL may be host-readable
            if spec.get("setter"):                                      # labels: not passed on)
                assert rc == 0
                getattr(L.lib(), entry)(None)
            else:
                assert rc == L.XP_ERR_LAUNCH and "aligned" not in msg, (entry, operand, dtype, n, rc, msg)


@needs_no_device
def test_gemm_uint8_frames_need_8():
    """desc.a_frames of decoded uint8 frames (alignment_cases.GEMM_U8_FRAMES): refused 1, 2 and 4 bytes off, accepted at 8"""
    operand, n, offsets = A.GEMM_U8_FRAMES_NEED
    at = _addresses("xp_gemm")
    for off in (0, n) + tuple(offsets):
        shifted = dict(at, **{operand: at[operand] + off})
        args, keep = A.build_call("xp_gemm", A.BF16, shifted.__getitem__, spec=A.GEMM_U8_FRAMES)
        rc, msg = L.lib().xp_gemm(*args), L.lib().xp_last_error().decode()
        if off % n:
            assert rc == L.XP_ERR_ARG and msg.startswith("xp_gemm:") and f" {operand}=" in msg and f"is not {n}-byte aligned" in msg, (off, rc, msg)
        else:
            assert rc == L.XP_ERR_LAUNCH and "aligned" not in msg, (off, rc, msg)


# ------------------------------------------------------------------------------------------------------------------ gradient sinks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


class _LayerProducer(torch.autograd.Function):
    """stand-in for functional.EncoderLayerFn's backward: ONE autograd node per layer that, inside a real backward pass, asks
    functional._claim_sink for the layer's sink as functional._layer_backward does, writes the layer's flat gradient into the sink
    or into a private buffer, and hands autograd the views"""

    @staticmethod
    def forward(ctx, h, rank, gi, log, *group):
        ctx.rank, ctx.gi, ctx.log, ctx.group = rank, gi, log, group
        return h.clone()

    @staticmethod
    def backward(ctx, g):
        import xpretrain_amd.functional as XF
        group, gi = ctx.group, ctx.gi
        key, numel = XF.grad_sink_key(group), sum(p.numel() for p in group)
        sink = XF.GRAD_SINKS.get(key)
        flat = XF._claim_sink(key, sink, numel, group[0].device, group)
        ctx.log.append((gi, sink is not None, sink.data_ptr() % 16 if sink is not None else None, flat is not None))
        if flat is None:
            flat = torch.empty(numel)
        flat.copy_((ctx.rank + 1) * torch.sin(torch.arange(numel, dtype=torch.float32) + gi))
        views = [v.view_as(p) for p, v in zip(group, flat.split_with_sizes([p.numel() for p in group]))]
        return (g, None, None, None) + tuple(views)


def _sink_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from oracle import clipvip_oracle as O
    from xpretrain_amd import distributed as D
    import xpretrain_amd.functional as XF
    from xpretrain_amd.modeling import VidCLIP
    D.init_from_env("gloo")
    torch.manual_seed(0)

    class Args:
        clip_config = O.hf_config_dict(128, 2, 2, 256, 16, 32, 128, 2, 2, 256, 120, 16, 64)
        clip_weights = ""
        clip_vision_additional_config = dict(type="ViP", temporal_size=3, if_use_temporal_embed=1, logit_scale_init_value=4.6, add_cls_num=3)
    model = VidCLIP(Args())
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    ls = [(n, p) for n, p in named if n.endswith("logit_scale")]
    assert len(ls) == 1 and ls[0][1].numel() == 1
    rest = [(n, p) for n, p in named if not n.endswith("logit_scale")]
    groups = XF.layer_grad_groups(model)
    assert len(groups) == 4
    out = {}
    # the reducer places parameters in REVERSE order: a logit_scale that comes last in the list leads the bucket
    for order, plist in (("natural", ls + rest), ("scale_in_front", rest + ls)):
        red = D.GradBucketReducer([p for _, p in plist], average=True, layout_groups=groups)
        assert len(red.buckets) == 1 and len(XF.GRAD_SINKS) == len(groups)
        log = []
        grouped = {id(p) for g in groups for p in g}
        h = sum((rank + 1.0) * p.sum() for _, p in plist if id(p) not in grouped)      # loose parameters: gradient rank + 1
        for gi, g in enumerate(groups):
            h = _LayerProducer.apply(h, rank, gi, log, *g)
        h.backward()
        red.synchronize()
        out[order] = dict(log=log,
                          grads={n: p.grad.detach().clone() for n, p in plist})
        red.zero_grad()
        red.remove()
        assert not XF.GRAD_SINKS
    nat, odd = out["natural"], out["scale_in_front"]
    ok = all(has and mod == 0 and claimed for _, has, mod, claimed in nat["log"]) and len(nat["log"]) == len(groups)
    ok = ok and all(has and mod == 4 and not claimed for _, has, mod, claimed in odd["log"]) and len(odd["log"]) == len(groups)
    same = all(torch.equal(nat["grads"][n], odd["grads"][n]) for n in nat["grads"])
    mean = (1 + world) / 2
    want = torch.allclose(nat["grads"][ls[0][0]], torch.tensor(mean)) and float(nat["grads"][rest[0][0]].abs().sum()) > 0
    q.put((rank, bool(ok), bool(same), bool(want), nat["log"], odd["log"]))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_a_misaligned_gradient_sink_is_declined_and_the_gradients_stay_the_same():
    """logit_scale in front of the layer groups of the reducer's bucket: every sink starts 4 bytes off; _claim_sink declines each,
    the private buffer plus the reducer's pack copy take over, and the averaged gradients are those of the natural order bit for bit"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sink_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in res:
        assert r[1], ("claims", r[4], r[5])
        assert r[2], "the gradients differ between the two parameter orders"
        assert r[3]
