"""Planting NaN / Inf in one element of a kernel's input (a helper, not a test; it touches neither the GPU nor the package).

The rule the non-finite tests hold, per planted element e of one input:
  D(e)  the outputs whose value in the op's fp64 reference changes in any bit when e is replaced by e + 1.0 on the CLEAN inputs
        (`dependent_set`): the kernel's output must be non-finite on all of it.  The probe is finite, so structural zeros (masks,
        operands a kind does not read) drop out by themselves; it is a probe, not a bound.
  I(e)  outputs of an independent problem, stated structurally by the caller: the kernel's planted run must be finite there and
        bit-identical to its own clean run.
Everything else is unasserted.  No tolerance anywhere: non-finite, or bit-equal.

Inputs and outputs travel as dicts name -> tensor (an output that a case does not have is absent or None); a reference is a
callable `ref_fn(inputs, dtype=torch.float64) -> outputs` that converts the floating inputs to `dtype` itself and passes integer
inputs (ids, masks) through.
"""
import torch

NAN, INF = float("nan"), float("inf")


def value_name(v):
    return "nan" if v != v else ("+inf" if v > 0 else "-inf")


def _bits_differ(a, b):
    """elementwise: a and b differ in any bit (fp64; NaN payloads and the sign of zero count)"""
    return a.contiguous().view(torch.int64) != b.contiguous().view(torch.int64)


def as_double(inputs):
    return {k: (v.detach().double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inputs.items()}


def dependent_set(ref_fn, inputs, which, flat_index):
    """D(e) as {output name: bool mask}: where the fp64 reference on the clean inputs and on the inputs with element `flat_index` of
    `inputs[which]` raised by 1.0 (in fp64) differ in any bit."""
    base = as_double(inputs)
    probe = dict(base)
    t = base[which].clone()
    t.reshape(-1)[flat_index] += 1.0
    probe[which] = t
    a, b = ref_fn(base), ref_fn(probe)
    out = {}
    for name, x in a.items():
        if x is None:
            continue
        out[name] = _bits_differ(x.double(), b[name].double()).reshape(x.shape)
    return out


def plant(inputs, which, flat_index, value):
    """a copy of `inputs` whose tensor `which` is cloned with `value` at `flat_index` (-1 or a slice: wherever that indexes)"""
    out = dict(inputs)
    t = inputs[which].clone()
    t.reshape(-1)[flat_index] = value
    out[which] = t
    return out


def nonfinite(outputs):
    """{name: ~isfinite} of the outputs that are there"""
    return {k: ~torch.isfinite(v) for k, v in outputs.items() if v is not None}


def _where(mask, limit=4):
    idx = mask.nonzero()
    return f"{int(mask.sum())} of {mask.numel()} e.g. {[tuple(i.tolist()) for i in idx[:limit]]}"


def check(planted_out, clean_out, D, I, tag):
    """Every violation of the rule at once: `planted_out` must be non-finite on D and, on I, finite and bit-equal to `clean_out`.
    D, I: {output name: bool mask}; raises one AssertionError that names every violated output."""
    bad = []
    for name, mask in (D or {}).items():
        if mask is None or not mask.any():
            continue
        got = planted_out[name].detach().cpu()
        swallowed = mask & torch.isfinite(got).reshape(mask.shape)
        if swallowed.any():
            bad.append(f"{name}: finite where it depends on the plant (swallowed): {_where(swallowed)}")
    for name, mask in (I or {}).items():
        if mask is None or not mask.any():
            continue
        got, clean = planted_out[name].detach().cpu(), clean_out[name].detach().cpu()
        leak = mask & ~torch.isfinite(got).reshape(mask.shape)
        if leak.any():
            bad.append(f"{name}: non-finite in an independent problem (leaked): {_where(leak)}")
        moved = mask & ~leak & (got != clean).reshape(mask.shape)
        if moved.any():
            bad.append(f"{name}: an independent problem's bits moved: {_where(moved)}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def check_equal(a, b, tag):
    """never-read bytes: every output of run `a` torch.equal to run `b`, NaN positions included (compared as bits)"""
    bad = []
    for name, x in a.items():
        if x is None:
            continue
        x, y = x.detach().cpu().contiguous(), b[name].detach().cpu().contiguous()
        if x.shape != y.shape or not torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)):
            bad.append(name)
    assert not bad, f"{tag}: outputs changed by bytes that are never read: {bad}"


def count(D):
    return sum(int(m.sum()) for m in D.values() if m is not None)


class Plant:
    """One planted element of a case: input `which`, flat index, the values to plant, the structural D (`expect`: {name: mask}, or
    None where none is easy to state) and I ({name: mask}).  `where` is a word for the test id."""

    def __init__(self, which, index, values=(NAN,), expect=None, independent=None, where="", unread=None):
        self.which, self.index, self.values, self.expect, self.independent = which, index, tuple(values), expect, independent or {}
        self.where = where or f"{which}[{index}]"
        # a plant in an element that is never read must change NOTHING (every output bit-equal); by default that is a plant whose
        # structural D is empty.  unread=False: D is empty, but the element is read and masked (either answer is legal outside I)
        self.unread = (expect is not None and count(expect) == 0) if unread is None else unread

    def __repr__(self):
        return self.where


class Case:
    """A kernel case: `name`, `family`, `inputs` (dict, built once, never modified), `ref(inputs, dtype)`, its `plants`.
    `selects`: the op's gradient is piecewise constant in the planted operand (a hinge, a hardest negative), so the + 1.0 probe flips
    selections that a NaN does not travel through in the reference either: there the required set is D(e) cut to where the planted
    fp64 reference is itself non-finite, and must still hold the loss."""

    def __init__(self, family, name, inputs, ref, plants, selects=False, extra=None, derive=None):
        self.family, self.name, self.inputs, self.ref, self.plants, self.selects = family, name, inputs, ref, plants, selects
        self.extra = extra or {}
        # derive(D): outputs that are plain sums of other outputs (column sums over thousands of rows) take their D from the addends'
        # -- in the fp64 sum itself a one-row change can round away
        self.derive = derive
        self._D = {}

    def D(self, p):
        key = (p.which, p.index)
        if key not in self._D:
            self._D[key] = dependent_set(self.ref, self.inputs, p.which, p.index)
            if self.derive is not None:
                self.derive(self._D[key])
        return self._D[key]

    def required(self, p, value):
        """the set the kernel must make non-finite for plant p of `value`"""
        D = self.D(p)
        if not self.selects:
            return D
        nf = nonfinite(self.ref(plant(as_double(self.inputs), p.which, p.index, value)))
        return {k: m & nf[k].reshape(m.shape) for k, m in D.items()}

    def pairs(self):
        return [(p, v) for p in self.plants for v in p.values]


def verify_reference(case):
    """The CPU side of one case, for every (plant, value) it lists: (a) the planted fp64 reference is non-finite on the required set
    (which, for a case that `selects`, still holds the first output: the loss); (b) D equals the structural set where the plant
    states one -- an empty one for a plant that must change nothing; (c) the planted reference is bit-unchanged on I; a +-inf plant also has the same non-finite set in fp32 as in fp64.
    Returns the number of required outputs."""
    total = 0
    clean = case.ref(as_double(case.inputs))
    for p in case.plants:
        D = case.D(p)
        tag = f"{case.family} {case.name} {p}"
        empty = p.expect is not None and count(p.expect) == 0              # a plant that must reach nothing: D is empty, by (b)
        assert empty or count(D) > 0, f"{tag}: nothing depends on the plant"
        if p.expect is not None:
            for name, mask in D.items():
                want = p.expect.get(name)
                want = torch.zeros_like(mask) if want is None else want.reshape(mask.shape)
                assert torch.equal(mask, want), f"{tag}: D[{name}] is not the structural set: {_where(mask ^ want)} differ"
        for name, mask in p.independent.items():
            assert not (D[name] & mask.reshape(D[name].shape)).any(), f"{tag}: I[{name}] overlaps D"
        for v in p.values:
            vtag = f"{tag} {value_name(v)}"
            planted = case.ref(plant(as_double(case.inputs), p.which, p.index, v))
            req = case.required(p, v)
            check(planted, clean, req, None, vtag + " (a)")
            if case.selects:
                first = next(iter(req))
                assert req[first].any(), f"{vtag}: the primary output {first} is not required"
            for name, mask in p.independent.items():
                same = ~_bits_differ(planted[name].double(), clean[name].double()).reshape(mask.shape)
                assert same[mask].all(), f"{vtag} (c): the reference moved on I[{name}]"
            if v == v:                                                    # +-inf: usable only where fp32 agrees with fp64
                lo = case.ref(plant(case.inputs, p.which, p.index, v), dtype=torch.float32)
                for name, m in nonfinite(planted).items():
                    assert torch.equal(m, ~torch.isfinite(lo[name])), f"{vtag}: fp32 and fp64 non-finite sets differ on {name}"
            total += count(req)
    return total


def drive(case, run, tag=""):
    """One case on a kernel: `run(inputs) -> outputs` (CPU tensors or device tensors) once on the clean inputs and once per
    (plant, value); every plant is checked and ALL violations are reported together.  Returns the number of outputs required."""
    clean = run(case.inputs)
    assert all(torch.isfinite(v).all() for v in clean.values() if v is not None), f"{case.name}: the clean run is not finite"
    bad, total = [], 0
    for p, v in case.pairs():
        planted = run(plant(case.inputs, p.which, p.index, v))
        req = case.required(p, v)
        total += count(req)
        try:
            check(planted, clean, req, p.independent, f"{case.family} {case.name}{tag} {p} {value_name(v)}")
            if p.unread:
                check_equal(planted, clean, f"{case.family} {case.name}{tag} {p} {value_name(v)}")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
    return total
