"""GPU: the three optimizer updates produce the bits recorded in ``tests/golden/optim_bits.json`` -- no tolerance.

The fixture was recorded on an MI355X with the library built from the commit named in its header (``python -m tests.optim_bits
--record``; ``tests/optim_bits.py`` says what is run and what is hashed).  Whatever is done to ``csrc/optim.hip`` afterwards, the
unguarded ``AdamW``, ``Adam`` and ``Adamax`` steps keep every bit of p, m, v, the shadow copies and the gradient norm on the ragged
tensor set: scalar tail, 16-byte path on and off, chunk edges, two launch tables, two parameter groups.  The guarded kernels hang on
the same bits through ``tests/test_guarded_step_gpu.py::test_finite_steps_have_the_unguarded_bits``."""
import json

import pytest

from tests import guarded_step_ref as G
from tests import optim_bits as B

pytestmark = pytest.mark.gpu

with open(B.FIXTURE) as _f:
    RECORDED = json.load(_f)


def test_the_inputs_are_the_recorded_ones():
    assert B.inputs_digest() == RECORDED["header"]["inputs_sha256"], \
        "the inputs differ from the ones the fixture was recorded on (tests/optim_bits.py::inputs, or the ragged set's SIZES): " \
        "no digest below can be compared"


def test_the_fixture_holds_every_case():
    assert set(RECORDED["cases"]) == {B.case_name(kind, clip) for kind in G.KINDS for clip in B.CLIPS}
    for name, case in RECORDED["cases"].items():
        assert set(case["tensors"]) == {str(i) for i in B.NAMED} and len(case["shadows"]) == 3
        assert len(case["norms"]) == (0 if name.endswith("None") else 3)


@pytest.mark.parametrize("clip", B.CLIPS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_three_steps_have_the_recorded_bits(kind, clip):
    assert B.inputs_digest() == RECORDED["header"]["inputs_sha256"], "the inputs differ from the recorded ones"
    diff = B.differences(RECORDED["cases"][B.case_name(kind, clip)], B.run(kind, clip))
    assert not diff, f"{kind}, clip {clip}: bits differ from the library at {RECORDED['header']['recorded_at_commit'][:7]}:\n" + "\n".join(diff)
