"""GPU: the loss family, the pair losses and the materialised retrieval-evaluation kernels produce the bits recorded in
``tests/golden/loss_bits.json`` -- no tolerance.  The fixture was recorded on an MI355X with the library built from the commit named
in its header (``python -m tests.loss_bits --record``; ``tests/loss_bits.py`` says what is run and what is hashed).  Whatever is done
afterwards to the four files of ``csrc`` that hold the loss family, the pair losses, the retrieval kernels and the small GEMM, every
output keeps every bit."""
import pytest

from tests import loss_bits as B

pytestmark = pytest.mark.gpu


def test_the_inputs_are_the_recorded_ones_and_keep_the_margin():
    B.check_inputs()
    B.check_pair_margins()


def test_the_fixture_holds_every_case():
    cases = B.recorded()["cases"]
    names = [B.family_name(*c) for c in B.family_cases()] + [B.pair_name(*c) for c in B.pair_cases()] + list(B.RETRIEVAL_NAMES)
    assert len(set(names)) == len(names) and set(cases) == set(names)
    for c in B.family_cases():
        _, use_img, use_cap = B.R.KINDS[c[0]]
        want = {"loss", "d_vis", "d_txt", "d_log_scale"} | ({"d_img"} if use_img else set()) | ({"d_cap"} if use_cap else set())
        assert set(cases[B.family_name(*c)]) == want
    assert all(set(cases[B.pair_name(*c)]) == {"loss", "d_vis", "d_txt"} for c in B.pair_cases())


@pytest.mark.parametrize("case", B.family_cases(), ids=lambda c: B.family_name(*c))
def test_family_has_the_recorded_bits(case):
    B.check(B.family_name(*case), B.run_family(*case))


@pytest.mark.parametrize("case", B.pair_cases(), ids=lambda c: B.pair_name(*c))
def test_pair_loss_has_the_recorded_bits(case):
    B.check(B.pair_name(*case), B.run_pair(*case))


def test_retrieval_kernels_have_the_recorded_bits():
    got = B.run_retrieval()
    assert set(got) == set(B.RETRIEVAL_NAMES)
    for name in B.RETRIEVAL_NAMES:
        B.check(name, got[name])
