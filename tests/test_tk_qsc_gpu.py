"""The q4_0 persistent kernel's per-layer scale records (csrc/token_kernel.h tk_qsc) against a float64 pass: what every launch
leaves there (invariant R of DESIGN.md section 3d2: a field tagged p holds position p's maximum of the sequence actually fed), who
clears it, what a redone position leaves, and that the counter of range events counts events in a row.  The model, the sequences,
the mirror of the scale rule and the drivers are tests/qsc_ref.py's; tests/test_tk_qsc_cpu.py proves them without a device.

Measured on an MI355X (the figures DESIGN.md quotes; each test prints its own): records within 1.7e-5 of the float64 pass, logits
within 1.3e-5 of max |logit| (top-8 element-wise 9.2e-6); the floor of the comparison, float32 against float64, is 1.2e-6."""
import pytest

import qsc_ref as Q
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    return Q.build()


@pytest.fixture(scope="module")
def worst():
    w = Q.Worst()
    yield w
    print("\ntk_qsc, all tests:", w)


@pytest.fixture
def ctx(built):
    made = []

    def make():
        m = llmk.Llmk(built.fw)
        made.append(m)
        assert m.path() == 1, "TkTinyLlamaQ4's columns: the persistent kernel"
        return m
    yield make
    for m in made:
        m.close()


def test_g1_clean_run(built, worst, ctx):
    Q.g1(ctx(), built, worst)
    print(worst)


def test_g2_event_and_the_positions_after_it(built, worst, ctx):
    Q.g2(ctx(), built, worst)
    print(worst)


def test_g3_spike_after_spike(built, worst, ctx):
    Q.g3(ctx(), built, worst)
    print(worst)


@pytest.mark.parametrize("how", ["reset", "prefill", "score"])
def test_g4_clearing(how, built, worst, ctx):
    Q.g4(ctx(), built, worst, how)


def test_g5_rewind_over_an_event(built, worst, ctx):
    Q.g5(ctx(), built, worst)


def test_g6_pipelined_loop_over_two_events(built, worst, ctx):
    Q.g6(ctx(), built, worst, ctx)


def test_g7_events_with_clean_positions_between_them_are_not_in_a_row(built, worst, ctx):
    Q.g7(ctx(), built, worst)
    print(worst)


def test_g8_a_record_with_another_positions_tag_is_not_history(built, worst, ctx):
    Q.g8(ctx(), built, worst, ctx)
