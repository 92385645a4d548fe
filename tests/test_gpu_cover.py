"""Matching the detected cover to a ground-truth cover, on the device (include/ammsb_cover.h).  Everything against the
numpy statement M = pi >= np.float32(thr); overlap[g] = M[members_g].sum(0); the argmax of overlap / (t_g + d_k) by
integer cross-multiplication, equal rationals to the lower index -- integers throughout, so every figure exactly equal,
the dense overlap included.

One child process per group (cover_child.py):
  exact    K in {1, 3, 64, 65, 100, 256, 260, 1024, 2048, 8192} x G in {1, 7, 300}, N from 600 to 4999; community
           sizes 0, 1, 2, 63, 64, 65, unit - 1, unit, unit + 1 and 3 unit + 5, so that communities end on, just before
           and just after a unit boundary and one spans several; rows fitted-looking, flat, one-hot, with NaNs, with a
           planted value and with the next float below it; thresholds 0, 0.05, the planted value's bits and one above
           every value (everything unmatched); members == N and == 2^32 - 1, a duplicated member; the dense output on
           and off; two calls bit-equal; the words past every output and past the workspace untouched.  With K = 3
           also the planted ties: identical columns, 1/4 against 2/8 in both orders and its mirror image over g, and
           4095/8191 against 4096/8193 (equal as binary32 quotients) in both directions.
  persistent  more units than the grid has waves at K in {64, 256, 1024, 8192}.
  layout   pi as one, two and eleven-plus-a-ragged-one blocks; a misaligned block base takes the generic form at
           K = 256 and gives the same results.
  forms    every counting form is named and reached, at K on both sides of every chunk boundary.
  big      K = 8192 beyond 2^32 elements (17 GB, zeroed), members among the last rows; again from a base 4 bytes past a
           16-byte boundary: cover_generic, the same outputs.
  constructed  pi built from the generator's planted cover under a known column permutation: the match is the
           permutation and every F1 is exactly 1; one community halved has the hand-computed F1.
  learner  Learner.CompareCover on bench.py's C1 after 30 steps (eager and graph launch) with hostlib.generate_cover
           as the truth, over the checkpointed pi; Run(20) + the calls + Run(20) leaves the checkpoint buffers Run(40)
           leaves.  No recovery score is asserted: nobody has measured one.
  cpp      tests/cpp/cover_test.cc (mcmc::Learner::CompareCover / WriteCoverMatch against GetPiRow compares); its file
           and ammsb_main --ground-truth ... --cover-match-out ... parsed back and compared with the statement over the
           pi of the checkpoint the same process wrote, for a data-set dump (dense ids) and for a text graph whose ids
           are not dense (mapped, the unknown ones dropped and counted); the Python writer's bytes match.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "cover_child.py")


@pytest.mark.parametrize("ks", ["1 3 64 65 100", "256 260 1024", "2048", "8192"])
def test_matches_equal_the_numpy_statement(ks):
    _run(["exact"] + ks.split(), "exact ok", 180)


@pytest.mark.parametrize("ks", ["64 256", "1024 8192"])
def test_units_through_the_persistent_loop(ks):
    _run(["persistent"] + ks.split(), "persistent ok", 180)


def test_blocks_of_pi_and_a_misaligned_base():
    _run(["layout"], "layout ok", 120)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 120)


def test_rows_beyond_2_to_the_32_elements():
    _run(["big"], "big ok", 180)


def test_a_constructed_pi_recovers_its_planted_cover():
    _run(["constructed"], "constructed ok", 120)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_compare_cover_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
