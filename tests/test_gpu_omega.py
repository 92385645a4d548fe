"""The Omega index of the detected cover against a ground-truth cover, on the device (include/ammsb_omega.h).
Everything against the numpy statement of the header's definitions (omega_child.py states it): integer adds on both
sides, so every count is asserted equal.

One child process per group (omega_child.py):
  exact    n in {1, 2, 63, 64, 65, 129, 300} and 257 (just past two tiles of 128), K in {1, 31, 32, 33, 65, 260, 1024,
           1028, 8192}, G in {1, 7, 33, 300, 5000} (8192 and 5000 at n = 300); pi with about K^-1/2 of the entries at or
           above thr, NaNs and values equal to thr planted; the universes all, covered and a ragged list; members == N
           and == 2^32 - 1 (skipped) and members outside the list.  agree, detected, truth, skipped, outside and the
           per-row counts equal the statement; sum detected == sum truth == P; clipped == 0; two calls bit-equal; the
           words past every output untouched; the whole triangle, a tile per launch and a ragged three-way cut
           bit-equal; with L one below the need, clipped and the histograms equal the statement cut at that level.
  planted  truth == the detected cover under a column permutation (omega == 1.0); n = 4, D = {{0,1},{2,3}}, T =
           {{0,1,2,3}} (omega == 0.0); a pair that shares 2 communities in both covers; thr = 0 and thr above every
           value; a truth whose members are all skipped (NaN).
  forms    every kernel form named and reached on both sides of its dispatch boundary; a misaligned pi takes the generic
           form and writes the same words; the identity universe.
  persistent  n = 3000 at K = 64, G = 64 (300 tiles), and n = 4200 (561 tiles, more than the grid's 512 blocks).
  big      pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, 17 GB, zero but 640
           planted rows in four windows that straddle byte offset 2^32, element 2^31 and element 2^32): detected bits of
           the 640 planted rows and of the last window alone, as omega_bits_fast and, from a base 4 bytes past a 16-byte
           boundary, as omega_bits_generic; truth bits and pairs against a ground truth with members >= N (skipped) and
           members in zero rows (outside).  The inputs are first shown to tell a wrapped 32-bit offset apart in every
           figure that reads pi.
  learner  Learner.CoverOmega on bench.py's C1 after 30 steps (eager and graph launch) with hostlib.generate_cover as
           the truth, over a universe of 2000 nodes and "covered", against the statement over the checkpointed pi;
           Run(20) + the call + Run(20) leaves the checkpoint buffers Run(40) leaves.  No recovery score is asserted:
           nobody has measured one.
  cpp      tests/cpp/omega_test.cc (mcmc::Learner::CoverOmega / WriteCoverOmega); its file and ammsb_main --ground-truth
           ... --cover-omega-out ... parsed back and compared with the statement over the pi of the checkpoint the same
           process wrote; the Python writer's bytes match; --cover-match-out and --cover-nmi-out alone still work.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "omega_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4 5", "6 7", "8 9 10 11"])
def test_counts_equal_the_numpy_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 180)


def test_planted_covers_and_hand_worked_pairs():
    _run(["planted"], "planted ok", 120)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 120)


def test_tiles_through_the_persistent_loop():
    _run(["persistent"], "persistent ok", 120)


def test_pi_past_element_2_32_in_both_forms():
    _run(["big"], "big ok", 300)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_cover_omega_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
