"""Scoring communities against a graph, on the device (include/ammsb_quality.h).  Everything against the numpy
statement M = pi >= np.float32(thr); both = M[a] & M[b]; one = M[a] ^ M[b]; column sums over the valid edges for
internal and boundary, both.sum(1) for shared -- integer counts over binary32 compares, so every figure exactly equal.

One child process per group (quality_child.py):
  exact    K in {1, 3, 64, 65, 100, 256, 260, 1024, 2048, 8192} x n in {1, 3, 257, 5000}, N from 600 to 4999; rows
           fitted-looking, flat, one-hot, with NaNs, with a planted value and with the next float below it; thresholds
           0 (every bit set), 0.05, the planted value's bits (the tie is a member, the float below is not) and one
           above every value (all uncovered); both orders of the ends, a == b, duplicates, an end == N and == 2^32 - 1;
           counts-only and shared-only calls against the full call; two calls bit-equal; the words past every output
           untouched; the set bits of the mask are the members and no more; 2 internal + boundary = the members'
           degrees summed.
  persistent  20 011 edges at K in {64, 256, 1024, 2048, 8192}: more edges than the grid has groups of lanes, several
           edges per wave and several words per lane, special edges past 8192.
  layout   pi as one, two and eleven-plus-a-ragged-one blocks; a misaligned block base takes the generic mask form at
           K = 256 and writes the fast form's bytes.
  forms    every mask and edges form is named and reached.
  big      K = 8192 beyond 2^32 elements (17 GB, zeroed), members and edges among the last rows; again from a base 4
           bytes past a 16-byte boundary: quality_mask_generic, the same mask and counts.
  learner  Learner.CommunityQuality / SharedCommunities on bench.py's C1 after 30 steps (eager and graph launch) over
           the checkpointed pi; size equals CommunitySizes; Run(20) + the calls + Run(20) leaves the checkpoint buffers
           Run(40) leaves.
  cpp      tests/cpp/quality_test.cc; its file and ammsb_main --community-quality-out parsed back and compared with
           the statement over the pi of the checkpoint the same process wrote; the Python writer's bytes.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "quality_child.py")


@pytest.mark.parametrize("ks", ["1 3 64 65 100", "256 260 1024", "2048", "8192"])
def test_counts_and_shared_equal_the_numpy_statement(ks):
    _run(["exact"] + ks.split(), "exact ok", 180)


@pytest.mark.parametrize("ks", ["64 256 1024", "2048 8192"])
def test_groups_through_their_persistent_loop(ks):
    _run(["persistent"] + ks.split(), "persistent ok", 180)


def test_blocks_of_pi_and_a_misaligned_base():
    _run(["layout"], "layout ok", 120)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 120)


def test_rows_beyond_2_to_the_32_elements():
    _run(["big"], "big ok", 180)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_community_quality_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_command_line():
    _run(["cpp"], "cli ok", 300)
