"""The chain average of pi and beta, on the device (include/ammsb_average.h).  The library against the numpy statement of
its header (average_statement.py states it once, and test_average_host.py checks it on the CPU against the dense float64
mean of every sample): mean, last, beta's binary64 mean and its rounding are asserted bit for bit.  The learner's mean
against the float64 mean of pi snapshots taken after every iteration, within (n + 1) * 2^-22 per entry.

One child process per group (average_child.py):
  exact    the library driven directly over a pi the test mutates between calls.  N = 3000 in blocks of 1100 rows; K in {1, 5,
           64, 65, 256, 1024, 4096, 4160} and 13, 30: every group width, both kernel forms, a ragged last trip; K = 64 once
           more with blocks 4 bytes off a 16-byte boundary.  Six iterations of node lists that straddle the three blocks, with
           repeats and ids >= N; a range flush in three ragged slabs and in one.  mean and last bit-equal to the statement
           after every call, two runs equal, the words past every buffer untouched, rows with w == 0 not written (NaNs
           planted in mean behind last == n survive), beta's mean and its rounding bit-equal.
  far      rows past byte 2^32, element 2^31 and element 2^32 of a block: K = 8192, uninitialised pi and mean.
  contend  one node listed 4096 times in one call is flushed once.
  learner  bench.py's C1, eager loop, Run(1) x 40: the mean against the dense mean of the snapshots, rows no mini-batch held
           bit-equal to pi, a view that follows the chain; Run(20) + StartAverage + Run(20) + Averaged() leaves the checkpoint
           Run(40) leaves; the graph loop and force_exchange are refused; Parse() ends the average; n = 0 raises.
  views    Averaged().Memberships / CommunitySizes / LinkProbabilities / CommunityCores equal their libraries called on the
           downloaded mean; the held-out AUC of the mean is printed beside the last draw's (not a condition).
  cpp      tests/cpp/average_test.cc: the synchronous and the async loop against a float64 mean kept from GetPiRow,
           ReadAverage(true) against a read-out of the downloaded mean, the refusal under graph_launch.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "average_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 8 9 10", "4 5", "6 7"])
def test_mean_and_last_equal_the_statement_bit_for_bit(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_rows_past_element_2_32_of_a_block():
    _run(["far"], "far ok", 300)


def test_a_node_listed_4096_times_is_flushed_once():
    _run(["contend"], "contend ok", 180)


def test_learner_mean_against_the_dense_mean_of_every_sample():
    _run(["learner"], "learner ok", 300)


def test_every_analysis_reads_the_mean():
    _run(["views"], "views ok", 300)


def test_cpp_learner_keeps_the_same_mean():
    _run(["cpp"], "cpp ok", 600)
