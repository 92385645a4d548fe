"""The chain spread of pi and beta, on the device (include/ammsb_spread.h).  The library against the numpy statement of its
header (spread_statement.py states it once, and test_spread_host.py checks it on the CPU against the dense float64 variance
of every sample): mean, var, last, the bound, the row sums and beta's moments are asserted bit for bit.  The learner's
variance against the float64 variance of pi snapshots taken after every iteration, within the header's bound.

One child process per group (spread_child.py):
  exact    the library driven directly over a pi the test mutates between calls.  N = 3000 in blocks of 1100 rows; K in {1, 5,
           13, 30, 64, 65, 256, 1024, 4096, 4160, 8192}: every group width, both kernel forms, a ragged last trip; K = 64 and
           1024 once more with blocks 4 bytes off a 16-byte boundary.  Twelve rounds at every K of node lists that
           straddle the three blocks, with repeats and ids >= N, and range calls between them; a range flush in three ragged
           slabs.  mean, var and last bit-equal to the statement after every call, the mean bit-equal to what
           ammsb_average_rows leaves over the same calls, two runs equal (K <= 1024), the words past every buffer
           untouched, rows with w == 0 not written; the bound at z in {-2, 0, 1.5} and the row sums bit-equal, in ragged slabs.
  far      rows past byte 2^32, element 2^31 and element 2^32 of a block for rows, bound and rowsum: K = 8192.
  contend  one node listed 4096 times in one call is flushed once: its variance moves once.
  learner  N = 2000, K = 64, mini-batch 128, eager loop: Run(10), StartAverage(spread=True), Run(1) x 30 with every sample
           recorded; mean, var and beta's moments bit-equal to the recorded chain replayed through the statement, var within
           the bound of the dense variance, rows no mini-batch held have var 0, BetaStd to 1e-9, MembershipSpread and
           Unsettled against numpy; a twin with spread=False keeps the same mean bit for bit;
           Run(20) + StartAverage(spread=True) + Run(20) + Averaged() leaves the checkpoint Run(40) leaves.
  views    Averaged().Bound(-2): CommunitySizes, CommunityQuality, RelatedCommunities and NodeRoles equal the same analyses
           over the numpy statement of the bound; Bound(0) equals the mean's; the view refreshes after Run(5), answers
           for the new chain after a restart with the same spread and as many steps, and raises after StopAverage().
  cpp      tests/cpp/spread_test.cc: the synchronous and the async loop replayed through the statement from the recorded
           samples (GetVarPiRow, GetMeanPiRow and GetVarBeta bit-equal: the replay the Python learner is held to in
           `learner`), CommunityQuality under ReadBound(true, -2).
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "spread_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4 5 6 11", "7 8 12", "9", "10"])
def test_mean_var_bound_and_rowsum_equal_the_statement_bit_for_bit(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_rows_past_element_2_32_of_a_block():
    _run(["far"], "far ok", 300)


def test_a_node_listed_4096_times_moves_its_variance_once():
    _run(["contend"], "contend ok", 180)


def test_learner_variance_against_the_dense_variance_of_every_sample():
    _run(["learner"], "learner ok", 300)


def test_every_analysis_reads_the_bound():
    _run(["views"], "views ok", 300)


def test_cpp_learner_keeps_the_same_spread():
    _run(["cpp"], "cpp ok", 600)
