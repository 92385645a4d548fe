"""Merging and dropping communities of the fitted model, on the device (include/ammsb_reduce.h).  The library against the
numpy statement of its header (reduce_statement.py states it once, and test_reduce_host.py checks it on the CPU against the
dense float64 definition): pi', phi_sum', theta' and the count of emptied rows are asserted bit for bit.

One child process per group (reduce_child.py):
  exact    the library driven directly.  N = 3000, pi in blocks of 1100 rows and the outputs in blocks of 1300; K in {1, 5, 13,
           30, 64, 65, 256, 1024, 4096, 4160, 8192}: every group width, both load widths, blocks of 256 and of 128 lanes;
           K = 64 once more with every block 4 bytes off a 16-byte boundary.  Per K the identity, the reversal, "keep every
           third" (select, drops), "all into one" (one lane walks K sources), interleaved groups of 1..7 sources with and
           without drops, and K' = K - 1.  Rows hold zeros and subnormals; one row is all zero, one holds a NaN, one has its
           whole mass in dropped columns.  Three ragged slabs and one; a plan that selects runs in the select and in the
           merge form; every run equals the statement, reports the expected form and leaves the words before and after
           every output, and pi itself, untouched.
  far      DeviceBench.big_pi (K = 8192, rows past byte 2^32, element 2^31 and element 2^32 of a block), aligned and 4 bytes
           off: to K' = 8 over every row and, dropping, over the planted windows; by a permutation into a second block of
           the same size.  The windows equal the statement, every other output row is all-zero; the statement over the rows
           a wrapped 32-bit offset would read differs.
  learner  bench.py's C1, eager and graph launch: Reduce(identity) is the same model bit for bit at the same stepCount; a
           plan from RelatedCommunities(...).duplicates and drop_smaller(CommunitySizes(0.05), 2) equals the statement over
           the downloaded state, the new learner runs, its perplexity is finite, Memberships and CommunityQuality work at
           K'; Run(20) + Reduce + Run(20) leaves the old learner with Run(40)'s checkpoint; a sharded learner and a plan of
           another K are refused.  The perplexities before and after are printed, not asserted.
  cpp      tests/cpp/reduce_test.cc: mcmc::Learner::Reduce against a host restatement over GetPiRow / GetPhiSum / GetTheta
           bit for bit, the reduced learner stepping in the synchronous, the async and the graph form, the old learner
           unperturbed, the refusals; the plan file WritePlan leaves holds the bytes of Python's text form.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "reduce_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4 5 6 7 8", "9 10", "11"])
def test_the_reduced_model_equals_the_statement_bit_for_bit(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_rows_past_element_2_32_of_a_block_in_and_out():
    _run(["far"], "far ok", 300)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_reduce_carries_the_model_and_the_step_size(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_reduces_to_the_same_bits():
    _run(["cpp"], "cpp ok", 600)
