"""The overlapping modularity of the detected cover, on the device (include/ammsb_modularity.h).  Everything against the
Python-integer statement of the header's definitions (modularity_child.py states it once): the device adds integers modulo
2^128, so every sum, degree and count is asserted equal, and the float64 values, one host formula over equal integers,
bit-equal.

One child process per group (modularity_child.py):
  exact    N <= 2000, lists of <= 20000 keys with duplicates, self loops, both orders of the ends and ends >= N; K in {1,
           5, 64, 65, 256, 1024, 4096, 4160, 8192}: W = 1, 2, 4, 16, 64 and the two-word form, a last word with unused
           bits at 65 and 4160; NaNs and values equal to thr planted; one node without a community, one without an edge;
           thr = 0 at K = 64 (O = K for every node); an empty list.  internal, volume, degree and counts equal the
           statement, the words past every output untouched, two runs equal.
  carry    5 and 9 links inside a community of single-membership nodes (the low word wraps once and twice), a node of
           degree >= 4 in it (the product's high part); next to each other in one block and spread over the grid; both
           forms.
  cut      more edges than one pass of the persistent grid, in one call and in three ragged calls: bit-equal.
  cross    on a partition internal == CommunityQuality's internal << 62 and volume == (2 internal + boundary) << 62, and
           q is Newman's modularity.
  planted  hostlib's planted graph and cover at N = 10^4 with pi set to the planted memberships: q > 0, equal to the
           statement; against the unquantised rationals |dq_k| <= 8 2^-53 (2 in_k + s_k^2 / 2m) / 2m + 2^-36 |q_k| (the
           float64 rounding of the four operations, and the fixed-point bound at the library's limits: derived, not
           measured).
  big      pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, 17 GB, zero but 640
           planted rows in four windows that straddle byte offset 2^32, element 2^31 and element 2^32): run() over the
           keys of connect's big group, the mask as connect_mask_fast and, from a base 4 bytes past a 16-byte boundary, as
           connect_mask_generic; internal, volume and counts equal the statement's 128-bit integers, degree [N] equals it
           on the planted rows and is 0 elsewhere (modularity_edges_w2 / _nodes_w2).  The inputs are first shown to tell
           a wrapped 32-bit offset apart in internal and volume.  The _w1 forms (K <= 4096) read no pi and are left out.
  learner  bench.py's C1, eager and graph launch: Run(20) + Modularity() + Run(20) leaves the checkpoint buffers Run(40)
           leaves; the result equals the statement over the learner's pi copied to the host.
  cpp      tests/cpp/modularity_test.cc and ammsb_main --modularity-out: each file equals, byte for byte,
           write_modularity of the statement over the checkpoint's pi and the training links the same process wrote.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "modularity_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4", "5 6", "7 8"])
def test_sums_degrees_and_counts_equal_the_integer_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_the_low_word_wraps_and_the_product_has_a_high_part():
    _run(["carry"], "carry ok", 120)


def test_one_call_three_ragged_calls_and_more_than_one_pass_of_the_grid():
    _run(["cut"], "cut ok", 180)


def test_a_partition_gives_the_quality_counts_shifted_and_newmans_modularity():
    _run(["cross"], "cross ok", 120)


def test_planted_cover_scores_above_chance_within_the_derived_bound():
    _run(["planted"], "planted ok", 180)


def test_pi_past_element_2_32_in_both_forms():
    _run(["big"], "big ok", 300)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_modularity_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
