"""The role of every node in the detected cover, on the device (include/ammsb_roles.h).  Everything against the integer
statement of the header's definitions (roles_child.py states it once): the device adds and compares integers, so every
output is asserted equal, and the float64 values, one host formula over equal integers, bit-equal.

One child process per group (roles_child.py):
  exact    N <= 2000, at most 20000 targets; K in {1, 5, 64, 65, 256, 1024, 4096, 4160, 8192}: W = 1, 2, 4, 16, 64 and the
           two-word form, a last word with unused bits at 65 and 4160; rows of 0, 1, 63, 64 and 65 targets and a hub row of
           5000 (far longer than a trip of 64 targets; there is no block form); repeated targets, b == a, targets >= N;
           NaNs and values equal to thr planted; a node without a community and one whose neighbours all have none;
           offsets[0] > 0; among both ways, top 1, 4, 16 and 0, min_count 0 and 3; equal counts inside a word and across
           lanes; thr = 0 at K = 64 (O = K); an adjacency without a target and an empty range.  Every output equals the
           statement, the words past every output are untouched, two runs are equal, and garbage in the mask's bits past K
           changes nothing.
  cut      more nodes than one pass of the persistent grid under both forms, in one call and in three ragged ranges:
           bit-equal, the K-sized sums included; a range alone writes nothing outside it.
  cross    one edge list through the learner: degree == Modularity's, ksum == the diagonal of CommunityLinks == 2
           CommunityQuality.internal, kmembers == CommunitySizes, the sum of embedded == 2 (links - uncovered).
  planted  hostlib's planted graph and cover at N = 10^4 with pi set to the planted memberships: equal to the statement,
           misplaced() included; the mean embeddedness is larger than with the graph's node ids permuted (a sign).
  big      pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, 17 GB, zero but 640
           planted rows in four windows that straddle byte offset 2^32, element 2^31 and element 2^32): run() over the
           adjacency of the keys of connect's big group, the mask as connect_mask_fast and, from a base 4 bytes past a
           16-byte boundary, as connect_mask_generic; one state from one call equals one from two calls cut 128 rows
           before element 2^32; every per-node array equals the statement on the planted rows and is 0 (home: -1)
           elsewhere, the K-sized sums and counts are equal (roles_nodes_w2).  The inputs are first shown to tell a
           wrapped 32-bit offset apart in every figure that reads pi.  roles_nodes_w1 (K <= 4096) reads no pi and is left
           out.
  learner  bench.py's C1, eager and graph launch: Run(20) + NodeRoles() + Run(20) leaves the checkpoint buffers Run(40)
           leaves; the result equals the statement over the learner's pi and training_csr(); a node range.
  cpp      tests/cpp/roles_test.cc and ammsb_main --node-roles-out: each file equals, byte for byte, write_roles of the
           statement over the checkpoint's pi and the training adjacency the same process wrote.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "roles_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4", "5 6", "7 8"])
def test_every_output_equals_the_integer_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_one_call_three_ragged_ranges_and_more_than_one_pass_of_the_grid():
    _run(["cut"], "cut ok", 180)


def test_degrees_diagonal_sizes_and_coverage_agree_with_the_other_analyses():
    _run(["cross"], "cross ok", 180)


def test_planted_cover_equals_the_statement_and_is_more_embedded_than_a_permuted_graph():
    _run(["planted"], "planted ok", 180)


def test_pi_past_element_2_32_in_both_forms():
    _run(["big"], "big ok", 300)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_node_roles_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
