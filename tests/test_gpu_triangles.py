"""The triangles inside the detected communities, on the device (include/ammsb_triangles.h).  Everything against the integer
statement of the header's definitions (triangles_statement.py states it once, and test_triangles_host.py checks it on the
CPU against powers of the dense adjacency): the device adds and compares integers, so every output is asserted equal, and
the float64 values, one host formula over equal integers, bit-equal.

One child process per group (triangles_child.py):
  exact    N = 5600, fewer than 40000 targets; K in {1, 5, 64, 65, 256, 1024, 4096, 4160, 8192}: W = 1, 2, 4, 16, 64 and the
           two-word form, a last word with unused bits at 65 and 4160.  One graph: a node without a link, two triangles that
           share an edge, a K4, a clique of 70 (rows of 69: more than a wave of candidates), a star (a hub row without a
           triangle), rows of 0, 1, 2, 63, 64 and 65 targets, hubs of ROW_LDS - 1, ROW_LDS, ROW_LDS + 1 and 5000 neighbours
           over a sparse random graph among them, offsets[0] > 0.  Covers: a node without a community (a triangle with no
           shared community, whose edges at that node take the shortcut), corners that share exactly one community and
           several (across words and inside the last word), NaNs and values equal to thr planted, thr = 0 at K = 64 (every
           bit set), garbage in the mask's bits past K.  Every output equals the statement, the words past every output
           are untouched, two runs are equal, an empty range and an adjacency without targets are no-ops; an unsorted row,
           a loop and a target >= N are refused by ops.Triangles.nodes before anything is launched.
  cut      more nodes than one pass of the persistent grid under both forms, in one call and in three ragged ranges:
           bit-equal, the K-sized sums and counts included; a range alone writes nothing outside it.
  cross    through the learner on one edge list: with a partition the sum of ktri3 == the sum of tri_in and triangles[k]
           is the statement on each induced subgraph; with every node in community 0 ktri3[0] == the sum of tri, kpart[0]
           == #{tri > 0}, tri_in == tri; degree == NodeRoles' degree; wedges >= ktri3; a list with repeats and loops gives
           the integers of its simplified list, with .dropped and .skipped counted.
  far      a hand-made mask of 2^22 + 128 rows x 128 words (4 GiB + 128 KiB, K = 8192), zeroed on the device, planted rows
           in [0, 128), around row 2^21 and around row 2^22, triangles inside and across the windows: every output equals
           the statement over the planted rows and is 0 elsewhere (checked on the device).  The statement over the rows a
           wrapped 32-bit byte offset would read is first shown to differ in tri_in, ktri3 and kpart.
  planted  hostlib's planted graph and cover at N = 10^4 with pi set to the planted memberships: equal to the statement;
           the mean tpr over the communities of at least 3 members is larger than with the node ids permuted (a sign).
  learner  bench.py's C1, eager and graph launch: Run(20) + Triangles() + Run(20) leaves the checkpoint buffers Run(40)
           leaves; the result equals the statement over the learner's pi and the simplified training_csr(); a node range.
  cpp      tests/cpp/triangles_test.cc and ammsb_main --triangles-out: each file equals, byte for byte, write_triangles of
           the statement over the checkpoint's pi and the training links the same process wrote.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "triangles_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4", "5 6", "7 8"])
def test_every_output_equals_the_integer_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_one_call_three_ragged_ranges_and_more_than_one_pass_of_the_grid():
    _run(["cut"], "cut ok", 180)


def test_partitions_the_whole_graph_as_one_community_and_a_list_with_repeats():
    _run(["cross"], "cross ok", 240)


def test_a_mask_past_byte_offset_2_32():
    _run(["far"], "far ok", 300)


def test_planted_cover_equals_the_statement_and_has_a_higher_tpr_than_a_permuted_graph():
    _run(["planted"], "planted ok", 180)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_triangles_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
