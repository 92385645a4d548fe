"""The connected components of every detected community, on the device (include/ammsb_components.h).  Everything against the
statement of the header's definitions (components_statement.py states it once, and test_components_host.py checks it on the
CPU against boolean powers of the dense induced adjacency): every output is an integer that the partition alone determines,
so every one is asserted equal, and the float64 values, one host formula over equal integers, bit-equal.

One child process per group (components_child.py):
  exact    N = 6000, fewer than 60000 keys; K in {1, 5, 64, 65, 256, 1024, 4096, 4160, 8192}: W = 1, 2, 4, 16, 64 and the
           two-word form, a last word with unused bits at 65 and 4160.  One graph: a path of 5000 nodes inside one community
           with its keys ascending, descending and shuffled, a star of 5000 leaves, two cliques joined by keys through a node
           that is no member (two components) and, in another community, through the same node as a member (one), a community
           without an internal key, an empty community, a node in no community, two components of equal size, a == a keys,
           repeats, both orders of the ends, ends >= N; ends that share one community and several, across words and inside
           the last word; NaNs and values equal to thr planted; thr = 0 at K = 64; garbage in the mask's bits past K.  Two
           runs are equal, the words past every output are untouched, counts[3] == 0, an empty list gives all singletons,
           and 19 bad calls are refused before any launch.
  cut      more keys than one pass of the persistent grid under both forms: one call, three ragged pieces, the pieces in
           reverse order, the slots numbered in one call and in three node ranges: bit-equal.
  contend  N = 4096, every node in the communities 0 .. 7, 2 10^5 random keys: one component of size N each, shared = 8 links.
  cross    through the learner on one edge list: members == CommunitySizes, shared == the sum of SharedCommunities, a
           partition against the statement on each induced subgraph, every node in community 0 against the components of
           the whole graph, and the singletons against NodeRoles' members without a neighbour inside.
  deep     slot ids past 2^31 and byte offsets of parent past 2^32: K = 8192 at thr = 0 over a zeroed pi of 2^18 + 64 rows.
  far      a hand-made mask of 2^22 + 128 rows x 128 words (4 GiB + 128 KiB), planted rows in three windows.
  planted  hostlib's planted graph and cover at N = 10^4: equal to the statement; the mean giant over the communities of at
           least 3 members is larger than with the node ids permuted (a sign).
  learner  bench.py's C1, eager and graph launch: Run(20) + CommunityComponents() + Run(20) leaves the checkpoint buffers
           Run(40) leaves; the result equals the statement over the learner's pi and TrainingLinks().
  cpp      tests/cpp/components_test.cc: the file WriteCommunityComponents writes equals, byte for byte, write_components
           of the statement over the checkpoint's pi and the training links the same process wrote.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "components_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4", "5 6", "7 8"])
def test_every_output_equals_the_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_one_call_three_ragged_pieces_and_more_than_one_pass_of_the_grid():
    _run(["cut"], "cut ok", 180)


def test_heavy_concurrent_hooking_on_the_same_roots():
    _run(["contend"], "contend ok", 180)


def test_against_the_other_analyses_partitions_and_the_whole_graph():
    _run(["cross"], "cross ok", 240)


def test_slot_ids_past_2_31():
    _run(["deep"], "deep ok", 300)


def test_a_mask_past_byte_offset_2_32():
    _run(["far"], "far ok", 300)


def test_planted_cover_equals_the_statement_and_is_less_fragmented_than_a_permuted_graph():
    _run(["planted"], "planted ok", 180)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_components_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_writes_the_bytes_of_the_statement():
    _run(["cpp"], "cpp ok", 600)
