"""The k-core decomposition of every detected community, on the device (include/ammsb_cores.h).  Everything against the
statement of the header's definitions (cores_statement.py states it once, and test_cores_host.py checks it on the CPU against
the definition itself): every output is an integer that the cover and the simple adjacency alone determine, so every one is
asserted equal, and the float64 values, one host formula over equal integers, bit-equal.  scans and rounds are launch counts:
rounds <= M and scans <= 2 (distinct core values) + 1.

One child process per group (cores_child.py):
  exact    N = 6000, fewer than 60000 keys; K in {1, 5, 64, 65, 256, 1024, 4096, 4160, 8192}: every group width, the two-word
           form, a last word with unused bits at 65 and 4160.  One graph: a clique of 40, a cycle, a path of 2000 with its keys
           ascending, descending and shuffled, a star of 3000 leaves, a K20 with a fringe of degree-1 and degree-2 members, two
           communities that share a clique, a community without an internal link, an empty community, a node in no community,
           ends that share several communities across words and inside the last word; NaNs and values equal to thr planted;
           thr = 0 at K = 64; garbage in the mask's bits past K.  indeg, nbr_off, nbr, core and all K- and N-sized arrays
           equal the statement, two runs are equal, the words past every output are untouched, both kernel forms of each
           build pass are seen, an empty list gives core == 0 everywhere, and the bad calls the child lists are refused
           before any launch.
  cut      degrees and adjacency in one call, in three ragged node ranges and in the ranges reversed: bit-equal; a frontier
           of more than 2^18 slots that leave at one level, more than one pass of the peel's grid.
  contend  N = 2048, every node in the communities 0 .. 7, 2 10^5 random keys: equal to the statement, and the eight
           communities have identical cores.
  cross    through the learner on one edge list: members == CommunitySizes, inlinks2 == NodeRoles' ksum (among="own") == 2
           CommunityQuality.internal on the simple list, isolated == CommunityComponents.singletons, the corners of
           Triangles' inside triangles have core >= 2, and every node in community 0 against the cores of the whole graph.
  deep     slot ids past 2^31 in queue and nbr: K = 8192 at thr = 0 over a zeroed pi of 2^18 + 64 rows.
  far      library-level calls: nbr an uninitialised buffer of 2^30 + 2^16 entries, the rows of a small slot graph planted
           through nbr_off at its start, around byte offset 2^32 and at its end.
  planted  hostlib's planted graph and cover at N = 10^4: equal to the statement; the mean degeneracy over the communities of
           at least 3 members is larger than with the node ids permuted (a sign, verified on the CPU first).
  learner  bench.py's C1, eager and graph launch: Run(20) + CommunityCores() + Run(20) leaves the checkpoint buffers Run(40)
           leaves; the result equals the statement over the learner's pi and TrainingLinks().
  cpp      tests/cpp/cores_test.cc: the file WriteCommunityCores writes equals, byte for byte, write_cores of the statement
           over the checkpoint's pi and the training links the same process wrote.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "cores_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4", "5 6", "7 8"])
def test_every_output_equals_the_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_node_ranges_in_pieces_and_a_frontier_of_more_than_one_pass_of_the_grid():
    _run(["cut"], "cut ok", 180)


def test_heavy_concurrent_lowering_of_the_same_degrees():
    _run(["contend"], "contend ok", 180)


def test_against_the_other_analyses_and_the_whole_graph():
    _run(["cross"], "cross ok", 240)


def test_slot_ids_past_2_31():
    _run(["deep"], "deep ok", 300)


def test_neighbour_rows_past_byte_offset_2_32():
    _run(["far"], "far ok", 300)


def test_planted_cover_equals_the_statement_and_is_deeper_than_on_a_permuted_graph():
    _run(["planted"], "planted ok", 180)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_cores_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_writes_the_bytes_of_the_statement():
    _run(["cpp"], "cpp ok", 600)
