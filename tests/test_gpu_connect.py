"""How the detected communities are linked to each other, on the device (include/ammsb_connect.h).  Everything against the
numpy statement of the header's definitions (connect_child.py states it): integer adds and integer compares on both
sides, so every word, count and partner is asserted equal.

One child process per group (connect_child.py):
  exact    N in {1, 2, 65, 1000}, K in {1, 2, 63, 64, 65, 129, 260, 1024}, K = 4100 and 8192 at N = 300; pi with about
           K^-1/2 of the entries at or above thr, NaNs and values equal to thr planted, one column that holds every node
           and one that holds none; thr = 0 (at K = 65) and thr above every value; pi in two and in three blocks whose
           rows_in_block is no multiple of 64.  Edge lists of 0, 1, 257 and 3000 keys, sorted and shuffled, both orders of
           the ends, duplicates, self loops and keys with an end >= N.  The mask words equal the statement's np.packbits
           words; directed, links and counts equal the statement under every form the shape has; links its transpose,
           its diagonal twice ops.CommunityQuality's internal; partners, links and shared equal a stable host selection
           by fractions.Fraction for both measures, top in {1, 4, 64} and min_links in {1, 3}; the words past every
           output untouched; two calls bit-equal; one call and three ragged calls bit-equal.
  forms    every kernel form named and reached on both sides of its dispatch boundary; direct and runs forced on the same
           inputs give equal matrices; a pi misaligned by 4 bytes takes the generic mask form and writes the same words;
           an unknown AMMSB_CONNECT_FORM is refused.
  depth    more edges than one pass of either edge kernel's persistent grid (derived from the kernels' constants), one
           run longer than a wave's chunk, runs that straddle chunk boundaries.
  planted  two disjoint columns with every link between them (density exactly 1.0, in bridged()); disjoint columns
           without a link between them have no partner; ties to the lower id; a pair of communities without a pair of
           distinct nodes is no partner by density.
  big      pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, 17 GB, zero but 640
           planted rows in four windows that straddle byte offset 2^32, element 2^31 and element 2^32): the mask as
           connect_mask_fast and, from a base 4 bytes past a 16-byte boundary, as connect_mask_generic, equal to the
           statement's words on the planted rows and 0 elsewhere; edges (connect_edges_direct, the only form at this K),
           finish and top over keys between every two windows with loops, repeats, ends >= N and ends in zero rows.  The
           inputs are first shown to tell a wrapped 32-bit offset apart in every figure that reads pi.
           connect_edges_runs (K <= 4096) reads no pi and is left out.
  learner  bench.py's C1 after 30 steps (eager and graph launch): CommunityLinks and LinkedCommunities against the
           statement over the checkpointed pi and the data set's training links; the diagonal against CommunityQuality;
           Run(20) + the calls + Run(20) leaves the checkpoint buffers Run(40) leaves.  No property of the fitted cover is
           asserted: nobody has measured one.
  cpp      tests/cpp/connect_test.cc (mcmc::Learner::CommunityLinks / LinkedCommunities / WriteLinkedCommunities); its
           file and the files ammsb_main --linked-communities-out wrote, parsed back and compared with the statement over
           the pi of the checkpoint and the training links the same process wrote; the Python writer's bytes match.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "connect_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4 5 6", "7 8 9 10", "11", "12"])
def test_words_counts_and_partners_equal_the_numpy_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 300)


def test_more_edges_than_one_pass_and_runs_across_chunks():
    _run(["depth"], "depth ok", 180)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 180)


def test_planted_bridges_disjoint_columns_ties_and_empty_pairs():
    _run(["planted"], "planted ok", 120)


def test_pi_past_element_2_32_in_both_forms():
    _run(["big"], "big ok", 300)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_linked_communities_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
