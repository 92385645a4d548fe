"""How the detected communities relate to each other, on the device (include/ammsb_relate.h).  Everything against the
numpy statement of the header's definitions (relate_child.py states it): integer adds and integer compares on both
sides, so every word, count and partner is asserted equal.

One child process per group (relate_child.py):
  exact    N in {1, 63, 64, 65, 127, 129, 1000, 4100}, K in {1, 2, 31, 33, 64, 65, 127, 129, 260, 1024}, K = 8192 at
           N = 300; pi with about K^-1/2 of the entries at or above thr, NaNs and values equal to thr planted, one column
           that holds every node and one that holds none; thr = 0 and thr above every value; pi in two and in three
           blocks whose rows_in_block is no multiple of 64.  The bit words equal the statement's np.packbits words, the
           overlap equals M.T @ M, its diagonal CommunitySizes, the matrix its transpose; partners and shared equal a
           stable host selection by fractions.Fraction for the three measures, top in {1, 4, 64} and min_overlap in
           {1, 3}; the words past every output untouched; two calls bit-equal; one slab, slabs of 64 rows and a ragged
           three-way cut bit-equal.
  depth    shapes whose pair pass takes more than one depth slice per tile and more (tile, slice) items than the grid has
           blocks (relate_child.depth_group derives them from the kernel's constants).
  forms    every kernel form named and reached on both sides of its dispatch boundary; a pi misaligned by 4 bytes takes
           the generic form and writes the same words.
  planted  two identical columns (Jaccard exactly 1, each the other's first partner); a strict subset (inside == 1.0 on
           one side, contained == 1.0 on the other); disjoint columns without a partner; ties to the lower id.
  big      pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, 17 GB, zero but 640
           planted rows in four windows that straddle byte offset 2^32, element 2^31 and element 2^32): bits of all rows
           and of the slab that begins 128 rows before element 2^32, as relate_bits_fast and, from a base 4 bytes past a
           16-byte boundary, as relate_bits_generic; the words of the planted rows equal the statement's, every other word
           is 0, both forms equal; overlap, its diagonal and the partners of the full bits.  The inputs are first shown
           to tell a wrapped 32-bit offset apart in every figure compared.
  learner  bench.py's C1 after 30 steps (eager and graph launch): RelatedCommunities and CommunityOverlap against the
           statement over the checkpointed pi; a max_bytes that forces many slabs gives the same tensors; Run(20) + the
           calls + Run(20) leaves the checkpoint buffers Run(40) leaves.  No property of the fitted cover is asserted:
           nobody has measured one.
  cpp      tests/cpp/relate_test.cc (mcmc::Learner::CommunityOverlap / RelatedCommunities / WriteRelatedCommunities); its
           file and the files ammsb_main --related-communities-out wrote, parsed back and compared with the statement
           over the pi of the checkpoint the same process wrote; the Python writer's bytes match.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "relate_child.py")


@pytest.mark.parametrize("cases", ["0 1 2 3 4 5 6", "7 8 9", "10"])
def test_words_counts_and_partners_equal_the_numpy_statement(cases):
    _run(["exact"] + cases.split(), "exact ok", 180)


def test_depth_slices_through_the_persistent_loop():
    _run(["depth"], "depth ok", 120)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 120)


def test_planted_duplicates_subsets_disjoint_columns_and_ties():
    _run(["planted"], "planted ok", 120)


def test_pi_past_element_2_32_in_both_forms():
    _run(["big"], "big ok", 300)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_related_communities_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
