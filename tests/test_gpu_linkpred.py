"""Link prediction on the device (include/ammsb_linkpred.h).  Dense scores (`block`) and per-pair scores (`pairs`)
against a float64 numpy statement under the derived bound (K + 8) 2^-24 M + 2^-100; the T best candidates per query
(`top`) against the stable argsort of `block`'s rows with the ineligible entries removed, exactly: ids as integers,
scores by bit pattern.

One child process per group (linkpred_child.py):
  accuracy   K in {1, 3, 48, 64, 113, 256, 512, 1024, 2048, 4096, 8192} x Q in {1, 31, 32, 33, 200} x candidates in
             {1, 63, 65, 5000}; rows fitted-looking, flat, at the floor 1e-24 and mixed; beta near 0, near 1 and below
             eps; pairs over the same data, both orders of the ends, a == b, an end out of range.
  selection  T in {1, 10, 64} (T > the eligible candidates included); no set, one set, two sets; a query whose whole
             range is excluded; repeated and out-of-range queries; the two-slab merge; Q = 1 against the same query
             inside a batch of 200; two calls bit-equal; identical candidate rows spread over the whole range.
  layout     pi as one, two and eleven-plus-a-ragged-one blocks; cand_lo and the end inside a block.
  forms      every kernel form the dispatchers can select is named and reached.
  big        N = 10^6, K = 1024 (4.1 GB), Q = 64, T = 10 with the tie-tolerant check; K = 8192 beyond 2^32 elements
             (a zeroed block).
  planted    a constructed model whose AUC is exactly 1 (and 0 with the labels flipped).
  learner    Learner.LinkProbabilities / PredictLinks / HeldoutAUC on bench.py's C1 after 30 steps (eager and graph
             launch); slabs; Run(20) + the three calls + Run(20) leaves the checkpoint buffers Run(40) leaves.
  cpp        tests/cpp/linkpred_test.cc (mcmc::Learner::LinkProbabilities / PredictLinks against GetPiRow arithmetic
             under the bound, eligibility against the host sets), its links file against the pi of the checkpoint it
             wrote; ammsb_main --links-out parsed back and compared with the numpy statement over its checkpoint's pi.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "linkpred_child.py", timeout=1500)


def test_dense_and_pair_scores_meet_the_derived_bound():
    _run(["accuracy", "all"], "accuracy ok")


def test_top_equals_the_stable_argsort_of_block():
    _run(["selection"], "selection ok")


def test_blocks_of_pi_and_candidate_ranges_inside_a_block():
    _run(["layout"], "layout ok")


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok")


def test_a_million_rows_and_rows_beyond_2_to_the_32_elements():
    _run(["big"], "big ok")


def test_a_planted_model_has_auc_one():
    _run(["planted"], "planted ok")


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_link_prediction_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok")


def test_cpp_learner_and_command_line():
    _run(["cpp"], "cli ok")
