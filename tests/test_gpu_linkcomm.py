"""The communities that explain a link, on the device (include/ammsb_linkcomm.h).  ids and terms against the stable
argsort of the numpy float32 statement t = (pa * pb) * beta_odd, exactly: ids as integers, terms by bit pattern; prob
against float64 under the derived bound (K + 8) 2^-24 M + 2^-100; sizes against np.bincount of the statement's slot 0.

One child process per group (linkcomm_child.py):
  exact    K in {1, 3, 64, 100, 256, 260, 512, 1024, 2048, 8192} x T in {1, 4, 16} x n in {1, 3, 257, 5000}; rows
           fitted-looking, flat (all terms tied), one-hot, at the floor 1e-24 (subnormal and underflowing products),
           mixed, and with planted equal products in the same lane and in different lanes; beta near 0, near 1 and
           exactly 0; min_term 0, equal to the planted term's bits, and above every term; both orders of the ends;
           a == b; an end == N and == 2^32 - 1; two calls bit-equal; sizes-only equals the sizes of a full call; the
           words past every output untouched.
  persistent  K in {256, 1024, 1280, 2048} with 20 011 edges, more than the grid has waves: the fast forms' loop (the
           next edge requested before the rounds, the chunked hand-over, several edges per counter), special edges past 8192.
  layout   pi as one, two and eleven-plus-a-ragged-one blocks; a misaligned block base (generic at K = 256).
  forms    every kernel form the dispatcher can select is named and reached.
  big      K = 8192 beyond 2^32 elements (17 GB, zeroed), 512 edges among the last rows; again from a base 4 bytes past
           a 16-byte boundary: linkcomm_generic, the same ids, terms and sizes.
  learner  Learner.TrainingLinks / LinkCommunities / LinkCommunitySizes on bench.py's C1 after 30 steps (eager and
           graph launch); slabs; Run(20) + the calls + Run(20) leaves the checkpoint buffers Run(40) leaves.
  cpp      tests/cpp/linkcomm_test.cc; its file and ammsb_main --link-communities-out parsed back and compared with
           the statement over the pi of the checkpoint the same process wrote; the Python writer's bytes.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "linkcomm_child.py")


@pytest.mark.parametrize("ks", ["1 3 64 100", "256 260 512", "1024 2048", "8192"])
def test_ids_and_terms_equal_the_numpy_statement(ks):
    _run(["exact"] + ks.split(), "exact ok", 180)


@pytest.mark.parametrize("ks", ["256 1024", "1280 2048"])
def test_fast_forms_through_their_persistent_loop(ks):
    _run(["persistent"] + ks.split(), "persistent ok", 180)


def test_blocks_of_pi_and_a_misaligned_base():
    _run(["layout"], "layout ok", 120)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 120)


def test_rows_beyond_2_to_the_32_elements():
    _run(["big"], "big ok", 180)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_link_communities_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_command_line():
    _run(["cpp"], "cli ok", 300)
