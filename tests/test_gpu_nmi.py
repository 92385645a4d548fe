"""The overlapping NMI of the detected cover against a ground-truth cover, on the device (include/ammsb_nmi.h).
Everything against the numpy float64 statement of the header's definitions, fed the same integers and written with the
same association (nmi_child.py states it, the bound 2^-47 S and the borderline guard).

One child process per group (nmi_child.py):
  exact    K in {1, 3, 64, 65, 260, 1024, 1028, 8192} x G in {1, 7, 300}, N from 600 to 4999; overlap matrices (a) made
           from a random pi by the existing cover match (members == N and == 2^32 - 1 skipped) and (b) integers made by
           hand (sparse overlaps, columns above half the nodes, noisy copies, identical pairs, empty communities),
           passed straight to the library; the whole matrix, one row per slab and a ragged three-way split; every
           element within 2^-47 S, +inf and the exact 0 of identical pairs exactly; two calls bit-equal, the three
           slabbings bit-equal, the words past every output untouched; ops.CoverNMI gives the same bits.
  planted  truth == the detected cover under a column permutation (every c exactly 0, nmi_lfk == 1.0, nmi_max within
           4 ulp of 1); N = 8, t = d = 4, o = 2 (lhs == rhs, c = 1 = H); a complement and a complement plus one shared
           node (+inf, the fallback on the host); N = 1000, t = 1, d = 599, o = 0 (qualifies); thr = 0 and thr above
           every value; a ground truth whose members are all skipped; inputs that break the contract.
  forms    both kernel forms named and reached on both sides of the 1024-column chunk boundary; a misaligned overlap.
  persistent  more tiles than the grid has blocks: G = 3000 at K = 64, G = 300 at K = 8192.
  learner  Learner.CoverNMI on bench.py's C1 after 30 steps (eager and graph launch) with hostlib.generate_cover as
           the truth, over the checkpointed pi, at three slab sizes; Run(20) + the calls + Run(20) leaves the
           checkpoint buffers Run(40) leaves.  No recovery score is asserted: nobody has measured one.
  cpp      tests/cpp/nmi_test.cc (mcmc::Learner::CoverNMI / WriteCoverNMI); its file and ammsb_main --ground-truth ...
           --cover-nmi-out ... parsed back and compared with the statement over the pi of the checkpoint the same
           process wrote, for a data-set dump and a text graph with non-dense ids; the Python writer's bytes match; the
           flag rules give status 2; --cover-match-out alone still works.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "nmi_child.py")


@pytest.mark.parametrize("ks", ["1 3 64 65 260", "1024 1028", "8192"])
def test_entropies_equal_the_numpy_statement(ks):
    _run(["exact"] + ks.split(), "exact ok", 180)


def test_planted_covers_and_hand_worked_pairs():
    _run(["planted"], "planted ok", 120)


def test_every_kernel_form_is_named_and_reached():
    _run(["forms"], "forms ok", 120)


def test_tiles_through_the_persistent_loop():
    _run(["persistent"], "persistent ok", 120)


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_cover_nmi_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok", 300)


def test_cpp_learner_and_the_command_line_driver():
    _run(["cpp"], "cli ok", 600)
