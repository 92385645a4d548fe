"""The read-out of a fitted pi on the device (include/ammsb_readout.h): memberships, counts and community sizes equal a
numpy statement written in the child (`np.argsort(-row, kind="stable")` is exactly "value descending, column
ascending"), compared exactly: ids, count and sizes as integers, weights by bit pattern.

One child process per group (readout_child.py):
  shapes   K in {1, 3, 48, 64, 113, 256, 512, 1024, 2048, 4096, 8192} x T in {1, 4, 16} (T > K included) x rows in
           {1, 63, 65, 5000}; rows drawn as fitted rows (Dirichlet alpha = 1/K: the early exit), flat rows (alpha = 1:
           all T rounds) and a mix; thresholds 0, exactly a stored value, above every entry, one that leaves more than
           T columns; the library names the fast form for K a multiple of 256 and the generic form otherwise.
  layout   pi as one, two and eleven-plus-a-ragged-one blocks; row slabs that start and end inside a block, with sizes
           accumulated across the calls; a node list in descending order with repeats.
  ties     uniform rows, a whole row at the floor 1e-24, the maximum repeated inside one lane, across lanes and across
           256-column pieces, more holders of the maximum than T.
  big      K = 8192 and a little over 2^32 elements in one block: the last 4096 rows, a node list and sizes; again from a
           base 4 bytes past a 16-byte boundary: readout_generic, the same outputs.
  learner  Learner.Memberships / CommunitySizes / Communities on bench.py's C1 after 30 steps (eager and graph launch);
           slabs; Run(20) + read-out + Run(20) leaves the checkpoint buffers Run(40) leaves.
  cpp      tests/cpp/readout_test.cc (mcmc::Learner::Memberships against GetPiRow), its memberships and communities file
           against the numpy statement over the pi of the checkpoint it wrote; ammsb_main --communities-out.
"""
import functools

import pytest

from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "readout_child.py", timeout=1500)


def test_every_shape_equals_the_numpy_statement():
    _run(["shapes", "all"], "shapes ok all")


def test_blocks_slabs_and_node_lists():
    _run(["layout"], "layout ok")


def test_ties_go_to_the_lower_column():
    _run(["ties"], "ties ok")


def test_rows_beyond_2_to_the_32_elements():
    _run(["big"], "big ok")


@pytest.mark.parametrize("graph", [0, 1])
def test_learner_read_out_and_an_unperturbed_run(graph):
    _run(["learner", str(graph)], "learner ok")


def test_cpp_learner_and_command_line():
    _run(["cpp"], "cli ok")
