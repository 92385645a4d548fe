"""The reference's rand_r mini-batch stream drawn on the device (Config.sampling_stream = "reference",
ops.ReferenceStreamSampler, include/ammsb_refsample.h) against the reference-exact host sampler, bit for bit.

One child process per group (refsample_child.py):
  sampler     ReferenceStreamSampler against hostlib.Dataset.sample (host/sample.cc) from the same seed: edges, nodes,
              counts, weight, seed afterwards and the number of rand_r calls consumed, every batch of >= 200 consecutive
              ones per strategy (each batch's seed is the previous one's result); m = 32, 1024, 65536 on N = 2^17 .. 10^6;
              a data set without held-out edges; a run that holds (u, u) edges; a 5000-edge vertex forced as u.  The
              child first establishes that the CSR the device reads is the host Graph's adjacency order, and for every
              batch that the host stream needs no more candidates than the sizing rule provides.
  shortfall   a capacity too small is an error the caller sees, and nothing is written past what is reported.
  trajectory  a Learner with the reference stream equals a Learner with host sampling after 60 steps on bench.py's C1
              and C2 (pi rows, beta, theta, phi sums, both Sample seeds, the perplexity), with
              sample_parallel on and off; each mode's mid-run checkpoint resumed in the other mode ends in the same state.
"""
import functools

import pytest

import refsample_child as rc
from postfit_support import run_group

pytestmark = pytest.mark.gpu

_run = functools.partial(run_group, "refsample_child.py", timeout=1500)


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_sampler_equals_the_host_sampler(case):
    _run(["sampler", case], "sampler ok %s" % case)


def test_shortfall_is_reported_and_memory_safe():
    _run(["shortfall"], "shortfall ok")


@pytest.mark.parametrize("workload,parallel", [("C1", 1), ("C1", 0), ("C2", 1), ("C2", 0)])
def test_learner_trajectory_equals_host_sampling(workload, parallel):
    _run(["trajectory", workload, str(parallel)], "trajectory ok %s" % workload)
