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
import os
import subprocess
import sys

import pytest

import refsample_child as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "refsample_child.py")


def _run(args, expect):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no fallback path exists)")
    out = subprocess.run([sys.executable, CHILD] + args, capture_output=True, text=True, timeout=1500,
                         cwd=os.path.dirname(HERE))
    if out.returncode != 0:
        pytest.fail("group %r (exit %d):\n%s\n%s" % (args, out.returncode, out.stdout[-2000:], out.stderr[-5000:]),
                    pytrace=False)
    assert expect in out.stdout and "group ok" in out.stdout, out.stdout[-2000:]
    print(out.stdout)


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_sampler_equals_the_host_sampler(case):
    _run(["sampler", case], "sampler ok %s" % case)


def test_shortfall_is_reported_and_memory_safe():
    _run(["shortfall"], "shortfall ok")


@pytest.mark.parametrize("workload,parallel", [("C1", 1), ("C1", 0), ("C2", 1), ("C2", 0)])
def test_learner_trajectory_equals_host_sampling(workload, parallel):
    _run(["trajectory", workload, str(parallel)], "trajectory ok %s" % workload)
