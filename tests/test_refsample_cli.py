"""`ammsb_main --sampling-stream reference` (the C++ mcmc::Learner with Config::sampling_stream): the flag table and the
refused combinations without a GPU; on the GPU the same perplexity lines as host sampling from the same seeds, in the
synchronous loop and under --async, and a checkpoint of either mode resumed in the other."""
import os
import re
import subprocess

import pytest

import test_cli as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as ge
    ge.build()
    assert os.path.exists(tc.EXE)
    return tc.EXE


def test_help_lists_the_flag(exe):
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    line = [ln for ln in out.stdout.splitlines() if "--sampling-stream arg" in ln]
    assert len(line) == 1 and "(=own" in line[0] and "reference" in line[0] and "--graph" in line[0], out.stdout


def test_refused_combinations(exe, tmp_path):
    g = tmp_path / "g.txt"
    g.write_text("#\n#\n#\n#\n0\t1\n")
    base = [exe, "-f", str(g)]
    r = subprocess.run(base + ["--device-sampling", "1", "--async", "1", "--graph", "1", "--sampling-stream", "reference"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--sampling-stream reference cannot be combined with --graph 1" in r.stderr
    r = subprocess.run(base + ["--sampling-stream", "reference"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "needs --device-sampling 1" in r.stderr
    r = subprocess.run(base + ["--sampling-stream", "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "invalid" in r.stderr


def _lines(stderr):
    """the perplexity lines as printed (text, not parsed numbers: equal means equal to the last digit shown)"""
    return re.findall(r"ppx\[\d+\] = \S+", stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["Node", "NodeNonLink"])
def test_same_perplexity_lines_as_host_sampling(exe, tmp_path, strategy):
    g, d = str(tmp_path / "g.txt"), str(tmp_path / "g.bin.gz")
    tc._snap_file(g, N=12000, deg=16)
    r = subprocess.run([exe, "-f", g, "--dump-data", "1", "--dump-file", d, "-r", "0.05"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    common = ["--load-data", "1", "--load-file", d, "-k", "32", "-m", "256", "-n", "16", "-s", strategy,
              "--phi-wg", "32", "--beta-wg", "32", "--ppx-wg", "32", "--sample-seed0", "12345", "--sample-seed1", "678910"]
    ref = ["--device-sampling", "1", "--sampling-stream", "reference"]

    def run(extra, name):
        out = subprocess.run([exe] + common + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, "%s:\n%s" % (name, out.stderr[-3000:])
        return out.stderr
    host = run(["-x", "150", "-i", "50"], "host sampling")
    want = _lines(host)
    assert len(want) == 4 and want[0] != want[-1]
    assert "sampling_stream: own" in host
    sync = run(["-x", "150", "-i", "50"] + ref, "reference stream")
    assert "sampling_stream: reference" in sync
    assert _lines(sync) == want, "synchronous loop"
    assert _lines(run(["-x", "150", "-i", "50", "--async", "1"] + ref, "reference stream --async")) == want, "--async"
    # a checkpoint of either mode resumed in the other: the same lines as the same mode's own resume
    ck_h, ck_r = str(tmp_path / "host.ckpt"), str(tmp_path / "ref.ckpt")
    a = run(["-x", "100", "-i", "50", "--checkpoint-out", ck_h], "host, checkpoint")
    b = run(["-x", "100", "-i", "50", "--checkpoint-out", ck_r] + ref, "reference, checkpoint")
    assert _lines(a) == _lines(b) == want[:3]
    hh = _lines(run(["-x", "50", "-i", "50", "--checkpoint-in", ck_h], "host resumes host"))
    assert len(hh) == 2
    assert _lines(run(["-x", "50", "-i", "50", "--checkpoint-in", ck_h] + ref, "reference resumes host")) == hh
    assert _lines(run(["-x", "50", "-i", "50", "--checkpoint-in", ck_r], "host resumes reference")) == hh
    assert _lines(run(["-x", "50", "-i", "50", "--checkpoint-in", ck_r, "--async", "1"] + ref, "async reference resumes")) == hh
