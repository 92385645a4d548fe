"""What the post-fit suites share (test_gpu_{readout,linkpred,linkcomm,quality,cover,nmi,omega,relate,refsample}.py, their
*_child.py and the test_*_host.py beside them): the launcher of a child process and the child's dispatcher, the device
bench, the checkpoint parsing and comparison, bench.py's C1 learner with the "a call does not perturb the run" check, and
the runners of the C++ tests and the command-line driver.  A plain module: importing it needs neither torch nor the
built package; both are imported where a helper first uses them."""
import io
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PKG = os.path.join(ROOT, "mcmc-ammsb-gpu_amd")
GUARD = 64                      # words past every output that must stay untouched
WORKLOADS = {"C1": (10_000, 32, 1024, 32, 32, 32), "C2": (100_000, 256, 8192, 32, 32, 64)}   # bench.py's C1, C2


# ------------------------------------------------------------------ the launcher (pytest side) and the child's dispatcher

def run_group(child, args, expect, timeout):
    """One fresh process `python tests/<child> <args>`, from the repository root.  It must exit 0 and print both `expect`
    and the dispatcher's last line."""
    import pytest
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no fallback path exists)")
    out = subprocess.run([sys.executable, os.path.join(HERE, child)] + args, capture_output=True, text=True,
                         timeout=timeout, cwd=ROOT)
    if out.returncode != 0:
        pytest.fail("group %r (exit %d):\n%s\n%s" % (args, out.returncode, out.stdout[-2000:], out.stderr[-5000:]),
                    pytrace=False)
    assert expect in out.stdout and "group ok" in out.stdout, out.stdout[-2000:]
    print(out.stdout)


def child_main(groups, argv):
    """groups: name -> callable over the arguments after the name"""
    import __graft_entry__ as ge
    ge.build()
    if argv[0] not in groups:
        raise SystemExit("unknown group %r" % argv[0])
    groups[argv[0]](argv[1:])
    print("group ok", flush=True)


# ------------------------------------------------------------------ the device bench

class Raw:
    """a descriptor that is not a RowPartitionedMatrix: what a library call or an ops class needs of one"""

    def __init__(self, desc, cols, keep):
        self.desc, self.cols, self.keep = desc, cols, keep


class DeviceBench:
    def __init__(self):
        import torch
        from mcmc_ammsb_gpu_amd import ops
        self.torch, self.ops = torch, ops
        self.ctx = ops.Context(ops.make_params(1024, 32, E=1024))

    def matrix(self, host, rows_in_block=0):
        pi = self.ops.RowPartitionedMatrix(self.ctx, host.shape[0], host.shape[1], rows_in_block)
        pi.load(host)
        return pi

    def misaligned(self, host):
        """one block whose base is 4 bytes past a 16-byte boundary"""
        from mcmc_ammsb_gpu_amd._capi import Rpm
        buf = self.ctx.empty((host.size + 1,), self.torch.float32)
        buf[1:].copy_(self.ctx.from_numpy(host.reshape(-1)))
        d = Rpm()
        d.blocks[0] = buf.data_ptr() + 4
        assert d.blocks[0] % 16 == 4
        d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = host.shape[0], host.shape[0], host.shape[1], 1
        r = Raw(d, host.shape[1], buf)
        r.rows = host.shape[0]
        return r

    def guarded(self, words, dtype, fill, zero=False):
        """`words` words for a call to write, followed by GUARD words of `fill` that must survive it"""
        buf = self.ctx.empty((words + GUARD,), dtype)
        buf.fill_(fill)
        if zero:
            buf[:words].zero_()
        return buf

    def dev(self, a):
        return self.ctx.from_numpy(a)


# ------------------------------------------------------------------ checkpoints

def records(data):
    recs, pos = [], 0
    while pos < len(data):
        (n,) = struct.unpack_from("<Q", data, pos)
        recs.append(data[pos + 8:pos + 8 + n])
        pos += 8 + n
    assert pos == len(data)
    return recs


def pi_beta_of_checkpoint(data, N, K):
    recs = records(data)   # beta, theta, RpmProperties, the blocks of pi, ... (learner.cc:316-329)
    beta, raw = recs[0], recs[3]
    assert len(raw) >= N * K * 4 and len(recs[2]) < 64 and len(beta) >= 2 * K * 4
    return (np.frombuffer(raw[len(raw) - N * K * 4:], dtype=np.float32).reshape(N, K),
            np.frombuffer(beta[len(beta) - 2 * K * 4:], dtype=np.float32))


def sample_buffers(lrn):
    """records of the per-sample device buffers in Learner.Serialize's order (13 records precede the first Sample:
    beta, theta, pi's properties and block, phi, 2 + 3 operator records, 2 perplexity records, the learner's properties;
    a Sample is its message, dev_edges, dev_nodes, the neighbour streams, the neighbour data)"""
    assert lrn.trainingPerplexity is None and len(lrn.pi.blocks) == 1
    out, n = [], lrn.cfg.num_node_sample
    for i, s in enumerate(lrn.samples):
        base = 13 + 5 * i
        data = s.neighbor_sampler.GetData()
        out += [(base + 1, s.dev_edges.numel() * 8, s.n_edges * 8), (base + 2, s.dev_nodes.numel() * 4, s.n_nodes * 4),
                (base + 4, data.numel() * 4, s.n_nodes * n * 4)]
    return out


def same_buffers(a, b, what, partly):
    """Every buffer record byte for byte.  partly: [(record, bytes of the buffer, bytes the pending mini-batch holds)] for
    the per-sample device buffers, which are allocated uninitialised and written up to the mini-batch's size only: the
    bytes past it were never written by either run and are whatever the allocator handed out.  The short records carry
    accumulated wall times as varints (as in tests/test_gpu_pi_placement.py), whose LENGTH changes when a time crosses a
    power of 128 ns, so they are counted, not measured."""
    ra, rb = records(a), records(b)
    assert len(ra) == len(rb) and sum(len(x) >= 200 for x in ra) >= 6, what
    cut = {}
    for i, total, valid in partly:
        head = len(ra[i]) - total
        assert 2 <= head <= 11 and valid <= total, (what, i, len(ra[i]), total)
        cut[i] = head + valid
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert (len(x) >= 200) == (len(y) >= 200), (what, i)
        if len(x) >= 200:
            n = cut.get(i, len(x))
            assert len(x) == len(y) and x[:n] == y[:n], "%s: record %d (%d bytes) differs" % (what, i, len(x))


# ------------------------------------------------------------------ bench.py's C1 learner and the unperturbed run

def c1_learner(graph, workload="C1"):
    """-> (the data set of the workload, make): make() is a fresh Learner over it with device sampling and graph launch
    both `graph`; keyword arguments to make() replace those two settings"""
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd.learner import Config, Learner
    N, K, m, n, deg, k_true = WORKLOADS[workload]
    ds = hostlib.Dataset.robust(N, hostlib.generate_graph(N, k_true, deg, seed=20260101), heldout_ratio=0.01, rand_seed=1)

    def make(**cfg):
        cfg = cfg or dict(device_sampling=graph, graph_launch=graph)
        return Learner(Config.from_cli_defaults(K=K, mini_batch_size=m, num_node_sample=n, strategy="Node", **cfg), ds)
    return ds, make


def unperturbed_run(make, calls, what):
    """Run(20), calls(learner), Run(20) leaves the state Run(40) leaves: the sample sizes, the checkpoint buffers and the
    held-out perplexity.  -> the two checkpoints"""
    a, b = make(), make()
    a.Run(20)
    calls(a)
    a.Run(20)
    b.Run(40)
    ca, cb = io.BytesIO(), io.BytesIO()
    a.Serialize(ca)
    b.Serialize(cb)
    assert [(s.n_edges, s.n_nodes) for s in a.samples] == [(s.n_edges, s.n_nodes) for s in b.samples]
    same_buffers(ca.getvalue(), cb.getvalue(), "Run(20) + %s + Run(20) against Run(40)" % what, sample_buffers(a))
    assert a.HeldoutPerplexity() == b.HeldoutPerplexity()
    a.close()
    b.close()
    return ca.getvalue(), cb.getvalue()


# ------------------------------------------------------------------ smaller helpers

def rejects(exc_type, calls):
    """every call raises exc_type -> the exceptions"""
    caught = []
    for call in calls:
        try:
            call()
        except exc_type as e:
            caught.append(e)
        else:
            raise AssertionError("a bad argument was accepted")
    return caught


def run_cpp_test(name, workdir, timeout):
    """tests/cpp/<name>.cc as built into the package directory, over a directory for its files"""
    r = subprocess.run([os.path.join(PKG, name), workdir], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def run_ammsb_main(args, timeout, status=0):
    """the command-line driver; it must end with `status` -> the finished process"""
    r = subprocess.run([os.path.join(PKG, "ammsb_main")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == status, r.stderr[-3000:]
    return r


def exported_symbols(lib_path):
    """the functions a shared library defines and exports, the runtime's own left out"""
    nm = next((p for p in ("/usr/bin/nm", "/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None)
    assert nm, "no nm / llvm-nm to list the library's symbols"
    out = subprocess.run([nm, "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in ("T", "t")}
    return {s for s in exported if not s.startswith(("_init", "_fini", "__hip", "_ZSt", "_ZNSt", "_ZNKSt"))}
