"""What the post-fit suites share (test_gpu_{readout,linkpred,linkcomm,quality,cover,nmi,omega,relate,refsample}.py, their
*_child.py and the test_*_host.py beside them): the launcher of a child process and the child's dispatcher, the device
bench, the fixture of a pi whose last rows lie past element 2^32, the checkpoint parsing and comparison, bench.py's C1
learner with the "a call does not perturb the run" check, and the runners of the C++ tests and the command-line driver.
A plain module: importing it needs neither torch nor the built package; both are imported where a helper first uses
them."""
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


# ------------------------------------------------------------------ pi past element 2^32: the pure part of the fixture
#
# K = 8192 is the largest K the post-fit libraries accept, and 2^32 / 8192 = 2^19 is the first row whose element offset
# needs 33 bits: BIG_ROWS x BIG_K is the smallest shape in which a product kept in 32 bits reads another row.  All of pi is
# zero but four windows of rows (640 in all), so the numpy statement over those rows alone (in "compact" numbering: the
# position of a row in big_ids()) equals the statement over the whole matrix at any threshold above 0.

BIG_K = 8192
BIG_ROWS = (1 << 19) + 128
BIG_ZERO_ROWS = (128, (1 << 17) - 65, (1 << 18) + 64, (1 << 19) - 129)   # valid rows next to a window that hold no member


def big_windows():
    """[0, 128): what a wrapped element offset of the last 128 rows reads; then the rows that straddle byte offset 2^32,
    element 2^31 (where a signed 32-bit index fails) and element 2^32"""
    return ((0, 128), ((1 << 17) - 64, (1 << 17) + 64), ((1 << 18) - 64, (1 << 18) + 64), ((1 << 19) - 128, BIG_ROWS))


def big_ids():
    """-> the 640 planted rows, ascending"""
    return np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in big_windows()])


def big_alias(rows, K=BIG_K):
    """the row that an element offset row * K kept in 32 bits falls into"""
    return (np.asarray(rows, dtype=np.int64) * K % (1 << 32)) // K


def big_positions(rows, zero_rows=BIG_ZERO_ROWS):
    """global rows -> compact positions: a planted row to its place in big_ids(), zero_rows[j] to 640 + j, a row >=
    BIG_ROWS to one >= 640 + len(zero_rows) (invalid before, invalid after, at most 2^32 - 1); any other row is refused"""
    rows = np.asarray(rows, dtype=np.int64)
    ids = np.concatenate([big_ids(), np.asarray(zero_rows, dtype=np.int64)])
    order = np.argsort(ids, kind="stable")
    at = np.minimum(np.searchsorted(ids[order], rows), ids.size - 1)
    known = ids[order][at] == rows
    past = rows >= BIG_ROWS
    if not (known | past).all():
        raise ValueError("rows %s are neither planted nor listed as zero rows" % rows[~(known | past)][:8])
    return np.where(known, order[at], np.minimum(rows - BIG_ROWS + ids.size, 0xFFFFFFFF))


def big_remap(keys, zero_rows=BIG_ZERO_ROWS):
    """keys (a << 32) | b over global rows -> the same keys over compact positions"""
    keys = np.asarray(keys, dtype=np.uint64)
    a, b = big_positions(keys >> np.uint64(32), zero_rows), big_positions(keys & np.uint64(0xFFFFFFFF), zero_rows)
    return (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def big_extended(compact, zero_rows=BIG_ZERO_ROWS):
    """the compact rows followed by one zero row per entry of zero_rows: what big_positions() numbers"""
    return np.concatenate([compact, np.zeros((len(zero_rows), compact.shape[1]), compact.dtype)])


def big_wrapped(compact):
    """the compact rows as a kernel sees them that keeps row * K in 32 bits: every row >= 2^19 reads its alias in [0, 128)"""
    ids = big_ids()
    out = compact.copy()
    out[ids >= (1 << 19)] = compact[big_positions(big_alias(ids[ids >= (1 << 19)]))]
    return out


def big_threshold(compact, per_row=40):
    """the stored value that leaves about per_row memberships per planted row; above 0, so a zero row has no member"""
    thr = float(np.sort(compact.reshape(-1))[-per_row * compact.shape[0]])
    assert thr > 0
    return thr


def big_keys(seed, per_pair=280, zero_rows=BIG_ZERO_ROWS):
    """a few thousand keys (a << 32) | b, ends in either order: per_pair keys for every two windows and for every window
    with itself, of which the pairs that involve the last window take half their ends from the rows >= 2^19; then about a
    twentieth each self loops, repeats of earlier keys and keys with an end >= BIG_ROWS (BIG_ROWS itself, a little past it,
    2^32 - 1); then four keys per zero row, one of them between two zero rows"""
    rng = np.random.default_rng(seed)
    wins = big_windows()
    a, b = [], []
    for i, (lo, hi) in enumerate(wins):
        for lo2, hi2 in wins[i:]:
            u, v = rng.integers(lo, hi, per_pair), rng.integers(lo2, hi2, per_pair)
            if hi2 == BIG_ROWS:
                v[::2] = rng.integers(1 << 19, BIG_ROWS, v[::2].size)
            swap = rng.random(per_pair) < 0.5
            a.append(np.where(swap, v, u))
            b.append(np.where(swap, u, v))
    a, b = np.concatenate(a).astype(np.uint64), np.concatenate(b).astype(np.uint64)
    n = a.size
    loops = rng.random(n) < 0.05
    b[loops] = a[loops]
    bad = rng.random(n) < 0.05
    past = rng.choice(np.array([BIG_ROWS, BIG_ROWS + 5, 2 ** 32 - 1], dtype=np.uint64), n)
    side = rng.random(n) < 0.5
    a[bad & side] = past[bad & side]
    b[bad & ~side] = past[bad & ~side]
    keys = (a << np.uint64(32)) | b
    for i in np.flatnonzero(rng.random(n) < 0.05):
        if i:
            keys[i] = keys[rng.integers(0, i)]
    ids = big_ids()
    extra = []
    for j, z in enumerate(zero_rows):
        other = [int(ids[-1 - j]), int(ids[j]), int(ids[300 + j]), int(zero_rows[(j + 1) % len(zero_rows)])]
        extra += [(z << 32) | other[0], (other[1] << 32) | z, (z << 32) | other[2], (z << 32) | other[3]]
    return np.concatenate([keys, np.array(extra, dtype=np.uint64)])


def big_csr(keys, n):
    """keys over n nodes -> (offsets [n + 1] uint64, targets uint32): per key b in a's row where a < n and a in b's row
    where b < n, so a row holds the ends >= n of its keys as targets (a key with both ends >= n is in no row); rows by
    node, the targets of a row in the order of the keys"""
    keys = np.asarray(keys, dtype=np.uint64)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    keep = src < n
    src, dst = src[keep], dst[keep]
    order = np.argsort(src, kind="stable")
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=n))
    return off, dst[order].astype(np.uint32)


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

    def zeroed(self, n, K, misaligned=False):
        """n x K zeros in one block, allocated and zeroed on the device (nothing of it passes through host memory)
        -> (what a library call takes for pi, the block's [n, K] tensor).  misaligned: the block's base is 4 bytes past a
        16-byte boundary, which is what misaligned() does for a host array"""
        if not misaligned:
            pi = self.ops.RowPartitionedMatrix(self.ctx, n, K)
            pi.blocks[0].zero_()
            return pi, pi.blocks[0]
        from mcmc_ammsb_gpu_amd._capi import Rpm
        buf = self.ctx.empty((n * K + 1,), self.torch.float32)
        buf.zero_()
        d = Rpm()
        d.blocks[0] = buf.data_ptr() + 4
        assert d.blocks[0] % 16 == 4
        d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = n, n, K, 1
        r = Raw(d, K, buf)
        r.rows = n
        return r, buf[1:].view(n, K)

    def big_pi(self, seed, misaligned=False):
        """BIG_ROWS x BIG_K floats in one block (2^32 + 2^20 elements, 17.2 GB), zero but for the 640 rows of
        big_windows(), which are filled on the device: a few large entries per row (u^64), row-normalised, from a generator
        seeded with `seed` (the same seed gives the same rows, aligned or not)
        -> (pi, the planted rows as a host array [640, BIG_K] in the order of big_ids(), big_ids())"""
        torch = self.torch
        pi, blk = self.zeroed(BIG_ROWS, BIG_K, misaligned)
        gen = torch.Generator(device=blk.device)
        gen.manual_seed(seed)
        ids = big_ids()
        r = torch.rand((ids.size, BIG_K), generator=gen, device=blk.device).pow_(64).clamp_(min=1e-24)
        r.div_(r.sum(1, keepdim=True))
        at = 0
        for lo, hi in big_windows():
            blk[lo:hi].copy_(r[at:at + hi - lo])
            at += hi - lo
        compact = torch.cat([blk[lo:hi] for lo, hi in big_windows()]).cpu().numpy()
        assert np.array_equal(compact, r.cpu().numpy()) and (compact.sum(1) > 0.5).all()
        return pi, compact, ids

    def release(self):
        """after the caller dropped its own names of a block: give the freed memory back to the device, so that the next
        17 GB block is the only one alive"""
        import gc
        gc.collect()
        self.torch.cuda.empty_cache()

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
