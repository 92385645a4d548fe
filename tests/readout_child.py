"""Child process of test_gpu_readout.py (one per group): the read-out of pi (include/ammsb_readout.h,
ops.CommunityReadout, Learner.Memberships / CommunitySizes / Communities, mcmc::Learner::Memberships,
ammsb_main --communities-out) against a numpy statement, exactly: ids, count and sizes as integers, weights by bit
pattern.  No tolerance appears anywhere."""
import os
import struct
import sys
import tempfile

import numpy as np

import postfit_support as ps

NONE = 0xFFFFFFFF
KS = (1, 3, 48, 64, 113, 256, 512, 1024, 2048, 4096, 8192)
TS = (1, 4, 16)
ROWS = (1, 63, 65, 5000)


def sort_order(pi):
    """a stable sort of -row is "value descending, column ascending" (the first 20 are all any T and threshold here need)"""
    return np.argsort(-np.asarray(pi, dtype=np.float32), axis=1, kind="stable")[:, :20].copy()


def expected(pi, T, thr, order=None):
    """The contract as a numpy statement (order: sort_order(pi), when the caller asks about the same pi repeatedly)."""
    pi = np.asarray(pi, dtype=np.float32)
    n, K = pi.shape
    thr = np.float32(thr)
    order = (sort_order(pi) if order is None else order)[:, :T]
    vals = np.take_along_axis(pi, order, axis=1)
    keep = vals >= thr
    ids = np.full((n, T), NONE, dtype=np.uint32)
    weights = np.zeros((n, T), dtype=np.float32)
    ids[:, :order.shape[1]][keep] = order[keep]
    weights[:, :order.shape[1]][keep] = vals[keep]
    return ids, weights, (pi >= thr).sum(1).astype(np.uint32), (pi >= thr).sum(0).astype(np.int64)


def same(got, want, what):
    ids, weights, count = (g.cpu().numpy() for g in got[:3])
    wi, ww, wc = want[:3]
    assert np.array_equal(ids.view(np.uint32), wi), "%s: ids differ at rows %s" % (
        what, np.nonzero((ids.view(np.uint32) != wi).any(1))[0][:8])
    assert np.array_equal(weights.view(np.uint32), ww.view(np.uint32)), "%s: weights differ" % what
    assert np.array_equal(count.view(np.uint32), wc), "%s: count differs" % what
    if len(got) > 3:
        assert np.array_equal(got[3].cpu().numpy(), want[3]), "%s: sizes differ" % what


def form_for(K):
    if K % 256:
        return "readout_generic"
    nv = K // 256
    return "readout_fast<%d>" % next(v for v in (1, 2, 4, 8, 16, 32) if nv <= v)


def draw(rng, n, K, kind):
    """fitted rows (a few large entries), flat rows, or a mix; float32, rows normalised as update_pi leaves them"""
    if kind == "fitted":
        g = rng.gamma(1.0 / K, 1.0, (n, K))
    elif kind == "flat":
        g = rng.gamma(1.0, 1.0, (n, K))
    else:
        g = np.where(rng.random((n, 1)) < 0.5, rng.gamma(1.0 / K, 1.0, (n, K)), rng.gamma(1.0, 1.0, (n, K)))
    g = np.maximum(g, 1e-24).astype(np.float32)
    return (g / g.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


class Bench(ps.DeviceBench):
    def __init__(self):
        super().__init__()
        self.ro = self.ops.CommunityReadout(self.ctx)

    def run(self, pi, T, thr, **kw):
        sizes = self.ctx.zeros((pi.cols,), self.torch.int64)
        got = self.ro.top(pi, T, thr, sizes=sizes, **kw)
        self.torch.cuda.synchronize()
        return got + (sizes,)


def thresholds(host, T, order):
    """0; exactly a stored value (the >= side); above every entry; one that leaves more than T columns where K allows"""
    K = host.shape[1]
    desc = np.take_along_axis(host, order, axis=1)   # each row's largest values, descending
    out = [0.0, float(desc[0, min(1, K - 1)]), float(np.nextafter(host.max(), np.float32(2)))]
    if K > T:
        out.append(float(desc[:, min(K - 1, T + 2, desc.shape[1] - 1)].min()))
    return out


def shapes_group(which):
    b = Bench()
    rng = np.random.default_rng(11)
    ks = KS if which == "all" else [int(which)]
    n_checks = 0
    for K in ks:
        for n in ROWS:
            for kind in ("fitted", "flat", "mix"):
                if kind != "mix" and n != 5000:
                    continue
                host = draw(rng, n, K, kind)
                pi = b.matrix(host)
                order = sort_order(host)
                for T in TS:
                    for thr in thresholds(host, T, order):
                        want = expected(host, T, thr, order)
                        got = b.run(pi, T, thr)
                        assert b.ro.kernel_name() == form_for(K), (K, b.ro.kernel_name())
                        same(got, want, "K=%d rows=%d %s T=%d thr=%g" % (K, n, kind, T, thr))
                        if thr > host.max():
                            assert (want[0] == NONE).all() and not want[2].any() and not want[3].any()
                        if thr and K > T and thr <= np.take_along_axis(host, order, axis=1)[:, T].min():
                            assert (want[2] > T).all()     # the case really leaves more than T columns
                        n_checks += 1
                # sizes alone (nothing else written)
                sz = b.ro.sizes(pi, float(host[0, 0]))
                assert np.array_equal(sz.cpu().numpy(), (host >= host[0, 0]).sum(0))
        print("shapes ok K=%d (%s)" % (K, form_for(K)), flush=True)
    print("shapes ok %s: %d comparisons" % (which, n_checks), flush=True)


def layout_group():
    b = Bench()
    rng = np.random.default_rng(12)
    for K in (256, 113):
        n = 5000
        host = draw(rng, n, K, "mix")
        thr = float(np.float32(2.0 / K))
        want = expected(host, 4, thr)
        for rib in (0, 2500, 431):   # one block, two blocks, eleven blocks + a ragged twelfth
            pi = b.matrix(host, rib)
            assert len(pi.blocks) == {0: 1, 2500: 2, 431: 12}[rib]
            same(b.run(pi, 4, thr), want, "K=%d rows_in_block=%d" % (K, rib))
            # row slabs that start and end inside a block; sizes accumulate across the calls
            sizes = b.ctx.zeros((K,), b.torch.int64)
            lo = 0
            for hi in (17, 500, 2501, 2600, 4999, 5000):
                got = b.ro.top(pi, 4, thr, rows=(lo, hi), sizes=sizes)
                same(got, tuple(w[lo:hi] for w in want[:3]), "K=%d rows_in_block=%d slab %d..%d" % (K, rib, lo, hi))
                lo = hi
            assert np.array_equal(sizes.cpu().numpy(), want[3])
            # a node list: descending, with repeats (a repeated node counts twice in sizes)
            nodes = np.concatenate([np.arange(n - 1, 0, -7), [5, 5, 5, n - 1, 0, 0]]).astype(np.uint32)
            wn = expected(host[nodes], 4, thr)
            same(b.run(pi, 4, thr, nodes=nodes), wn, "K=%d rows_in_block=%d node list" % (K, rib))
        print("layout ok K=%d" % K, flush=True)
    print("layout ok", flush=True)


def ties_group():
    b = Bench()
    rng = np.random.default_rng(13)
    for K in (48, 113, 256, 1024, 2048):
        rows = []
        rows.append(np.full(K, np.float32(1.0) / np.float32(K), dtype=np.float32))     # uniform: ids 0 .. T-1
        rows.append(np.full(K, np.float32(1e-24), dtype=np.float32))                    # the whole row at the floor
        base = draw(rng, 1, K, "flat")[0] * np.float32(0.5)
        top = np.float32(0.25)

        def with_max(cols):
            r = base.copy()
            r[list(cols)] = top
            return r
        if K % 256 == 0:
            rows.append(with_max((8, 9)))              # two columns of one lane (lane 2, components 0 and 1)
            rows.append(with_max((9, 8 + 256 * (K // 256 - 1))) if K > 256 else with_max((9, 10)))  # one lane, two pieces
            rows.append(with_max((201, 13)))           # different lanes
            rows.append(with_max((K - 1, 300 % K, 7)))  # different lanes and 256-column pieces
        else:
            rows.append(with_max((5, 5 + 64 if K > 69 else 6)))   # one lane of the generic form (columns l, l + 64)
            rows.append(with_max((K - 1, 3)))
            rows.append(with_max((40, 41, 42)))
        rows.append(with_max(range(0, K, 5)))          # many holders: more ties than T
        host = np.stack(rows)
        pi = b.matrix(host)
        for T in TS:
            for thr in (0.0, float(top), float(np.float32(1e-24)), float(np.float32(1.0) / np.float32(K))):
                want = expected(host, T, thr)
                same(b.run(pi, T, thr), want, "ties K=%d T=%d thr=%g" % (K, T, thr))
        w = expected(host, 16, 0.0)[0]
        assert np.array_equal(w[0, :min(16, K)], np.arange(min(16, K)))
        print("ties ok K=%d" % K, flush=True)
    print("ties ok", flush=True)


def big_group():
    """K = 8192 and a little over 2^32 elements in ONE block: the last rows are only reachable with 64-bit offsets.  Then
    the same values in a block whose base is 4 bytes past a 16-byte boundary, which takes the generic form: the same
    outputs"""
    b = Bench()
    torch = b.torch
    K, n = 8192, 524288 + 4096
    assert n * K > 1 << 32
    step = 32768

    def fill(blk):
        gen = torch.Generator(device=blk.device)
        gen.manual_seed(5)
        for lo in range(0, n, step):   # values >= 0, a few large ones per row (u^64), rows not normalised: any finite >= 0
            blk[lo:lo + step].copy_(torch.rand((min(step, n - lo), K), generator=gen, device=blk.device).pow_(64))

    pi, blk = b.zeroed(n, K)
    fill(blk)
    thr, T = 0.25, 4
    sizes = b.ctx.zeros((K,), torch.int64)
    tail = 4096
    got = b.ro.top(pi, T, thr, rows=(n - tail, n))
    torch.cuda.synchronize()
    assert b.ro.kernel_name() == "readout_fast<32>"
    host_tail = blk[n - tail:].cpu().numpy()
    same(got, expected(host_tail, T, thr), "beyond 2^32 elements: last %d rows" % tail)
    nodes = np.array([n - 1, n - 2, 0, n - 4096], dtype=np.uint32)
    listed = b.ro.top(pi, 16, 0.0, nodes=nodes)
    same(listed, expected(blk[torch.from_numpy(nodes.astype(np.int64)).to(blk.device)].cpu().numpy(), 16, 0.0),
         "beyond 2^32 elements: node list")
    b.ro.sizes(pi, thr, out=sizes)
    want = np.zeros(K, dtype=np.int64)
    for lo in range(0, n, step):
        want += (blk[lo:lo + step].cpu().numpy() >= np.float32(thr)).sum(0)
    assert np.array_equal(sizes.cpu().numpy(), want), "sizes over %d rows" % n
    del pi, blk
    b.release()
    mis, blk = b.zeroed(n, K, misaligned=True)
    fill(blk)
    assert np.array_equal(blk[n - tail:].cpu().numpy(), host_tail)
    got2 = b.ro.top(mis, T, thr, rows=(n - tail, n))
    assert b.ro.kernel_name() == "readout_generic"
    listed2 = b.ro.top(mis, 16, 0.0, nodes=nodes)
    assert b.ro.kernel_name() == "readout_generic"
    sizes2 = b.ro.sizes(mis, thr)
    assert b.ro.kernel_name() == "readout_generic"
    for x, y in zip(got + listed + (sizes,), got2 + listed2 + (sizes2,)):
        assert torch.equal(x, y), "the generic form's outputs differ from the fast form's"
    print("big ok: %d x %d (%.1f GB), sizes sum %d" % (n, K, n * K * 4 / 1e9, int(want.sum())), flush=True)


def learner_group(graph):
    import torch
    from mcmc_ammsb_gpu_amd import _readout
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    assert (lrn.loop is not None) == graph
    lrn.Run(30)
    for top, thr in ((4, 0.0), (4, 0.05), (16, 0.01), (1, 0.5)):
        sizes = lrn.ctx.zeros((K,), torch.int64)
        got = lrn.Memberships(top, thr, sizes=sizes)
        host = lrn.pi.host()
        want = expected(host, top, thr)
        same(got + (sizes,), want, "Memberships top=%d thr=%g" % (top, thr))
        assert np.array_equal(lrn.CommunitySizes(thr).cpu().numpy(), want[3])
        off, mem = lrn.Communities(top, thr)
        woff, wmem = _readout.communities_csr(want[0], K)
        assert np.array_equal(off, woff) and np.array_equal(mem, wmem)
        for k in range(K):   # the definition, spelled out: nodes whose slots hold k, ascending
            assert np.array_equal(mem[off[k]:off[k + 1]], np.nonzero((want[0] == k).any(1))[0])
    nodes = np.array([N - 1, 3, 3, 0, 77], dtype=np.uint32)
    same(lrn.Memberships(4, 0.05, nodes=nodes), expected(lrn.pi.host()[nodes], 4, 0.05), "Memberships of a node list")
    # slabs: a budget that cuts N into many calls gives the same tables
    lrn.READOUT_SLAB_BYTES = 36 * 1000
    sizes = lrn.ctx.zeros((K,), torch.int64)
    same(lrn.Memberships(4, 0.05, sizes=sizes) + (sizes,), expected(lrn.pi.host(), 4, 0.05), "Memberships in slabs")
    same(lrn.Memberships(4, 0.05, nodes=np.arange(N - 1, -1, -1, dtype=np.uint32)),
         expected(lrn.pi.host()[::-1], 4, 0.05), "Memberships of a node list in slabs")
    lrn.close()
    # Run(20), read-out, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.Memberships(4, 0.05)
        a.CommunitySizes(0.05)
        a.Communities(2, 0.1)
    ca, cb = ps.unperturbed_run(make, calls, "read-out")
    assert [len(x) for x in ps.records(ca)] == [len(y) for y in ps.records(cb)]   # the short records included
    print("learner ok graph=%s" % graph, flush=True)


def cpp_group():
    from mcmc_ammsb_gpu_amd import _readout, hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("readout_test", d, 900)
        # bit-level cross-host check through the checkpoint: pi parsed here, the numpy statement applied
        raw = open(os.path.join(d, "memberships.bin"), "rb").read()
        N, K, top = struct.unpack_from("<III", raw, 0)
        (thr,) = struct.unpack_from("<f", raw, 12)
        pos = 16
        ids = np.frombuffer(raw, np.uint32, N * top, pos).reshape(N, top)
        pos += N * top * 4
        weights = np.frombuffer(raw, np.float32, N * top, pos).reshape(N, top)
        pos += N * top * 4
        count = np.frombuffer(raw, np.uint32, N, pos)
        pos += N * 4
        sizes = np.frombuffer(raw, np.uint64, K, pos)
        assert pos + 8 * K == len(raw)
        pi = ps.pi_beta_of_checkpoint(open(os.path.join(d, "cpp.ckpt"), "rb").read(), N, K)[0]
        wi, ww, wc, ws = expected(pi, top, thr)
        assert np.array_equal(ids, wi) and np.array_equal(weights.view(np.uint32), ww.view(np.uint32))
        assert np.array_equal(count, wc) and np.array_equal(sizes.astype(np.int64), ws)
        fN, fK, ftop, fthr, fsizes, off, mem = _readout.read_communities(os.path.join(d, "communities.txt"))
        assert (fN, fK, ftop) == (N, K, top) and np.float32(fthr) == np.float32(thr)
        woff, wmem = _readout.communities_csr(wi, K)
        assert np.array_equal(fsizes, ws) and np.array_equal(off, woff) and np.array_equal(mem, wmem)
        print("cpp ok: Learner::Memberships equals the numpy statement over the checkpoint's pi", flush=True)
        # the command-line driver on a small generated graph
        N = 6000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck = os.path.join(d, "comm.txt"), os.path.join(d, "main.ckpt")
        for extra, top, thr in (([], 4, 0.0), (["--membership-top", "2", "--membership-threshold", "0.1"], 2, 0.1)):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f, "-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30",
                               "--communities-out", out, "--checkpoint-out", ck] + extra, 600)
            fN, fK, ftop, fthr, fsizes, off, mem = _readout.read_communities(out)
            assert (fN, fK, ftop) == (N, 48, top) and np.float32(fthr) == np.float32(thr)
            per_node = np.bincount(mem, minlength=N)
            assert per_node.max() <= top and mem.size > 0
            for k in range(48):
                mk = mem[off[k]:off[k + 1]]
                assert fsizes[k] >= mk.size and (np.diff(mk) > 0).all() and (mk.size == 0 or (0 <= mk[0] and mk[-1] < N))
            # ... and against the pi of the checkpoint written by the same process
            wi, _, _, ws = expected(ps.pi_beta_of_checkpoint(open(ck, "rb").read(), N, 48)[0], top, thr)
            woff, wmem = _readout.communities_csr(wi, 48)
            assert np.array_equal(fsizes, ws) and np.array_equal(off, woff) and np.array_equal(mem, wmem)
        print("cli ok", flush=True)


GROUPS = {
    "shapes": lambda a: shapes_group(a[0]),
    "layout": lambda a: layout_group(),
    "ties": lambda a: ties_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
