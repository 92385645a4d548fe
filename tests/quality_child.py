"""Child process of test_gpu_quality.py (one per group): scoring communities against a graph
(include/ammsb_quality.h, ops.CommunityQuality, Learner.CommunityQuality / SharedCommunities) against the numpy
statement, every figure exactly equal:

    M = pi >= np.float32(thr);  both = M[a] & M[b];  one = M[a] ^ M[b]
    internal = both.sum(0), boundary = one.sum(0) over the valid edges;  shared = both.sum(1), -1 for an invalid edge
    uncovered = the valid edges with shared == 0;  skipped = the edges with an end >= N"""
import ctypes as C
import io
import os
import sys

import numpy as np

import postfit_support as ps

NONE = 0xFFFFFFFF
SEEN = set()
F32 = np.float32
PLANTED = F32(0.125)                                   # a planted value: a threshold equal to its bits keeps it
BELOW = np.nextafter(PLANTED, F32(0), dtype=F32)       # the next float below: not a member at that threshold
ABOVE = 2.0                                            # above every value of a row
U32 = np.uint64(32)


def planted_cols(K):
    """columns of the planted values: neighbours in a 16-byte load, the same lane of the next load, another word"""
    k0 = 2 if K > 8 else 0
    return np.array(sorted({k for k in (k0, k0 + 1, k0 + 4, k0 + 64, k0 + 256, K - 1) if k < K}), dtype=np.int64)


def draw_rows(rng, n, K):
    """a sixth each: fitted-looking rows (Dirichlet alpha = 1/K), flat rows (1/64 everywhere), one-hot rows, fitted rows
    with NaNs in them, rows with PLANTED on planted_cols(K), and rows with the next float below PLANTED there"""
    kind = np.arange(n) % 6
    rng.shuffle(kind)
    fitted = np.maximum(rng.gamma(1.0 / K, 1.0, (n, K)), 1e-24)
    fitted /= fitted.sum(1, keepdims=True)
    fitted = fitted.astype(F32)
    flat = np.full((n, K), 1.0 / 64, dtype=F32)
    onehot = np.zeros((n, K), dtype=F32)
    onehot[np.arange(n), rng.integers(0, K, n)] = 1.0
    nans = fitted.copy()
    nans[rng.random((n, K)) < 0.25] = np.nan
    nans[:, 0] = np.nan
    planted = (fitted * F32(0.01)).astype(F32)
    below = planted.copy()
    planted[:, planted_cols(K)] = PLANTED
    below[:, planted_cols(K)] = BELOW
    rows = np.choose(kind[:, None], [fitted, flat, onehot, nans, planted, below]).astype(F32)
    return rows, kind


def draw_edges(rng, N, n, kind=None):
    u, v = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
    if kind is not None and n >= 200:     # some edges inside one kind of rows, and planted against below
        for kd in range(6):
            rows = np.flatnonzero(kind == kd)
            at = slice(20 * kd, 20 * kd + 20)
            u[at], v[at] = rng.choice(rows, 20), rng.choice(rows, 20)
        u[120:140], v[120:140] = rng.choice(np.flatnonzero(kind == 4), 20), rng.choice(np.flatnonzero(kind == 5), 20)
        u[140:150], v[140:150] = u[:10], v[:10]          # duplicates
        u[150:160], v[150:160] = v[:10], u[:10]          # ... and in the other order
    if n >= 3:
        u[-1] = v[-1]                     # a == b
    if n >= 200:
        u[-2] = N                         # an end == N
        v[-3] = NONE                      # an end == 2^32 - 1
        u[-4], v[-4] = NONE, NONE
        u[-5] = u[-6] = v[-6]             # a == b again, next to an ordinary edge
    return (u << U32) | v


def ends(edges):
    return (edges >> U32).astype(np.int64), (edges & np.uint64(NONE)).astype(np.int64)


def reference(pi, thr, edges):
    """-> counts [2K + 2] int64 (internal, boundary, uncovered, skipped), shared [n] int32"""
    N, K = pi.shape
    with np.errstate(invalid="ignore"):
        M = pi >= F32(thr)
    u, v = ends(edges)
    valid = (u < N) & (v < N)
    counts = np.zeros(2 * K + 2, dtype=np.int64)
    shared = np.full(edges.size, -1, dtype=np.int32)
    idx = np.flatnonzero(valid)
    for lo in range(0, idx.size, 2048):
        sel = idx[lo:lo + 2048]
        both, one = M[u[sel]] & M[v[sel]], M[u[sel]] ^ M[v[sel]]
        counts[:K] += both.sum(0)
        counts[K:2 * K] += one.sum(0)
        shared[sel] = both.sum(1)
    counts[2 * K] = (shared[valid] == 0).sum()
    counts[2 * K + 1] = (~valid).sum()
    # the identity: 2 internal + boundary = the members' degrees in the list, summed (a == b counts twice at its node)
    deg = np.bincount(u[valid], minlength=N) + np.bincount(v[valid], minlength=N)
    assert np.array_equal(2 * counts[:K] + counts[K:2 * K], deg @ M.astype(np.int64)), "the reference breaks its identity"
    return counts, shared


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _quality
        super().__init__()
        self.q = _quality
        self.lib = _quality.load()
        self.api = self.ops.CommunityQuality(self.ctx)

    def mask(self, pi, thr):
        """the library call over a workspace of this test's own, followed by GUARD words that must survive
        -> the mask, a device tensor of exactly ammsb_quality_mask_bytes / 8 words"""
        t = self.torch
        N, K = int(pi.desc.num_rows), int(pi.cols)
        words = int(self.lib.ammsb_quality_mask_bytes(N, K)) // 8
        assert words == N * ((K + 63) // 64)
        buf = self.guarded(words, t.int64, 0x5A5A5A5A5A5A)
        self.q.check(self.lib.ammsb_quality_mask(C.byref(pi.desc), thr, C.c_void_p(buf.data_ptr()), None))
        t.cuda.synchronize()
        SEEN.add(self.q.last_kernel_name())
        assert (buf[words:] == 0x5A5A5A5A5A5A).all().item(), "the words past the mask were written"
        return buf[:words]

    def edges(self, mask, N, K, edges, counts=True, shared=True):
        """-> (counts [2K + 2] int64 or None, shared [n] int32 or None) as numpy arrays"""
        t = self.torch
        n = int(edges.size)
        d_edges = self.ctx.from_numpy(np.ascontiguousarray(edges, dtype=np.uint64))
        cnt = self.guarded(2 * K + 2, t.int64, 0x5A5A5A5A5A5A, zero=True) if counts else None
        sh = self.guarded(n, t.int32, 0x5A5A5A5A) if shared else None
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
        self.q.check(self.lib.ammsb_quality_edges(ptr(mask), N, K, ptr(d_edges), n, ptr(cnt), ptr(sh), None))
        t.cuda.synchronize()
        SEEN.add(self.q.last_kernel_name())
        out = []
        for buf, words, fill in ((cnt, 2 * K + 2, 0x5A5A5A5A5A5A), (sh, n, 0x5A5A5A5A)):
            if buf is None:
                out.append(None)
                continue
            h = buf.cpu().numpy()
            assert (h[words:] == fill).all(), "the words past an output were written"
            out.append(h[:words])
        return tuple(out)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def check(got, ref, what):
    counts, shared = got
    rc, rs = ref
    if counts is not None:
        K = (rc.size - 2) // 2
        bad = np.flatnonzero(counts != rc)
        assert not bad.size, "%s: counts differ at %s (K = %d): got %s, want %s" % (what, bad[:8], K, counts[bad[:8]], rc[bad[:8]])
    if shared is not None:
        bad = np.flatnonzero(shared != rs)
        assert not bad.size, "%s: shared differs at edge %s: got %s, want %s" % (what, bad[:8], shared[bad[:8]], rs[bad[:8]])


def thresholds():
    return (("0", 0.0), ("0.05", 0.05), ("planted", float(PLANTED)), ("above", ABOVE))


def exact_group(ks):
    b = Bench()
    rng = np.random.default_rng(41)
    for K in ks:
        N = {1: 4999, 3: 1237}.get(K, 600 if K >= 1024 else 911)
        host, kind = draw_rows(rng, N, K)
        pi = b.matrix(host)
        edge_lists = {n: draw_edges(rng, N, n, kind) for n in (1, 3, 257, 5000)}
        for name, thr in thresholds():
            mask = b.mask(pi, thr)
            with np.errstate(invalid="ignore"):
                M = host >= F32(thr)
            # every bit that stands for no community is zero: the bits set are the members, no more
            assert popcount(mask.cpu().numpy()) == int(M.sum()), "K=%d thr=%s: set bits" % (K, name)
            assert b.torch.equal(mask, b.mask(pi, thr)), "K=%d thr=%s: a second mask differs" % (K, name)
            if name == "0":        # everything that is not a NaN is a member
                assert np.array_equal(M, ~np.isnan(host))
            if name == "planted":  # the tie is a member, the next float below is not
                pc = planted_cols(K)
                assert M[kind == 4][:, pc].all() and not M[kind == 5][:, pc].any()
            if name == "above":
                assert not M.any()
            for n, edges in edge_lists.items():
                what = "K=%d n=%d thr=%s" % (K, n, name)
                ref = reference(host, thr, edges)
                got = b.edges(mask, N, K, edges)
                check(got, ref, what)
                if name == "above":
                    assert got[0][2 * K] == (ref[1] >= 0).sum() and got[0][:2 * K].sum() == 0, what
                if name == "0" and n == 257:
                    valid = ref[1] >= 0
                    nonan = valid & (kind[ends(edges)[0] % N] != 3) & (kind[ends(edges)[1] % N] != 3)
                    assert nonan.sum() > 100 and (got[1][nonan] == K).all(), what   # every bit set
                if n in (3, 257):
                    # counts alone and shared alone agree with the full call; a second call and swapped ends too
                    check(b.edges(mask, N, K, edges, shared=False), (ref[0], None), what + ": counts only")
                    check(b.edges(mask, N, K, edges, counts=False), (None, ref[1]), what + ": shared only")
                    again = b.edges(mask, N, K, edges)
                    sw = b.edges(mask, N, K, (edges << U32) | (edges >> U32))
                    for x, y, z in zip(got, again, sw):
                        assert np.array_equal(x, y), what + ": second call"
                        assert np.array_equal(x, z), what + ": ends swapped"
        # the layers above: ops.CommunityQuality over its own tensors
        edges = edge_lists[257]
        m2 = b.api.mask(pi, 0.05)
        cnt, sh = b.api.edges(m2, N, K, edges, shared=True)
        check((cnt.cpu().numpy(), sh.cpu().numpy()), reference(host, 0.05, edges), "ops K=%d" % K)
        assert np.array_equal(b.api.edges(m2, N, K, b.ctx.from_numpy(edges)).cpu().numpy(), cnt.cpu().numpy())
        empty = b.api.edges(m2, N, K, np.zeros(0, np.uint64), shared=True)
        assert empty[0].sum().item() == 0 and empty[1].numel() == 0
        print("exact K=%d ok (%s)" % (K, b.q.last_kernel_name()), flush=True)
    print("exact ok", flush=True)


def persistent_group(ks):
    """More edges than the grid has groups of lanes: every group takes several edges, so the next edge's words are
    requested before the current edge's bit walk and a block's counters take several edges per group.  K = 64 and 256
    put 64 and 16 edges into a wave, 1024 and 2048 four and two, 8192 gives a lane two words.  The invalid ends, a == b
    and the edges inside one kind of rows sit past index 8192 as well, where only the loop reaches them."""
    b = Bench()
    rng = np.random.default_rng(45)
    n, N = 20011, 600
    for K in ks:
        host, kind = draw_rows(rng, N, K)
        pi = b.matrix(host)
        edges = draw_edges(rng, N, n, kind)
        tail = draw_edges(rng, N, 257, kind)           # its special edges again, in odd places past the first pass
        at = 8197 + 41 * np.arange(257)
        edges[at] = tail
        assert at.min() > 8192 and at.max() < n - 6
        for name, thr in thresholds():
            what = "persistent K=%d thr=%s" % (K, name)
            mask = b.mask(pi, thr)
            ref = reference(host, thr, edges)
            assert ref[0][2 * K + 1] >= 6
            got = b.edges(mask, N, K, edges)
            assert b.q.last_kernel_name() == ("quality_edges_w2" if K > 4096 else "quality_edges_w1")
            check(got, ref, what)
            if name == "0.05":
                check(b.edges(mask, N, K, edges, shared=False), (ref[0], None), what + ": counts only")
                check(b.edges(mask, N, K, edges, counts=False), (None, ref[1]), what + ": shared only")
                sw = b.edges(mask, N, K, (edges << U32) | (edges >> U32))
                assert all(np.array_equal(x, y) for x, y in zip(got, sw)), what + ": ends swapped"
        print("persistent K=%d ok (%s)" % (K, b.q.last_kernel_name()), flush=True)
    print("persistent ok", flush=True)


def layout_group():
    """pi as one, two and eleven-plus-a-ragged-one blocks, edges whose ends fall in different blocks; a misaligned
    block base, which forces the generic mask form at K = 256: its bytes are the fast form's"""
    b = Bench()
    rng = np.random.default_rng(42)
    n, K = 4700, 256
    host, kind = draw_rows(rng, n, K)
    edges = draw_edges(rng, n, 3000, kind)
    edges[:8] = (np.arange(8, dtype=np.uint64) << U32) | np.uint64(n - 1)   # first block against the last
    for name, thr in (("0.05", 0.05), ("planted", float(PLANTED)), ("0", 0.0)):
        ref = reference(host, thr, edges)
        first = None
        for rib in (0, (n + 1) // 2, 400):
            pi = b.matrix(host, rib)
            assert len(pi.blocks) == {0: 1, (n + 1) // 2: 2, 400: 12}[rib]
            mask = b.mask(pi, thr)
            assert b.q.last_kernel_name() == "quality_mask_fast"
            first = mask if first is None else first
            assert b.torch.equal(mask, first), "rows_in_block=%d: the mask differs" % rib
            check(b.edges(mask, n, K, edges), ref, "rows_in_block=%d thr=%s" % (rib, name))
        mask = b.mask(b.misaligned(host), thr)
        assert b.q.last_kernel_name() == "quality_mask_generic"
        assert b.torch.equal(mask, first), "thr=%s: the generic form's bytes differ from the fast form's" % name
        check(b.edges(mask, n, K, edges), ref, "misaligned base thr=%s" % name)
    print("layout ok", flush=True)


def forms_group():
    """every kernel form the dispatchers can select is reached and reported"""
    import re
    from mcmc_ammsb_gpu_amd import _quality
    b = Bench()
    rng = np.random.default_rng(44)
    for K, mform, eform in ((100, "generic", "w1"), (256, "fast", "w1"), (4096, "fast", "w1"), (4100, "generic", "w2"),
                            (4352, "fast", "w2"), (8192, "fast", "w2")):
        host, kind = draw_rows(rng, 300, K)
        edges = draw_edges(rng, 300, 257, kind)
        mask = b.mask(b.matrix(host), 0.05)
        assert b.q.last_kernel_name() == "quality_mask_" + mform, (K, b.q.last_kernel_name())
        got = b.edges(mask, 300, K, edges)
        assert b.q.last_kernel_name() == "quality_edges_" + eform, (K, b.q.last_kernel_name())
        check(got, reference(host, 0.05, edges), "forms K=%d" % K)
    src = open(os.path.join(ps.ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_quality.hip")).read()
    in_source = set(re.findall(r'"(quality_(?:mask|edges)_[a-z0-9_]+)"', src))
    assert in_source == set(_quality.KERNEL_FORMS), in_source ^ set(_quality.KERNEL_FORMS)
    print("forms seen: %s" % " ".join(sorted(SEEN)), flush=True)
    assert SEEN == in_source, SEEN ^ in_source
    print("forms ok", flush=True)


def big_group():
    """K = 8192 and a little over 2^32 elements in one block (17 GB), zeroed and then filled on the device where the
    edges touch it: members and edges among the last rows, against numpy over those rows only; then the same rows in a
    block whose base is 4 bytes past a 16-byte boundary, which takes the generic mask form: the same mask, the same
    counts"""
    b = Bench()
    torch = b.torch
    K, tail = 8192, 256
    n = (1 << 32) // K + tail // 2      # the last tail / 2 rows start past element 2^32
    pi, blk = b.zeroed(n, K)
    gen = torch.Generator(device=blk.device)
    gen.manual_seed(9)
    r = torch.rand((tail, K), generator=gen, device=blk.device).pow_(64).clamp_(min=1e-24)
    r = r / r.sum(1, keepdim=True)
    blk[n - tail:].copy_(r)
    host_tail = blk[n - tail:].cpu().numpy()
    thr = float(np.sort(host_tail.reshape(-1))[-40 * tail])     # about 40 memberships per node
    rng = np.random.default_rng(43)
    local = draw_edges(rng, tail, 512)[:-6]            # (the out-of-range ends of draw_edges are relative to `tail`)
    u, v = local >> U32, local & np.uint64(NONE)
    off = np.uint64(n - tail)
    edges = np.concatenate([((u + off) << U32) | (v + off), [(np.uint64(n) << U32) | np.uint64(n - 1),
                                                            (np.uint64(n - 1) << U32) | np.uint64(n - 1)]])
    local = np.concatenate([local, [(np.uint64(tail) << U32) | np.uint64(tail - 1),
                                    (np.uint64(tail - 1) << U32) | np.uint64(tail - 1)]])
    mask = b.mask(pi, thr)
    assert b.q.last_kernel_name() == "quality_mask_fast"
    with np.errstate(invalid="ignore"):
        M = host_tail >= F32(thr)
    assert M.sum() >= 40 * tail
    got = b.edges(mask, n, K, edges)
    assert b.q.last_kernel_name() == "quality_edges_w2"
    ref = reference(host_tail, thr, local)
    assert ref[0][:K].sum() > 0 and ref[0][2 * K + 1] == 1
    check(got, ref, "beyond 2^32 elements")
    del pi, blk
    b.release()
    mis, blk = b.zeroed(n, K, misaligned=True)
    blk[n - tail:].copy_(r)
    again = b.mask(mis, thr)
    assert b.q.last_kernel_name() == "quality_mask_generic"
    assert torch.equal(mask, again), "the generic form's bytes differ from the fast form's"
    got2 = b.edges(again, n, K, edges)
    check(got2, ref, "beyond 2^32 elements, misaligned base")
    assert all(np.array_equal(x, y) for x, y in zip(got, got2))
    print("big ok: %d x %d" % (n, K), flush=True)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _quality
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    lrn.Run(30)
    ck = io.BytesIO()
    lrn.Serialize(ck)
    host, _ = ps.pi_beta_of_checkpoint(ck.getvalue(), N, K)
    assert np.array_equal(host.view(np.uint32), lrn.pi.host().view(np.uint32))
    links = lrn.TrainingLinks().cpu().numpy().view(np.uint64)
    E = links.size
    for thr in (0.05, 0.01, 0.0, 2.0):
        r = lrn.CommunityQuality(thr)
        assert isinstance(r, _quality.Quality)
        rc, rs = reference(host, F32(thr), links)
        assert np.array_equal(r.internal, rc[:K]) and np.array_equal(r.boundary, rc[K:2 * K]), "thr=%g" % thr
        assert (r.links, r.uncovered, r.skipped) == (E, int(rc[2 * K]), 0), "thr=%g" % thr
        with np.errstate(invalid="ignore"):
            size = (host >= F32(thr)).sum(0)
        assert np.array_equal(r.size, size) and np.array_equal(r.size, lrn.CommunitySizes(thr).cpu().numpy())
        assert r.size.dtype == r.internal.dtype == r.boundary.dtype == np.int64
        assert np.array_equal(r.conductance, _quality.conductance(rc[:K], rc[K:2 * K], E))
        assert np.array_equal(r.density, _quality.density(size, rc[:K])) and r.coverage == 1.0 - rc[2 * K] / E
        sh = lrn.SharedCommunities(None, thr).cpu().numpy()
        assert sh.dtype == np.int32 and np.array_equal(sh, rs), "SharedCommunities thr=%g" % thr
        print("thr=%g: %d links, %d uncovered, coverage %.4f, median conductance %.4f" % (
            thr, E, r.uncovered, r.coverage, float(np.median(r.conductance))), flush=True)
    # a list of the caller's, host array or device tensor, either order of the ends, with an end >= N in it
    some = np.concatenate([links[::37], [(np.uint64(N) << U32) | np.uint64(3), links[5], links[5]]])
    rc, rs = reference(host, F32(0.05), some)
    for arg in (some, lrn.ctx.from_numpy((some << U32) | (some >> U32))):
        r = lrn.CommunityQuality(0.05, arg)
        assert np.array_equal(r.internal, rc[:K]) and np.array_equal(r.boundary, rc[K:2 * K])
        assert (r.links, r.uncovered, r.skipped) == (some.size - 1, int(rc[2 * K]), 1)
        assert np.array_equal(lrn.SharedCommunities(arg, 0.05).cpu().numpy(), rs)
    # an empty list is a valid no-op at every layer
    for none in (np.zeros(0, np.uint64), lrn.ctx.from_numpy(np.zeros(0, np.uint64))):
        r = lrn.CommunityQuality(0.05, none)
        assert (r.links, r.uncovered, r.skipped, r.coverage) == (0, 0, 0, -1.0) and (r.conductance == -1).all()
        assert r.internal.sum() == 0 and np.array_equal(r.size, lrn.CommunitySizes(0.05).cpu().numpy())
        assert lrn.SharedCommunities(none, 0.05).numel() == 0
    ps.rejects(AmmsbError, (lambda: lrn.CommunityQuality(-1.0), lambda: lrn.CommunityQuality(float("nan")),
                            lambda: lrn.SharedCommunities(some, float("inf"))))
    lrn.close()
    # Run(20), the calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.CommunityQuality()
        a.CommunityQuality(0.01, some)
        a.SharedCommunities(some, 0.05)
    ps.unperturbed_run(make, calls, "community quality")
    print("learner ok graph=%s" % graph, flush=True)


def _check_file(path, ckpt, K, thr):
    """a community-quality file against the numpy statement over the pi of the checkpoint the same process wrote and
    the links the file counts; the Python writer reproduces its bytes"""
    from mcmc_ammsb_gpu_amd import _quality
    fN, fK, fE, fthr, unc, size, internal, boundary, cond, dens = _quality.read_community_quality(path)
    assert fK == K and F32(fthr) == F32(thr), (fK, fthr)
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    again = path + ".py"
    _quality.write_community_quality(again, fN, fthr, size, internal, boundary, fE, unc)
    assert open(again, "rb").read() == open(path, "rb").read(), "the Python writer's bytes differ"
    return fN, fE, pi, (unc, size, internal, boundary)


def _check_counts(pi, thr, links, got, what):
    unc, size, internal, boundary = got
    K = pi.shape[1]
    rc, _ = reference(pi, F32(thr), links)
    assert np.array_equal(internal, rc[:K]) and np.array_equal(boundary, rc[K:2 * K]) and unc == rc[2 * K], what
    assert np.array_equal(size, (pi >= F32(thr)).sum(0)), what


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import _linkcomm, hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("quality_test", d, 240)
        fN, fE, pi, got = _check_file(os.path.join(d, "quality.txt"), os.path.join(d, "cpp.ckpt"), 64, 0.05)
        assert fN == 20000 and fE > 100000
        links = _linkcomm.read_link_communities(os.path.join(d, "links.txt"))[4]
        assert fE == links.size
        _check_counts(pi, 0.05, links, got, "quality_test")
        print("cpp ok: Learner::WriteCommunityQuality equals the statement over the checkpoint's pi", flush=True)
        # the command-line driver on a small generated graph; the links from the link-communities file of the same run
        N = 6000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, lc, ck = os.path.join(d, "q.txt"), os.path.join(d, "lc.txt"), os.path.join(d, "main.ckpt")
        base = ["--load-data", "1", "--load-file", f, "-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30",
                "--community-quality-out", out, "--link-communities-out", lc, "--checkpoint-out", ck]
        for extra, thr in (([], 0.05), (["--community-quality-threshold", "0.01"], 0.01)):
            ps.run_ammsb_main(base + extra, 240)
            fN, fE, pi, got = _check_file(out, ck, 48, thr)
            links = _linkcomm.read_link_communities(lc)[4]
            assert fN == N and fE == links.size and fE > 1000
            _check_counts(pi, thr, links, got, "ammsb_main thr=%g" % thr)
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(k) for k in a) or (1, 3, 64, 65, 100, 256, 260, 1024, 2048, 8192)),
    "persistent": lambda a: persistent_group(tuple(int(k) for k in a) or (64, 256, 1024, 2048, 8192)),
    "layout": lambda a: layout_group(),
    "forms": lambda a: forms_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
