"""Child process of test_gpu_linkcomm.py (one per group): the communities that explain a link
(include/ammsb_linkcomm.h, ops.LinkCommunities, Learner.LinkCommunities / LinkCommunitySizes) against numpy statements.

  (i)   ids and terms exactly: t = (pa.astype(f32) * pb) * beta_odd in numpy float32 (two multiplications, subnormals
        kept), order = np.lexsort((k, -t)) restricted to (t > 0) & (t >= min_term); ids as integers, terms by bit pattern.
  (ii)  prob against p64 = eps + sum_k pi_ak pi_bk (beta_k - eps) in float64 over the stored binary32 values, under
        |got - p64| <= (K + 8) 2^-24 M + 2^-100, M = eps + sum_k pi_ak pi_bk |beta_k - eps|: the bound the header
        derives (at most K + 3 roundings touch a summand), not a measured one.
  (iii) sizes against np.bincount of the reference's slot 0, the edges with valid ends and no slot counted at K."""
import ctypes as C
import os
import sys

import numpy as np

import postfit_support as ps

NONE = 0xFFFFFFFF
EPS = float(np.float32(1e-7))
SEEN = set()
F32 = np.float32


def planted_cols(K):
    """columns that hold equal products in the planted rows: the same lane of both forms (k0 + 1 shares a float4 in
    fast, k0 + 256 the lane in fast and generic, k0 + 64 the lane in generic) and different lanes (k0 + 4)"""
    k0 = 2 if K > 8 else 0
    return np.array(sorted({k for k in (k0, k0 + 1, k0 + 4, k0 + 64, k0 + 256) if k < K}), dtype=np.int64)


def draw_rows(rng, n, K):
    """a sixth each: fitted-looking rows (Dirichlet alpha = 1/K, floored at 1e-24), flat rows (1/64 everywhere: all
    products tie), one-hot rows, rows at the floor 1e-24 (against an ordinary row their products are subnormal or
    underflow), rows mixing a floor half with a fitted half, and planted rows: 0.125 on planted_cols(K), so an edge
    between two of them has equal products there"""
    kind = np.arange(n) % 6
    rng.shuffle(kind)
    fitted = np.maximum(rng.gamma(1.0 / K, 1.0, (n, K)), 1e-24)
    fitted /= fitted.sum(1, keepdims=True)
    flat = np.full((n, K), 1.0 / 64)
    onehot = np.zeros((n, K))
    onehot[np.arange(n), rng.integers(0, K, n)] = 1.0
    floor = np.full((n, K), 1e-24)
    mixed = np.where(rng.random((n, K)) < 0.5, 1e-24, fitted * 1e-14)
    planted = fitted * 0.01
    planted[:, planted_cols(K)] = 0.125
    rows = np.choose(kind[:, None], [fitted, flat, onehot, floor, mixed, planted])
    return rows.astype(F32), kind


def draw_beta(rng, K):
    """[2K] as the learner stores it (beta_k at 2k + 1): near 0, near 1, exactly 0, and in between; equal on the
    planted columns"""
    b = rng.random(K)
    sel = rng.integers(0, 4, K)
    b = np.where(sel == 0, b * 1e-6, np.where(sel == 1, 1.0 - b * 1e-6, np.where(sel == 2, 0.0, b)))
    b[planted_cols(K)] = 0.75
    if K > 8:
        b[0] = 0.0
    out = rng.random(2 * K)
    out[1::2] = b
    return out.astype(F32)


def draw_edges(rng, N, n, kind=None):
    u, v = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
    if kind is not None and n >= 200:     # some edges inside one kind of rows (planted-planted, flat-flat, ...)
        for kd in range(6):
            rows = np.flatnonzero(kind == kd)
            at = slice(20 * kd, 20 * kd + 20)
            u[at], v[at] = rng.choice(rows, 20), rng.choice(rows, 20)
    if n >= 3:
        u[-1] = v[-1]                     # a == b
    if n >= 200:
        u[-2] = N                         # an end == N
        v[-3] = NONE                      # an end == 2^32 - 1
        u[-4], v[-4] = NONE, NONE
    return (u << np.uint64(32)) | v


def reference(pi, beta, eps, edges, T, min_term):
    """-> ids [n, T] uint32, terms [n, T] float32, p64 [n], bound [n], valid [n], slot0 [n] (K: no slot)"""
    N, K = pi.shape
    u, v = (edges >> np.uint64(32)).astype(np.int64), (edges & np.uint64(NONE)).astype(np.int64)
    valid = (u < N) & (v < N)
    n = edges.size
    ids = np.full((n, T), NONE, dtype=np.uint32)
    terms = np.zeros((n, T), dtype=F32)
    p64, bound = np.full(n, -1.0), np.zeros(n)
    slot0 = np.full(n, K, dtype=np.int64)
    b_odd = beta[1::2].astype(F32)
    w = b_odd.astype(np.float64) - np.float64(F32(eps))
    k = np.arange(K)
    for lo in range(0, n, 512):
        sel = np.flatnonzero(valid[lo:lo + 512]) + lo
        if not sel.size:
            continue
        pa, pb = pi[u[sel]], pi[v[sel]]
        t = (pa.astype(F32) * pb) * b_odd
        assert t.dtype == F32
        ok = (t > 0) & (t >= F32(min_term))
        for j, i in enumerate(sel):
            order = np.lexsort((k, -t[j]))
            order = order[ok[j][order]][:T]
            ids[i, :order.size], terms[i, :order.size] = order, t[j][order]
            if order.size:
                slot0[i] = order[0]
        q = pa.astype(np.float64) * pb.astype(np.float64)
        p64[sel] = np.float64(F32(eps)) + (q * w).sum(1)
        bound[sel] = (K + 8) * 2.0 ** -24 * (np.float64(F32(eps)) + (q * np.abs(w)).sum(1)) + 2.0 ** -100
    return ids, terms, p64, bound, valid, slot0


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _linkcomm
        super().__init__()
        self.lc = _linkcomm
        self.lib = _linkcomm.load()
        self.api = self.ops.LinkCommunities(self.ctx)

    def call(self, pi, beta, edges, T, min_term=0.0, eps=EPS, tops=True, prob=True, sizes=True):
        """the library call over outputs of this test's own, each followed by GUARD words of a pattern that must
        survive -> (ids, terms, prob, sizes) as numpy arrays (None for the outputs not asked for)"""
        t, guarded = self.torch, self.guarded
        n, K = int(edges.size), pi.cols
        d_edges = self.dev(np.ascontiguousarray(edges, dtype=np.uint64))
        ids = guarded(n * T, t.int32, 0x5A5A5A5A) if tops else None
        terms = guarded(n * T, t.float32, 7.25) if tops else None
        pr = guarded(n, t.float32, 7.25) if prob else None
        sz = guarded(K + 1, t.int64, 0x5A5A5A5A5A5A, zero=True) if sizes else None
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
        self.lc.check(self.lib.ammsb_linkcomm_edges(C.byref(pi.desc), ptr(beta), eps, ptr(d_edges), n, T, min_term,
                                                    ptr(ids), ptr(terms), ptr(pr), ptr(sz), None))
        t.cuda.synchronize()
        SEEN.add(self.lc.last_kernel_name())
        out = []
        for buf, words, fill in ((ids, n * T, 0x5A5A5A5A), (terms, n * T, 7.25), (pr, n, 7.25), (sz, K + 1, 0x5A5A5A5A5A5A)):
            if buf is None:
                out.append(None)
                continue
            h = buf.cpu().numpy()
            assert (h[words:] == fill).all(), "the bytes past an output were written"
            out.append(h[:words])
        ids, terms, pr, sz = out
        if ids is not None:
            ids, terms = ids.view(np.uint32).reshape(n, T), terms.reshape(n, T)
        return ids, terms, pr, sz


def check(got, ref, K, what, tops=True):
    ids, terms, prob, sizes = got
    rids, rterms, p64, bound, valid, slot0 = ref
    if tops:
        bad = np.flatnonzero((ids != rids).any(1) | (terms.view(np.uint32) != rterms.view(np.uint32)).any(1))
        assert not bad.size, "%s: edge %d: ids %s / %s, terms %s / %s" % (
            what, bad[0], ids[bad[0]], rids[bad[0]], terms[bad[0]], rterms[bad[0]])
    if prob is not None:
        assert (prob[~valid] == -1.0).all(), what
        err = np.abs(prob[valid].astype(np.float64) - p64[valid])
        assert (err <= bound[valid]).all(), "%s: prob off by %.3g x the bound" % (what, (err / bound[valid]).max())
    if sizes is not None:
        want = np.bincount(slot0[valid], minlength=K + 1)
        assert np.array_equal(sizes, want), "%s: sizes differ at %s" % (what, np.flatnonzero(sizes != want)[:8])


def exact_group(ks=(1, 3, 64, 100, 256, 260, 512, 1024, 2048, 8192)):
    b = Bench()
    rng = np.random.default_rng(31)
    for K in ks:
        N = 600
        host, kind = draw_rows(rng, N, K)
        beta_h = draw_beta(rng, K)
        pi, beta = b.matrix(host), b.dev(beta_h)
        planted = F32(F32(0.125) * F32(0.125)) * F32(0.75)      # the planted term, as the kernel forms it
        ns = (1, 3, 257, 5000)
        refs = {}
        for n in ns:
            edges = draw_edges(rng, N, n, kind)
            for T in (1, 4, 16):
                floors = (0.0, float(planted), 2.0) if (n == 257 or T == 4) else (0.0,)
                for min_term in floors:
                    what = "K=%d n=%d T=%d min_term=%g" % (K, n, T, min_term)
                    if (n, min_term) not in refs:      # the statement once per (edges, floor): T slots are a prefix
                        refs[n, min_term] = reference(host, beta_h, EPS, edges, 16, min_term)
                    r16 = refs[n, min_term]
                    ref = (r16[0][:, :T], r16[1][:, :T]) + r16[2:]
                    got = b.call(pi, beta, edges, T, min_term)
                    check(got, ref, K, what)
                    if n == 257:
                        if min_term == float(planted):   # the planted terms are AT the floor: they keep their slots
                            both = np.flatnonzero((kind[(edges >> np.uint64(32)).astype(np.int64) % N] == 5)
                                                  & (kind[(edges & np.uint64(NONE)).astype(np.int64) % N] == 5)
                                                  & ref[4])
                            assert both.size and (ref[1][both, 0] == planted).all(), what
                            assert (ref[0][both, :min(T, planted_cols(K).size)]
                                    == planted_cols(K)[:T]).all(), what
                        if min_term == 2.0:
                            assert (got[0] == NONE).all() and got[3][K] == ref[4].sum(), what
                        # both orders of the ends: the same bits, prob included
                        sw = b.call(pi, beta, (edges << np.uint64(32)) | (edges >> np.uint64(32)), T, min_term)
                        again = b.call(pi, beta, edges, T, min_term)
                        for x, y, z in zip(got, sw, again):
                            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what + ": ends swapped"
                            assert np.array_equal(x.view(np.uint32), z.view(np.uint32)), what + ": second call"
                        # sizes only: the same counters, nothing else written; tops without sizes; prob alone
                        only = b.call(pi, beta, edges, T, min_term, tops=False, prob=False)
                        assert np.array_equal(only[3], got[3]), what + ": sizes-only"
                        check(b.call(pi, beta, edges, T, min_term, prob=False, sizes=False), ref, K, what)
                        check(b.call(pi, beta, edges, T, min_term, tops=False, sizes=False), ref, K, what, tops=False)
        # all terms tied: flat rows and a constant beta give ids 0, 1, 2, ...
        flat = np.flatnonzero(kind == 1)
        const = np.full(2 * K, 0.5, dtype=F32)
        edges = (rng.choice(flat, 64).astype(np.uint64) << np.uint64(32)) | rng.choice(flat, 64).astype(np.uint64)
        got = b.call(pi, b.dev(const), edges, 16)
        check(got, reference(host, const, EPS, edges, 16, 0.0), K, "K=%d flat" % K)
        want = np.where(np.arange(16) < K, np.arange(16), NONE).astype(np.uint32)
        assert (got[0] == want).all() and got[3][0] == 64
        # one-hot rows: fewer positive terms than T (often none)
        hot = np.flatnonzero(kind == 2)
        edges = (rng.choice(hot, 64).astype(np.uint64) << np.uint64(32)) | rng.choice(hot, 64).astype(np.uint64)
        edges[0] = (np.uint64(hot[0]) << np.uint64(32)) | np.uint64(hot[0])
        got = b.call(pi, b.dev(const), edges, 4)
        check(got, reference(host, const, EPS, edges, 4, 0.0), K, "K=%d one-hot" % K)
        assert got[0][0, 0] != NONE and (got[0][:, 1:] == NONE).all()
        print("exact K=%d ok (%s)" % (K, b.lc.last_kernel_name()), flush=True)
    print("exact ok", flush=True)


def persistent_group(ks=(256, 1024, 1280, 2048)):
    """More edges than the grid has waves (2048 blocks x 4): every wave of a fast form takes a second and a third edge,
    so the next edge's key and rows are requested into the live row registers before the current edge's rounds, a block's
    counters take several edges per wave, and in v4_chunked the last chunk hands over to the next edge's first chunk.
    Invalid ends, a == b and edges inside one kind of rows sit past index 8192, where only the loop reaches them."""
    b = Bench()
    rng = np.random.default_rng(35)
    n, N = 20011, 600
    for K in ks:
        host, kind = draw_rows(rng, N, K)
        beta_h = draw_beta(rng, K)
        pi, beta = b.matrix(host), b.dev(beta_h)
        edges = draw_edges(rng, N, n, kind)
        tail = draw_edges(rng, N, 257, kind)           # its special edges again, from index 8192 + 5 on, in odd places
        at = 8197 + 41 * np.arange(257)
        edges[at] = tail
        assert at.min() > 8192 and at.max() < n - 4
        r16 = reference(host, beta_h, EPS, edges, 16, 0.0)
        assert (~r16[4]).sum() >= 6 and (r16[4][:8192]).all()     # the invalid ends are all past the first pass
        for T in (1, 16):
            what = "persistent K=%d T=%d" % (K, T)
            ref = (r16[0][:, :T], r16[1][:, :T]) + r16[2:]
            got = b.call(pi, beta, edges, T)
            assert b.lc.last_kernel_name().startswith("linkcomm_fast"), b.lc.last_kernel_name()
            check(got, ref, K, what)
            sw = b.call(pi, beta, (edges << np.uint64(32)) | (edges >> np.uint64(32)), T)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, sw)), what + ": ends swapped"
        only = b.call(pi, beta, edges, 1, tops=False, prob=False)
        assert np.array_equal(only[3], got[3]) and only[3].sum() == r16[4].sum(), "persistent K=%d: sizes-only" % K
        floor = float(F32(F32(0.125) * F32(0.125)) * F32(0.75))
        check(b.call(pi, beta, edges, 4, floor), reference(host, beta_h, EPS, edges, 4, floor), K, "persistent K=%d, floor" % K)
        print("persistent K=%d ok (%s)" % (K, b.lc.last_kernel_name()), flush=True)
    print("persistent ok", flush=True)


def layout_group():
    """pi as one, two and eleven-plus-a-ragged-one blocks, edges whose ends fall in different blocks; a misaligned
    block base, which forces generic at K = 256"""
    b = Bench()
    rng = np.random.default_rng(32)
    n, K = 4700, 256
    host, kind = draw_rows(rng, n, K)
    beta_h = draw_beta(rng, K)
    beta = b.dev(beta_h)
    edges = draw_edges(rng, n, 3000, kind)
    edges[:8] = (np.arange(8, dtype=np.uint64) << np.uint64(32)) | np.uint64(n - 1)   # first block against the last
    ref = reference(host, beta_h, EPS, edges, 4, 0.0)
    first = None
    for rib in (0, (n + 1) // 2, 400):
        pi = b.matrix(host, rib)
        assert len(pi.blocks) == {0: 1, (n + 1) // 2: 2, 400: 12}[rib]
        got = b.call(pi, beta, edges, 4)
        assert b.lc.last_kernel_name() == "linkcomm_fast_v1"
        check(got, ref, K, "rows_in_block=%d" % rib)
        first = first or got
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, first))
    got = b.call(b.misaligned(host), beta, edges, 4)
    assert b.lc.last_kernel_name() == "linkcomm_generic"
    check(got, ref, K, "misaligned base")
    assert np.array_equal(got[0], first[0]) and np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32))
    assert np.array_equal(got[3], first[3])
    print("layout ok", flush=True)


def forms_group():
    """every kernel form the dispatcher can select is reached and reported"""
    import re
    from mcmc_ammsb_gpu_amd import _linkcomm
    b = Bench()
    rng = np.random.default_rng(34)
    for K, form in ((100, "generic"), (256, "fast_v1"), (512, "fast_v2"), (768, "fast_v4"), (1024, "fast_v4"),
                    (1280, "fast_v4_chunked"), (2048, "fast_v4_chunked")):
        host, kind = draw_rows(rng, 300, K)
        beta_h = draw_beta(rng, K)
        edges = draw_edges(rng, 300, 257, kind)
        got = b.call(b.matrix(host), b.dev(beta_h), edges, 4)
        assert b.lc.last_kernel_name() == "linkcomm_" + form, (K, b.lc.last_kernel_name())
        check(got, reference(host, beta_h, EPS, edges, 4, 0.0), K, "forms K=%d" % K)
    src = open(os.path.join(ps.ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_linkcomm.hip")).read()
    in_source = set(re.findall(r'"(linkcomm_(?:fast|generic)[a-z0-9_]*)"', src))
    assert in_source == set(_linkcomm.KERNEL_FORMS), in_source ^ set(_linkcomm.KERNEL_FORMS)
    print("forms seen: %s" % " ".join(sorted(SEEN)), flush=True)
    assert SEEN == in_source, SEEN ^ in_source
    print("forms ok", flush=True)


def big_group():
    """K = 8192 and a little over 2^32 elements in one block (17 GB), zeroed and then filled on the device where the
    edges touch it: 512 edges among the last rows, against numpy over the gathered rows only; then the same rows in a
    block whose base is 4 bytes past a 16-byte boundary, which takes the generic form: the same ids, terms and sizes, prob
    under its bound"""
    b = Bench()
    torch = b.torch
    K, tail = 8192, 256
    n = (1 << 32) // K + tail // 2      # the last tail / 2 rows start past element 2^32
    pi, blk = b.zeroed(n, K)
    gen = torch.Generator(device=blk.device)
    gen.manual_seed(8)
    r = torch.rand((tail, K), generator=gen, device=blk.device).pow_(64).clamp_(min=1e-24)
    r = r / r.sum(1, keepdim=True)
    blk[n - tail:].copy_(r)
    rng = np.random.default_rng(33)
    beta_h = draw_beta(rng, K)
    host_tail = blk[n - tail:].cpu().numpy()
    local = draw_edges(rng, tail, 512)[:-4]            # (the out-of-range ends of draw_edges are relative to `tail`)
    u, v = local >> np.uint64(32), local & np.uint64(NONE)
    edges = ((u + np.uint64(n - tail)) << np.uint64(32)) | (v + np.uint64(n - tail))
    edges = np.concatenate([edges, [(np.uint64(n) << np.uint64(32)) | np.uint64(n - 1), np.uint64(n - 1) << np.uint64(32) | np.uint64(n - 1)]])
    local = np.concatenate([local, [(np.uint64(tail) << np.uint64(32)) | np.uint64(tail - 1), np.uint64(tail - 1) << np.uint64(32) | np.uint64(tail - 1)]])
    refs, fast = {}, {}
    for T in (1, 16):
        refs[T] = reference(host_tail, beta_h, EPS, local, T, 0.0)
        fast[T] = b.call(pi, b.dev(beta_h), edges, T)
        assert b.lc.last_kernel_name() == "linkcomm_fast_v4_chunked"
        check(fast[T], refs[T], K, "beyond 2^32 elements, T=%d" % T)
    del pi, blk
    b.release()
    mis, blk = b.zeroed(n, K, misaligned=True)
    blk[n - tail:].copy_(r)
    for T in (1, 16):
        got = b.call(mis, b.dev(beta_h), edges, T)
        assert b.lc.last_kernel_name() == "linkcomm_generic"
        check(got, refs[T], K, "beyond 2^32 elements, misaligned base, T=%d" % T)
        # ids, terms and sizes are exact in both forms; prob is a sum whose order the form decides (layout_group)
        assert np.array_equal(got[0], fast[T][0]) and np.array_equal(got[1].view(np.uint32), fast[T][1].view(np.uint32))
        assert np.array_equal(got[3], fast[T][3])
    print("big ok: %d x %d" % (n, K), flush=True)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    lrn.Run(30)
    host, beta_h, eps = lrn.pi.host(), lrn.beta.cpu().numpy(), lrn.params.epsilon
    links = lrn.TrainingLinks().cpu().numpy().view(np.uint64)
    te = np.ascontiguousarray(ds.training_edges, dtype=np.uint64)
    lo, hi = np.minimum(te >> np.uint64(32), te & np.uint64(NONE)), np.maximum(te >> np.uint64(32), te & np.uint64(NONE))
    assert np.array_equal(links, np.unique((lo << np.uint64(32)) | hi)) and lrn.TrainingLinks() is lrn.TrainingLinks()
    E = links.size
    for top, min_term in ((1, 0.0), (4, 1e-3)):
        ids, share, prob = (t.cpu().numpy() for t in lrn.LinkCommunities(top=top, min_term=min_term))
        assert ids.shape == (E, top) and ids.dtype == np.int32 and share.shape == (E, top) and prob.shape == (E,)
        ref = reference(host, beta_h, eps, links, top, min_term)
        assert np.array_equal(ids.view(np.uint32), ref[0]), "LinkCommunities ids, top=%d" % top
        check((None, None, prob, None), ref, K, "LinkCommunities prob", tops=False)
        # share = terms / prob: one binary32 division of exact terms, accurate to an ulp (2^-23 relative)
        want = ref[1].astype(np.float64) / prob.astype(np.float64)[:, None]
        assert (np.abs(share - want) <= 2.0 ** -23 * want).all() and (share[ids < 0] == 0).all()
        # the terms under share, bit for bit, through the layer the Learner calls; share is their one division by prob
        lc = lrn._linkcomm()
        i2, t2, p2 = lc.edges(lrn.pi, lrn.beta, eps, lrn.TrainingLinks(), top, min_term)
        assert np.array_equal(t2.cpu().numpy().view(np.uint32), ref[1].view(np.uint32)), "terms, top=%d" % top
        assert np.array_equal(i2.cpu().numpy(), ids) and np.array_equal(p2.cpu().numpy().view(np.uint32), prob.view(np.uint32))
        assert np.array_equal((t2 / p2.unsqueeze(1)).cpu().numpy().view(np.uint32), share.view(np.uint32))
        sizes = lrn.LinkCommunitySizes(min_term).cpu().numpy()
        assert sizes.shape == (K + 1,) and sizes.dtype == np.int64 and sizes.sum() == E
        assert np.array_equal(sizes, np.bincount(np.where(ids[:, 0] < 0, K, ids[:, 0]), minlength=K + 1))
        print("top=%d min_term=%g: %d links, %d unexplained, largest community %d" % (top, min_term, E, sizes[K], sizes[:K].max()), flush=True)
    # a list of the caller's, host array or device tensor, either order of the ends
    some = links[::37]
    one = tuple(t.cpu().numpy() for t in lrn.LinkCommunities(some, top=3))
    sw = tuple(t.cpu().numpy() for t in lrn.LinkCommunities(lrn.ctx.from_numpy((some << np.uint64(32)) | (some >> np.uint64(32))), top=3))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(one, sw))
    assert np.array_equal(lrn.LinkCommunitySizes(edges=some).cpu().numpy(),
                          np.bincount(np.where(one[0][:, 0] < 0, K, one[0][:, 0]), minlength=K + 1))
    # an empty list is a valid no-op at every layer; an end >= N gives empty slots, share +0 and p = -1
    for none in (np.zeros(0, np.uint64), lrn.ctx.from_numpy(np.zeros(0, np.uint64))):
        e_ids, e_share, e_prob = lrn.LinkCommunities(none, top=3)
        assert e_ids.shape == (0, 3) and e_share.shape == (0, 3) and e_prob.shape == (0,) and e_ids.dtype == lrn.LinkCommunities(some, top=3)[0].dtype
        assert lrn.LinkCommunitySizes(edges=none).cpu().numpy().sum() == 0
    out = tuple(t.cpu().numpy() for t in lrn.LinkCommunities(np.array([(N << 32) | 3, some[0]], dtype=np.uint64), top=2))
    assert (out[0][0] == -1).all() and (out[1][0].view(np.uint32) == 0).all() and out[2][0] == -1.0
    assert np.array_equal(out[0][1], one[0][0, :2]) and np.array_equal(out[1][1].view(np.uint32), one[1][0, :2].view(np.uint32))
    ps.rejects(AmmsbError, (lambda: lrn.LinkCommunities(top=0), lambda: lrn.LinkCommunities(top=17),
                            lambda: lrn.LinkCommunities(min_term=-1.0), lambda: lrn.LinkCommunitySizes(float("nan"))))
    # slabs: a budget that cuts the links into many calls gives the same tensors
    whole = tuple(t.cpu().numpy() for t in lrn.LinkCommunities(top=4))
    lrn.LINKCOMM_SLAB_BYTES = 36 * 1000
    cut = tuple(t.cpu().numpy() for t in lrn.LinkCommunities(top=4))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(whole, cut))
    lrn.close()
    # Run(20), the calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.TrainingLinks()
        a.LinkCommunities(top=4)
        a.LinkCommunitySizes(1e-3)
    ps.unperturbed_run(make, calls, "link communities")
    print("learner ok graph=%s" % graph, flush=True)


def _check_file(path, ckpt, K, top, min_term):
    """a link-communities file against the numpy statement over the pi and beta of the checkpoint the same process
    wrote; the Python writer reproduces its bytes"""
    from mcmc_ammsb_gpu_amd import _linkcomm
    fN, fK, ftop, fmin, edges, prob, ids, terms = _linkcomm.read_link_communities(path)
    assert (fK, ftop, F32(fmin)) == (K, top, F32(min_term)), (fK, ftop, fmin)
    u, v = edges >> np.uint64(32), edges & np.uint64(NONE)
    assert (u < v).all() and (v < fN).all() and (np.diff(edges.astype(np.int64)) > 0).all()
    pi, beta = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    check((ids, terms, prob, None), reference(pi, beta, EPS, edges, top, F32(min_term)), K, os.path.basename(path))
    again = path + ".py"
    _linkcomm.write_link_communities(again, fN, fK, ftop, fmin, edges, prob, ids.view(np.int32), terms)
    assert open(again, "rb").read() == open(path, "rb").read(), "the Python writer's bytes differ"
    return fN, edges.size


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("linkcomm_test", d, 240)
        fN, E = _check_file(os.path.join(d, "linkcomm.txt"), os.path.join(d, "cpp.ckpt"), 64, 3, 0.0)
        assert fN == 20000 and E > 100000
        print("cpp ok: Learner::WriteLinkCommunities equals the statement over the checkpoint's pi", flush=True)
        # the command-line driver on a small generated graph
        N = 6000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck = os.path.join(d, "lc.txt"), os.path.join(d, "main.ckpt")
        base = ["--load-data", "1", "--load-file", f, "-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30",
                "--link-communities-out", out, "--checkpoint-out", ck]
        for extra, top, min_term in (([], 1, 0.0),
                                     (["--link-communities-top", "16", "--link-communities-min-term", "0.001"], 16, 0.001)):
            ps.run_ammsb_main(base + extra, 240)
            fN, E = _check_file(out, ck, 48, top, min_term)
            assert fN == N and E > 1000
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(k) for k in a) or (1, 3, 64, 100, 256, 260, 512, 1024, 2048, 8192)),
    "persistent": lambda a: persistent_group(tuple(int(k) for k in a) or (256, 1024, 1280, 2048)),
    "layout": lambda a: layout_group(),
    "forms": lambda a: forms_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
