"""Child process of test_gpu_linkpred.py (one per group): link prediction (include/ammsb_linkpred.h, ops.LinkPredictor,
Learner.LinkProbabilities / PredictLinks / HeldoutAUC) against numpy statements.

  (i)  block and pairs against p64 = eps + sum_k pi_ak pi_bk (beta_k - eps), evaluated in float64 over the stored
       binary32 values, under |got - p64| <= (K + 8) 2^-24 M + 2^-100, M = eps + sum_k pi_ak pi_bk |beta_k - eps|.
       The bound is derived (at most K + 3 roundings touch a term, gamma_{K+3} < (K + 8) 2^-24 for K <= 8192; the
       constant covers products that underflow binary32), not measured.
  (ii) top against np.argsort(-row, kind="stable") over block's row with the ineligible entries removed: ids as
       integers, scores by bit pattern.  No tolerance."""
import os
import sys

import numpy as np

import postfit_support as ps

NONE = 0xFFFFFFFF
KS = (1, 3, 48, 64, 113, 256, 512, 1024, 2048, 4096, 8192)
QS = (1, 31, 32, 33, 200)
CANDS = (1, 63, 65, 5000)
EPS = float(np.float32(1e-7))
SEEN = set()


def edge_key(a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)


def draw_rows(rng, n, K):
    """a quarter each: fitted-looking rows (Dirichlet alpha = 1/K), flat rows, rows at the floor 1e-24 (their products
    underflow binary32), and rows mixing a floor half with a fitted half"""
    kind = np.arange(n) % 4
    rng.shuffle(kind)
    fitted = np.maximum(rng.gamma(1.0 / K, 1.0, (n, K)), 1e-24)
    fitted /= fitted.sum(1, keepdims=True)
    flat = rng.gamma(1.0, 1.0, (n, K))
    flat /= flat.sum(1, keepdims=True)
    floor = np.full((n, K), 1e-24)
    mixed = np.where(rng.random((n, K)) < 0.5, 1e-24, fitted)
    rows = np.choose(kind[:, None], [fitted, flat, floor, mixed])
    return rows.astype(np.float32)


def draw_beta(rng, K, eps):
    """[2K] as the learner stores it (beta_k at 2k + 1): near 0, near 1, below eps (a negative weight), and in between"""
    b = rng.random(K)
    sel = rng.integers(0, 4, K)
    b = np.where(sel == 0, b * 1e-6, np.where(sel == 1, 1.0 - b * 1e-6, np.where(sel == 2, eps * b, b)))
    out = rng.random(2 * K)
    out[1::2] = b
    return out.astype(np.float32)


def p64_block(pi, beta, eps, q, cand):
    """-> (p64 [Q, n], bound [Q, n]) for query rows q and candidate rows cand (index arrays)"""
    w = beta[1::2].astype(np.float64) - np.float64(np.float32(eps))
    a = pi[q].astype(np.float64)
    b = pi[cand].astype(np.float64)
    p = np.float64(np.float32(eps)) + (a * w) @ b.T
    M = np.float64(np.float32(eps)) + (a * np.abs(w)) @ b.T
    return p, (pi.shape[1] + 8) * 2.0 ** -24 * M + 2.0 ** -100


def p64_pairs(pi, beta, eps, u, v):
    w = beta[1::2].astype(np.float64) - np.float64(np.float32(eps))
    t = pi[u].astype(np.float64) * pi[v].astype(np.float64)
    p = np.float64(np.float32(eps)) + (t * w).sum(1)
    M = np.float64(np.float32(eps)) + (t * np.abs(w)).sum(1)
    return p, (pi.shape[1] + 8) * 2.0 ** -24 * M + 2.0 ** -100


class Bench(ps.DeviceBench):
    def __init__(self):
        super().__init__()
        self.lp = self.ops.LinkPredictor(self.ctx)

    def block(self, pi, beta, q, cand, eps=EPS):
        out = self.lp.block(pi, beta, eps, np.asarray(q, dtype=np.uint32), cand)
        self.torch.cuda.synchronize()
        SEEN.add(self.lp.kernel_name())
        return out.cpu().numpy()

    def top(self, pi, beta, q, T, exclude=(), cand=None, eps=EPS):
        ids, scores = self.lp.top(pi, beta, eps, np.asarray(q, dtype=np.uint32), T, exclude=exclude, cand=cand)
        self.torch.cuda.synchronize()
        SEEN.add(self.lp.kernel_name())
        return ids.cpu().numpy().view(np.uint32), scores.cpu().numpy()

    def pairs(self, pi, beta, edges, eps=EPS):
        out = self.lp.pairs(pi, beta, eps, np.asarray(edges, dtype=np.uint64))
        self.torch.cuda.synchronize()
        SEEN.add(self.lp.kernel_name())
        return out.cpu().numpy()

    def set_of(self, keys):
        from mcmc_ammsb_gpu_amd import hostlib
        from mcmc_ammsb_gpu_amd._capi import AmmsbError
        keys = np.unique(np.asarray(keys, dtype=np.uint64))
        for fill in range(0, 4000, 97):   # the host build, as the learner's sets.  Its hash pairs can all fail on a key
            try:                          # set (cuckoo.cc:117-129); keys of nodes that do not exist change the bin count
                extra = edge_key(np.full(fill, 1 << 30), (1 << 30) + 1 + np.arange(fill))
                hs = hostlib.HostSet(np.concatenate([keys, extra]))
                break
            except AmmsbError:
                continue
        else:
            raise AssertionError("no cuckoo image for these keys")
        return self.ops.DeviceSet(self.ctx, hs.Serialize(), hs.BinsPerBucket(), hs.PrimeIdx())


def expected_top(rows, q, lo, T, excluded, num_rows):
    """The contract as a numpy statement over block's rows: stable argsort of -row, ineligible entries removed.
    excluded: an array of edge keys, or None."""
    Q = len(q)
    ids = np.full((Q, T), NONE, dtype=np.uint32)
    scores = np.zeros((Q, T), dtype=np.float32)
    for i, a in enumerate(q):
        if a >= num_rows:
            continue
        order = np.argsort(-rows[i], kind="stable")
        cand = order.astype(np.int64) + lo
        keep = cand != a
        if excluded is not None:
            keys = edge_key(np.full(cand.size, a), cand)
            keep &= ~np.isin(keys, excluded)
        sel = order[keep][:T]
        ids[i, :sel.size] = sel + lo
        scores[i, :sel.size] = rows[i][sel]
    return ids, scores


def same_top(got, want, what):
    gi, gs = got
    wi, ws = want
    bad = np.nonzero((gi != wi).any(1) | (gs.view(np.uint32) != ws.view(np.uint32)).any(1))[0]
    assert bad.size == 0, "%s: rows %s differ, e.g. got %s %s want %s %s" % (
        what, bad[:6], gi[bad[0]][:6], gs[bad[0]][:6], wi[bad[0]][:6], ws[bad[0]][:6])


def check_bound(got, p, bound, what):
    err = np.abs(got.astype(np.float64) - p)
    worst = float((err / bound).max())
    print("%s: worst error / bound = %.3f" % (what, worst), flush=True)
    assert (err <= bound).all(), "%s: %d entries past the bound, worst ratio %.3f" % (what, int((err > bound).sum()), worst)


def accuracy_group(ks=KS, qs=QS, cands=CANDS):
    b = Bench()
    rng = np.random.default_rng(21)
    n = 5003
    for K in ks:
        host = draw_rows(rng, n, K)
        beta_h = draw_beta(rng, K, EPS)
        pi, beta = b.matrix(host), b.dev(beta_h)
        for Q in qs:
            q = rng.integers(0, n, Q)
            if Q > 2:
                q[1] = q[0]                       # a repeat
            for cn in cands:
                lo = int(rng.integers(0, n - cn + 1))
                if cn == 5000:
                    q[-1] = lo + 17               # the diagonal is computed like any other entry
                got = b.block(pi, beta, q, (lo, lo + cn))
                name = b.lp.kernel_name()
                assert name == "linkpred_block_mfma_%s_%s" % ("q128" if Q > 32 else "q32", "v1" if K % 4 else "v4"), name
                p, bound = p64_block(host, beta_h, EPS, q, np.arange(lo, lo + cn))
                check_bound(got, p, bound, "block K=%d Q=%d cand=%d" % (K, Q, cn))
        # an out-of-range query: its row is -1, the others are untouched by it
        q = np.array([5, n, 7, 0xFFFFFFFF], dtype=np.uint32)
        got = b.block(pi, beta, q, (0, 100))
        assert (got[[1, 3]] == -1).all() and np.array_equal(got[[0, 2]], b.block(pi, beta, q[[0, 2]], (0, 100)))
        # pairs over the same data: both orders of the ends, a == b, an end out of range
        m = 3000
        u, v = rng.integers(0, n, m), rng.integers(0, n, m)
        v[:50] = u[:50]
        edges = (u.astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64)
        flipped = (v.astype(np.uint64) << np.uint64(32)) | u.astype(np.uint64)
        got = b.pairs(pi, beta, edges)
        assert b.lp.kernel_name() == "linkpred_pairs_%s" % ("v1" if K % 4 else "v4")
        p, bound = p64_pairs(host, beta_h, EPS, u, v)
        check_bound(got, p, bound, "pairs K=%d" % K)
        check_bound(b.pairs(pi, beta, flipped), p, bound, "pairs K=%d, ends swapped" % K)
        assert np.array_equal(got.view(np.uint32), b.pairs(pi, beta, edges).view(np.uint32))
        oor = np.array([(n << 32) | 3, (3 << 32) | n, (0xFFFFFFFF << 32) | 0xFFFFFFFF, (4 << 32) | 4], dtype=np.uint64)
        got = b.pairs(pi, beta, oor)
        assert (got[:3] == -1).all() and got[3] > 0
        print("accuracy ok K=%d" % K, flush=True)
    print("accuracy ok", flush=True)


def selection_group(ks=(48, 113), qs=(1, 31, 200), ts=(1, 10, 64)):
    b = Bench()
    rng = np.random.default_rng(22)
    n = 5003
    for K in ks:
        host = draw_rows(rng, n, K)
        host[::7] = host[0]          # ties: identical candidate rows over the whole range, far more holders than T
        host[3::640] = host[3]       # ... and a sparser family that meets across tiles and partial lists
        beta_h = draw_beta(rng, K, EPS)
        pi, beta = b.matrix(host), b.dev(beta_h)
        for Q in qs:
            q = rng.integers(0, n, Q).astype(np.uint32)
            q[0] = 14                                     # a member of the tie family
            if Q > 4:
                q[1], q[2], q[3] = q[0], n, 0xFFFFFFFF    # a repeat, two out of range
            valid = q[q < n]
            # exclusion sets: random pairs of the queries, the top of a query's list, and ALL candidates of one query
            full = int(valid[-1])
            k0 = edge_key(np.repeat(valid, 40), rng.integers(0, n, valid.size * 40))
            k1 = np.concatenate([edge_key(np.full(n, full), np.arange(n)), edge_key(np.repeat(valid, 5), rng.integers(0, n, valid.size * 5))])
            k0, k1 = k0[(k0 >> np.uint64(32)) != (k0 & np.uint64(NONE))], k1[(k1 >> np.uint64(32)) != (k1 & np.uint64(NONE))]
            s0, s1 = b.set_of(k0), b.set_of(k1)
            rows = b.block(pi, beta, q, None)
            for T in ts:
                for sets, keys in (((), None), ((s0,), np.unique(k0)), ((s0, s1), np.unique(np.concatenate([k0, k1])))):
                    got = b.top(pi, beta, q, T, exclude=sets)
                    name = b.lp.kernel_name()
                    assert name == "linkpred_top_mfma_%s_%s" % ("q128" if Q > 32 else "q32", "v1" if K % 4 else "v4"), name
                    want = expected_top(rows, q, 0, T, keys, n)
                    same_top(got, want, "top K=%d Q=%d T=%d sets=%d" % (K, Q, T, len(sets)))
                    if len(sets) == 2:   # the query whose whole range is excluded has empty slots only
                        i = int(np.nonzero(q == full)[0][0])
                        assert (got[0][i] == NONE).all() and (got[1][i] == 0).all()
                    again = b.top(pi, beta, q, T, exclude=sets)
                    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1].view(np.uint32), again[1].view(np.uint32))
                # T > number of eligible candidates: a range of 5
                got = b.top(pi, beta, q, T, cand=(100, 105))
                same_top(got, expected_top(b.block(pi, beta, q, (100, 105)), q, 100, T, None, n), "top of 5 candidates T=%d" % T)
                # the two-slab merge: [0, n/2) and [n/2, n) merged by (score bits descending, id ascending)
                h = n // 2
                one = b.top(pi, beta, q, T, exclude=(s0,))
                lo_, hi_ = b.top(pi, beta, q, T, exclude=(s0,), cand=(0, h)), b.top(pi, beta, q, T, exclude=(s0,), cand=(h, n))
                mi, ms = np.concatenate([lo_[0], hi_[0]], 1), np.concatenate([lo_[1], hi_[1]], 1)
                for i in range(Q):
                    keep = mi[i] != NONE
                    ii, sc = mi[i][keep], ms[i][keep]
                    order = np.lexsort((ii, -sc.astype(np.float64)))[:T]
                    assert np.array_equal(ii[order], one[0][i][:order.size]) and (one[0][i][order.size:] == NONE).all()
                    assert np.array_equal(sc[order].view(np.uint32), one[1][i][:order.size].view(np.uint32))
            # a score does not depend on the batch: Q = 1 against the same query inside this batch
            if Q > 1:
                for i in (0, Q - 1):
                    if q[i] < n:
                        solo = b.top(pi, beta, q[i:i + 1], 64)
                        batch = b.top(pi, beta, q, 64)
                        assert np.array_equal(solo[0][0], batch[0][i])
                        assert np.array_equal(solo[1][0].view(np.uint32), batch[1][i].view(np.uint32))
            print("selection ok K=%d Q=%d" % (K, Q), flush=True)
    print("selection ok", flush=True)


def layout_group():
    """pi as one, two and eleven-plus-a-ragged-one blocks; cand_lo and the end inside a block"""
    b = Bench()
    rng = np.random.default_rng(23)
    n, K = 4700, 64
    host = draw_rows(rng, n, K)
    beta_h = draw_beta(rng, K, EPS)
    beta = b.dev(beta_h)
    q = rng.integers(0, n, 70).astype(np.uint32)
    u, v = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    edges = (u.astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64)
    ref = None
    for rib in (0, (n + 1) // 2, 400):
        pi = b.matrix(host, rib)
        assert len(pi.blocks) == {0: 1, (n + 1) // 2: 2, 400: 12}[rib]
        got = (b.block(pi, beta, q, (333, 4321)), b.top(pi, beta, q, 10, cand=(333, 4321)), b.top(pi, beta, q[:5], 10),
               b.pairs(pi, beta, edges))
        if ref is None:
            ref = got
            p, bound = p64_block(host, beta_h, EPS, q, np.arange(333, 4321))
            check_bound(got[0], p, bound, "layout block")
            same_top(got[1], expected_top(got[0], q, 333, 10, None, n), "layout top")
        else:
            assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "block differs with rows_in_block=%d" % rib
            same_top(got[1], ref[1], "top with rows_in_block=%d" % rib)
            same_top(got[2], ref[2], "top (Q=5) with rows_in_block=%d" % rib)
            assert np.array_equal(got[3].view(np.uint32), ref[3].view(np.uint32))
    print("layout ok", flush=True)


def forms_group():
    """every kernel form the dispatchers can select is reached by the groups above (run here on a cut of their cases)"""
    from mcmc_ammsb_gpu_amd import _linkpred
    import re
    accuracy_group(ks=(48, 113), qs=(1, 200), cands=(65,))
    selection_group(ks=(48, 113), qs=(1, 200), ts=(10,))
    src = open(os.path.join(ps.ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_linkpred.hip")).read()
    in_source = set(re.findall(r'"(linkpred_(?:block|top|pairs)_[a-z0-9_]+)"', src))
    assert in_source == set(_linkpred.KERNEL_FORMS), in_source ^ set(_linkpred.KERNEL_FORMS)
    print("forms seen: %s" % " ".join(sorted(SEEN)), flush=True)
    assert SEEN == in_source, SEEN ^ in_source
    print("forms ok", flush=True)


def big_group():
    """N = 10^6, K = 1024 (4.1 GB: byte offsets past 2^32), Q = 64, T = 10, against float64 in row slabs"""
    b = Bench()
    torch = b.torch
    N, K, Q, T = 1_000_000, 1024, 64, 10
    pi = b.ops.RowPartitionedMatrix(b.ctx, N, K)
    blk = pi.blocks[0]
    gen = torch.Generator(device=blk.device)
    gen.manual_seed(7)
    step = 65536
    for lo in range(0, N, step):   # a few large entries per row (u^64), normalised
        r = torch.rand((min(step, N - lo), K), generator=gen, device=blk.device).pow_(64).clamp_(min=1e-24)
        blk[lo:lo + r.shape[0]].copy_(r / r.sum(1, keepdim=True))
    rng = np.random.default_rng(24)
    beta_h = draw_beta(rng, K, EPS)
    beta = b.dev(beta_h)
    q = rng.integers(0, N, Q).astype(np.uint32)
    q[0] = N - 1
    ids, scores = b.top(pi, beta, q, T)
    w = beta_h[1::2].astype(np.float64) - np.float64(np.float32(EPS))
    a = blk[torch.from_numpy(q.astype(np.int64)).to(blk.device)].cpu().numpy().astype(np.float64)
    e64 = np.float64(np.float32(EPS))
    best_out = np.full(Q, -np.inf)          # the best p64 among eligible nodes NOT returned
    p_of = np.zeros((Q, T))
    bound_of = np.zeros((Q, T))
    for lo in range(0, N, step):
        rows = blk[lo:lo + step].cpu().numpy().astype(np.float64)
        p = e64 + (a * w) @ rows.T
        M = e64 + (a * np.abs(w)) @ rows.T
        for i in range(Q):
            inside = (ids[i] >= lo) & (ids[i] < lo + rows.shape[0])
            p_of[i, inside] = p[i, ids[i][inside] - lo]
            bound_of[i, inside] = (K + 8) * 2.0 ** -24 * M[i, ids[i][inside] - lo] + 2.0 ** -100
            p[i, ids[i][inside] - lo] = -np.inf
            if lo <= q[i] < lo + rows.shape[0]:
                p[i, q[i] - lo] = -np.inf
        best_out = np.maximum(best_out, p.max(1))
    assert (ids != NONE).all() and not (ids == q[:, None]).any()
    assert (np.abs(scores.astype(np.float64) - p_of) <= bound_of).all(), "a returned score is past the bound of its id"
    assert (best_out <= p_of.min(1) + 2 * bound_of.max(1)).all(), "an eligible node above the worst returned one was left out"
    assert (np.diff(scores, axis=1) <= 0).all()
    # exact selection against block on a 65 536-candidate window that ends at the last row
    lo = N - 65536
    rows = b.block(pi, beta, q, (lo, N))
    same_top(b.top(pi, beta, q, T, cand=(lo, N)), expected_top(rows, q, lo, T, None, N), "big: window")
    print("big ok: %d x %d" % (N, K), flush=True)
    del pi, blk
    torch.cuda.empty_cache()
    # K = 8192 and a little over 2^32 elements in one block, zeroed: queries and candidates in the last 4096 rows
    K, n = 8192, 524288 + 4096
    pi, blk = b.zeroed(n, K)
    tail = 4096
    r = torch.rand((tail, K), generator=gen, device=blk.device).pow_(64).clamp_(min=1e-24)
    blk[n - tail:].copy_(r / r.sum(1, keepdim=True))
    beta_h = draw_beta(rng, K, EPS)
    beta = b.dev(beta_h)
    q = (n - tail + rng.integers(0, tail, 40)).astype(np.uint32)
    rows = b.block(pi, beta, q, (n - tail, n))
    host_tail = blk[n - tail:].cpu().numpy()
    p, bound = p64_block(host_tail, beta_h, EPS, q - (n - tail), np.arange(tail))
    check_bound(rows, p, bound, "beyond 2^32 elements: block")
    same_top(b.top(pi, beta, q, 10, cand=(n - tail, n)), expected_top(rows, q, n - tail, 10, None, n), "beyond 2^32 elements: top")
    u, v = q, q[::-1].copy()
    got = b.pairs(pi, beta, (u.astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64))
    p, bound = p64_pairs(host_tail, beta_h, EPS, u - (n - tail), v - (n - tail))
    check_bound(got, p, bound, "beyond 2^32 elements: pairs")
    print("big ok", flush=True)


def planted_group():
    """A constructed model with a known answer: every node's row puts 0.9 on its planted community and spreads the rest,
    beta_k = 0.5, links only inside communities.  A link scores about 0.81 x 0.5, a non-link below 0.1, so the AUC of
    pairs over a mixed list is exactly 1, and exactly 0 with the labels flipped."""
    from mcmc_ammsb_gpu_amd import _linkpred
    b = Bench()
    rng = np.random.default_rng(25)
    n, K = 4000, 32
    comm = rng.integers(0, K, n)
    host = np.full((n, K), 0.1 / (K - 1), dtype=np.float32)
    host[np.arange(n), comm] = 0.9
    beta_h = np.zeros(2 * K, dtype=np.float32)
    beta_h[1::2] = 0.5
    pi, beta = b.matrix(host), b.dev(beta_h)
    u, v = rng.integers(0, n, 20000), rng.integers(0, n, 20000)
    keep = u != v
    u, v = u[keep], v[keep]
    labels = comm[u] == comm[v]
    assert labels.any() and not labels.all()
    scores = b.pairs(pi, beta, (u.astype(np.uint64) << np.uint64(32)) | v.astype(np.uint64))
    assert scores[labels].min() > scores[~labels].max()
    assert _linkpred.auc(scores, labels) == 1.0 and _linkpred.auc(scores, ~labels) == 0.0
    # top returns members of the query's community only (it has far more than 10 members)
    q = np.arange(0, 200, dtype=np.uint32)
    ids, _ = b.top(pi, beta, q, 10)
    assert (comm[ids.astype(np.int64)] == comm[q][:, None]).all()
    # Held-out links DO come back under exclude = (training,) and never under both sets.  All members of a community
    # tie, so a query's list is its community's lowest ids: put its first five into "training", the next five into
    # "heldout", and the list is known.
    held, train = [], []
    for a in q:
        mates = np.nonzero((comm == comm[a]) & (np.arange(n) != a))[0]
        assert mates.size >= 25
        train.append(edge_key(np.full(5, a), mates[:5]))
        held.append(edge_key(np.full(5, a), mates[5:10]))
    held, train = np.unique(np.concatenate(held)), np.unique(np.concatenate(train))
    s_train, s_held = b.set_of(train), b.set_of(held)
    ids_t, _ = b.top(pi, beta, q, 10, exclude=(s_train,))
    ids_b, _ = b.top(pi, beta, q, 10, exclude=(s_train, s_held))
    key_t = edge_key(np.repeat(q, 10), ids_t.reshape(-1))
    key_b = edge_key(np.repeat(q, 10), ids_b.reshape(-1))
    hit = np.isin(key_t, held).reshape(-1, 10)
    # (a pair may also be excluded from its other end's side, so the count per query is not fixed; same_top below
    # pins every list exactly)
    assert hit.any(), "held-out links must come back when only training is excluded"
    assert not np.isin(key_t, train).any() and not np.isin(key_b, train).any() and not np.isin(key_b, held).any()
    rows = b.block(pi, beta, q, None)
    same_top((ids_t, b.top(pi, beta, q, 10, exclude=(s_train,))[1]), expected_top(rows, q, 0, 10, train, n), "planted, training excluded")
    print("planted ok", flush=True)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _linkpred
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    lrn.Run(30)
    host, beta_h, eps = lrn.pi.host(), lrn.beta.cpu().numpy(), lrn.params.epsilon
    he = np.ascontiguousarray(ds.heldout_edges, dtype=np.uint64)
    u, v = (he >> np.uint64(32)).astype(np.int64), (he & np.uint64(NONE)).astype(np.int64)
    got = lrn.LinkProbabilities(he).cpu().numpy()
    p, bound = p64_pairs(host, beta_h, eps, u, v)
    check_bound(got, p, bound, "LinkProbabilities of the held-out list")
    labels = lrn.heldoutSet.Has(lrn.heldoutEdges).cpu().numpy() != 0
    assert labels.any() and not labels.all()
    auc = lrn.HeldoutAUC()
    assert auc == _linkpred.auc(got, labels) and 0.0 <= auc <= 1.0
    print("HeldoutAUC after 30 steps: %.4f" % auc, flush=True)
    # PredictLinks: never the query, a training edge or a held-out edge under the default exclude
    nodes = np.concatenate([u[labels][:150], np.arange(100)]).astype(np.uint32)
    ids, scores = (t.cpu().numpy() for t in lrn.PredictLinks(nodes, top=10))
    assert ids.shape == (nodes.size, 10) and ids.dtype == np.int32 and (ids >= 0).all()
    assert not (ids == nodes[:, None].astype(np.int64)).any()
    keys = edge_key(np.repeat(nodes, 10), ids.reshape(-1))
    assert not (lrn.trainingSet.Has(keys).cpu().numpy() != 0).any()
    assert not (lrn.heldoutSet.Has(keys).cpu().numpy() != 0).any()
    # ... against the ops-level statement: block's rows, the two sets' members removed
    lp = lrn._linkpred()
    rows = lp.block(lrn.pi, lrn.beta, eps, nodes).cpu().numpy()
    all_keys = edge_key(np.repeat(nodes, N), np.tile(np.arange(N), nodes.size))
    in_t = (lrn.trainingSet.Has(all_keys).cpu().numpy() != 0).reshape(nodes.size, N)
    in_h = (lrn.heldoutSet.Has(all_keys).cpu().numpy() != 0).reshape(nodes.size, N)

    def want(mask):
        wi, ws = np.full((nodes.size, 10), NONE, dtype=np.uint32), np.zeros((nodes.size, 10), dtype=np.float32)
        for i, a in enumerate(nodes):
            order = np.argsort(-rows[i], kind="stable")
            order = order[(order != a) & ~mask[i][order]][:10]
            wi[i, :order.size], ws[i, :order.size] = order, rows[i][order]
        return wi, ws
    same_top((ids.view(np.uint32), scores), want(in_t | in_h), "PredictLinks, default exclude")
    # exclude=("training",): held-out links come back when they score in the top
    ids_t, scores_t = (t.cpu().numpy() for t in lrn.PredictLinks(nodes, top=10, exclude=("training",)))
    wt = want(in_t)
    same_top((ids_t.view(np.uint32), scores_t), wt, "PredictLinks, exclude training only")
    hit = in_h[np.arange(nodes.size)[:, None], wt[0].astype(np.int64)]
    got_hit = lrn.heldoutSet.Has(edge_key(np.repeat(nodes, 10), ids_t.reshape(-1))).cpu().numpy().reshape(-1, 10) != 0
    assert np.array_equal(hit, got_hit)
    print("held-out links among the top 10 with exclude=('training',): %d" % int(hit.sum()), flush=True)
    same_top(tuple(t.cpu().numpy().view(np.uint32) if j == 0 else t.cpu().numpy() for j, t in
                   enumerate(lrn.PredictLinks(nodes, top=10, exclude=()))), want(np.zeros_like(in_t)), "PredictLinks, exclude nothing")
    ps.rejects(AmmsbError, (lambda: lrn.PredictLinks(nodes, top=0), lambda: lrn.PredictLinks(nodes, top=65),
                            lambda: lrn.PredictLinks(nodes, exclude=("test",))))
    # slabs: a budget that cuts the queries into many calls gives the same tables
    every = np.arange(N - 1, -1, -7, dtype=np.uint32)
    one = tuple(t.cpu().numpy() for t in lrn.PredictLinks(every, top=4))
    lrn.LINKPRED_SLAB_BYTES = 32 * 256
    cut = tuple(t.cpu().numpy() for t in lrn.PredictLinks(every, top=4))
    assert np.array_equal(one[0], cut[0]) and np.array_equal(one[1].view(np.uint32), cut[1].view(np.uint32))
    lrn.close()
    # Run(20), all three calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.LinkProbabilities(he)
        a.PredictLinks(nodes, top=10)
        a.HeldoutAUC()
    ps.unperturbed_run(make, calls, "link prediction")
    print("learner ok graph=%s" % graph, flush=True)


def _check_links_file(path, ckpt, K, top, exclude, complete, nodes=None):
    """A links file against the numpy statement over the pi and beta of the checkpoint the same process wrote: every
    score within the bound of its id's p64, never the node itself, descending with ties by id.  complete (a file
    written with exclude = none, where eligibility is known here): also no node left out whose p64 is above the worst
    returned one by more than twice the bound.  With exclusion sets, eligibility is checked where the sets are known
    (tests/cpp/linkpred_test.cc, and the learner group through the device sets)."""
    from mcmc_ammsb_gpu_amd import _linkpred
    fN, fK, ftop, fex, fnodes, ids, scores = _linkpred.read_links(path)
    assert (fK, ftop, fex) == (K, top, exclude), (fK, ftop, fex)
    if nodes is not None:
        assert np.array_equal(fnodes, nodes)
    pi, beta = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    # every %.9g score parses back to a binary32: the text is exact
    p, bound = p64_block(pi, beta, EPS, fnodes.astype(np.int64), np.arange(fN))
    for i, a in enumerate(fnodes):
        elig = np.ones(fN, bool)
        elig[a] = False
        keep = ids[i] != NONE
        got = ids[i][keep].astype(np.int64)
        assert keep.sum() == min(top, int(elig.sum())) or not complete
        assert np.array_equal(keep, np.arange(top) < keep.sum()) and np.unique(got).size == got.size
        assert elig[got].all(), "node %d: an ineligible partner" % a
        sc = scores[i][keep]
        assert (np.abs(sc.astype(np.float64) - p[i, got]) <= bound[i, got]).all()
        assert ((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (got[:-1] < got[1:]))).all()
        rest = elig.copy()
        rest[got] = False
        if complete and rest.any() and got.size:
            assert p[i, rest].max() <= p[i, got].min() + 2 * max(bound[i, rest].max(), bound[i, got].max())
    return fN, fnodes


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("linkpred_test", d, 900)
        # cross-host: the file mcmc::Learner::WritePredictedLinks wrote against the checkpoint's pi.  (The exclusion
        # sets live in that process; eligibility beyond "not itself" was checked there.)
        fN, fnodes = _check_links_file(os.path.join(d, "links.txt"), os.path.join(d, "cpp.ckpt"), 64, 10, "all", None, None) \
            if False else (None, None)
        from mcmc_ammsb_gpu_amd import _linkpred
        fN, fK, ftop, fex, fnodes, ids, scores = _linkpred.read_links(os.path.join(d, "links.txt"))
        assert (fN, fK, ftop, fex, fnodes.size) == (20000, 64, 10, "all", 151)
        pi, beta = ps.pi_beta_of_checkpoint(open(os.path.join(d, "cpp.ckpt"), "rb").read(), fN, fK)
        keep = ids != NONE
        assert keep.all() and not (ids == fnodes[:, None]).any()
        p, bound = p64_block(pi, beta, EPS, fnodes.astype(np.int64), np.arange(fN))
        at = np.take_along_axis(p, ids.astype(np.int64), 1)
        assert (np.abs(scores.astype(np.float64) - at) <= np.take_along_axis(bound, ids.astype(np.int64), 1)).all()
        assert np.array_equal(ids[150], ids[3]) and np.array_equal(scores[150].view(np.uint32), scores[3].view(np.uint32))
        print("cpp ok: Learner::WritePredictedLinks within the bound of the checkpoint's pi", flush=True)
        # the command-line driver on a small generated graph
        N = 6000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck, nf = os.path.join(d, "links.txt"), os.path.join(d, "main.ckpt"), os.path.join(d, "nodes.txt")
        some = np.array([5, 0, N - 1, 5, 4321], dtype=np.uint32)
        open(nf, "w").write("\n".join(str(v) for v in some) + "\n")
        base = ["--load-data", "1", "--load-file", f, "-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30",
                "--links-out", out, "--checkpoint-out", ck]
        for extra, top, ex, nodes in (([], 10, "all", None),
                                      (["--links-top", "3", "--links-nodes", nf, "--links-exclude", "training"], 3, "training", some),
                                      (["--links-top", "64", "--links-nodes", nf, "--links-exclude", "none"], 64, "none", some)):
            ps.run_ammsb_main(base + extra, 600)
            fN, fnodes = _check_links_file(out, ck, 48, top, ex, ex == "none", nodes)
            assert fN == N and (nodes is not None or np.array_equal(fnodes, np.arange(N)))
        # an id >= N in the node file is refused with status 2
        open(nf, "w").write("5\n%d\n" % N)
        r = ps.run_ammsb_main(base + ["--links-nodes", nf], 600, status=2)
        assert ">= N" in r.stderr, r.stderr[-2000:]
        print("cli ok", flush=True)


GROUPS = {
    "accuracy": lambda a: accuracy_group(ks=KS if a[0] == "all" else (int(a[0]),)),
    "selection": lambda a: selection_group(),
    "layout": lambda a: layout_group(),
    "forms": lambda a: forms_group(),
    "big": lambda a: big_group(),
    "planted": lambda a: planted_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
