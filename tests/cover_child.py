"""Child process of test_gpu_cover.py (one per group): matching the detected cover to a ground-truth cover
(include/ammsb_cover.h, ops.CoverMatch, Learner.CompareCover) against the numpy statement, every figure exactly equal:

    M = pi >= np.float32(thr);  d = M.sum(0);  overlap[g] = M[the valid members of g].sum(0);  t_g = their number
    truth_best[g]    = the lowest k among those with overlap > 0 that maximise overlap / (t_g + d_k), else -1
    detected_best[k] = the lowest g among those with overlap > 0 that maximise overlap / (t_g + d_k), else -1
    skipped          = the members >= N

The rationals are compared by integer cross-multiplication (reference() asserts that statement for every winner)."""
import ctypes as C
import io
import os
import sys

import numpy as np

import postfit_support as ps

from quality_child import ABOVE, BELOW, PLANTED, draw_rows, planted_cols  # noqa: F401  (the rows of the sibling group)

NONE = 0xFFFFFFFF
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A
SEEN = set()
F32 = np.float32
UNIT = 128


def reference(pi, thr, offsets, members):
    """-> dict of the outputs, overlap [G, K] int64 among them"""
    N, K = pi.shape
    G = offsets.size - 1
    with np.errstate(invalid="ignore"):
        M = pi >= F32(thr)
    d = M.sum(0).astype(np.int64)
    ov = np.zeros((G, K), dtype=np.int64)
    t = np.zeros(G, dtype=np.int64)
    skipped = 0
    for g in range(G):
        mem = members[int(offsets[g]):int(offsets[g + 1])].astype(np.int64)
        ok = mem < N
        skipped += int((~ok).sum())
        t[g] = ok.sum()
        if t[g]:
            ov[g] = M[mem[ok]].sum(0)          # (a duplicated member's row is added twice: counted as written)
    s = t[:, None] + d[None, :]
    assert int(ov.max(initial=0)) * int(s.max(initial=1)) < 2**62 and int(s.max(initial=1))**2 < 2**50
    # distinct rationals with denominators below 2^25 differ in float64, equal ones round alike; argmax takes the first
    ratio = np.where(ov > 0, ov / np.maximum(s, 1), -1.0)
    tb = np.where((ov > 0).any(1), ratio.argmax(1), -1).astype(np.int32)
    db = np.where((ov > 0).any(0), ratio.argmax(0), -1).astype(np.int32)
    to = np.where(tb >= 0, ov[np.arange(G), np.maximum(tb, 0)], 0)
    do = np.where(db >= 0, ov[np.maximum(db, 0), np.arange(K)], 0)
    # ... and the statement itself, in integers: no candidate beats the winner, and none before it equals it
    for g in np.flatnonzero(tb >= 0):
        b = tb[g]
        lhs, rhs = ov[g] * s[g, b], ov[g, b] * s[g]
        assert (lhs <= rhs).all() and (lhs[:b] < rhs[:b]).all(), "the reference breaks its statement at g=%d" % g
    for k in np.flatnonzero(db >= 0):
        b = db[k]
        lhs, rhs = ov[:, k] * s[b, k], ov[b, k] * s[:, k]
        assert (lhs <= rhs).all() and (lhs[:b] < rhs[:b]).all(), "the reference breaks its statement at k=%d" % k
    return dict(truth_best=tb, truth_overlap=to.astype(np.uint32), truth_size=t.astype(np.uint32), detected_best=db,
                detected_overlap=do.astype(np.uint32), skipped=skipped, overlap=ov.astype(np.uint32), detected_size=d)


NAMES = ("truth_best", "truth_overlap", "truth_size", "detected_best", "detected_overlap")


def check(got, ref, what, dense=True):
    for n in NAMES:
        bad = np.flatnonzero(got[n] != ref[n])
        assert not bad.size, "%s: %s differs at %s: got %s, want %s" % (what, n, bad[:8], got[n][bad[:8]], ref[n][bad[:8]])
    assert got["skipped"] == ref["skipped"], "%s: skipped %d, want %d" % (what, got["skipped"], ref["skipped"])
    if dense and got.get("overlap") is not None:
        bad = np.argwhere(got["overlap"] != ref["overlap"])
        assert not bad.size, "%s: the dense overlap differs at %s" % (what, bad[:8].tolist())


def make_cover(rng, N, sizes, spoil=True):
    """communities of the given sizes, distinct members inside each; with `spoil`, a member == N, a member == 2^32 - 1
    and a duplicated member planted where the sizes allow it (the sizes stay what they are)"""
    lists = [rng.choice(N, int(sz), replace=False).astype(np.uint32) for sz in sizes]
    if spoil:
        big = [i for i, c in enumerate(lists) if c.size >= 5]
        for n, i in enumerate(big[:6]):
            if n % 3 == 0:
                lists[i][1] = N
            elif n % 3 == 1:
                lists[i][-1] = NONE
                lists[i][0] = N
            else:
                lists[i][3] = lists[i][2]          # a duplicate, next to its twin
        if len(big) > 6:
            lists[big[6]][-1] = lists[big[6]][0]   # ... and far from it
    offsets = np.zeros(len(lists) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([c.size for c in lists])
    members = np.concatenate(lists) if lists else np.zeros(0, np.uint32)
    return offsets, members.astype(np.uint32)


def special_sizes(G, rng):
    """the sizes at which a community ends on, just before and just after a unit boundary, and one that spans several"""
    if G == 1:
        return [3 * UNIT + 5]
    if G == 7:
        return [UNIT - 1, 1, UNIT, 0, UNIT + 1, 3 * UNIT + 5, 65]      # (the second and third end on a boundary)
    head = [0, 1, 2, 63, 64, 65, UNIT - 1, UNIT, UNIT + 1, 3 * UNIT + 5, 0, 0, UNIT - 3, 3, UNIT]
    return head + rng.integers(0, 40, G - len(head)).tolist()


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _cover
        super().__init__()
        self.cv = _cover
        self.lib = _cover.load()
        self.api = self.ops.CoverMatch(self.ctx)
        self.ro = self.ops.CommunityReadout(self.ctx)
        assert _cover.UNIT == UNIT

    def match(self, pi, thr, offsets, members, dense=True, dsize=None):
        """the library call over buffers of this test's own, each followed by GUARD words that must survive
        -> the outputs as numpy arrays"""
        t = self.torch
        K, G, M = int(pi.cols), offsets.size - 1, members.size
        if dsize is None:
            dsize = self.ro.sizes(pi, thr)
        d_off, d_mem = self.ctx.from_numpy(offsets), self.ctx.from_numpy(members)
        nbytes = int(self.lib.ammsb_cover_workspace_bytes(M, K))
        assert nbytes % 8 == 0 and nbytes > 0
        bufs = dict(truth_best=self.guarded(G, t.int32, FILL32), truth_overlap=self.guarded(G, t.int32, FILL32),
                    truth_size=self.guarded(G, t.int32, FILL32), detected_best=self.guarded(K, t.int32, FILL32),
                    detected_overlap=self.guarded(K, t.int32, FILL32), skipped=self.guarded(1, t.int64, FILL64),
                    ws=self.guarded(nbytes // 8, t.int64, FILL64))
        if dense:
            bufs["overlap"] = self.guarded(G * K, t.int32, FILL32)
        ptr = lambda n: C.c_void_p(bufs[n].data_ptr()) if n in bufs else None   # noqa: E731
        self.cv.check(self.lib.ammsb_cover_match(C.byref(pi.desc), thr, C.c_void_p(d_off.data_ptr()), G,
                                                 C.c_void_p(d_mem.data_ptr()), M, C.c_void_p(dsize.data_ptr()),
                                                 ptr("truth_best"), ptr("truth_overlap"), ptr("truth_size"),
                                                 ptr("detected_best"), ptr("detected_overlap"), ptr("skipped"),
                                                 ptr("overlap"), ptr("ws"), nbytes, None))
        t.cuda.synchronize()
        SEEN.add(self.cv.last_kernel_name())
        out = {}
        words = dict(truth_best=G, truth_overlap=G, truth_size=G, detected_best=K, detected_overlap=K, skipped=1,
                     ws=nbytes // 8, overlap=G * K)
        for n, buf in bufs.items():
            h = buf.cpu().numpy()
            fill = FILL64 if buf.dtype == t.int64 else FILL32
            assert (h[words[n]:] == fill).all(), "the words past %s were written" % n
            if n in ("truth_best", "detected_best"):
                out[n] = h[:words[n]]
            elif n == "skipped":
                out[n] = int(h[0])
            elif n == "overlap":
                out[n] = h[:words[n]].view(np.uint32).reshape(G, K)
            elif n != "ws":
                out[n] = h[:words[n]].view(np.uint32)
        out["detected_size"] = dsize.cpu().numpy()
        return out


def thresholds():
    return (("0", 0.0), ("0.05", 0.05), ("planted", float(PLANTED)), ("above", ABOVE))


def tie_matrix():
    """planted ties and near-ties, worked by hand (N = 9000, K = 9, threshold 0.5; G = 9)"""
    N, K = 9000, 9
    pi = np.zeros((N, K), dtype=F32)
    # equal rationals, the lower k wins: g0 = {0, 1, 2}: column 0 gives 1 / (3 + 1), column 1 gives 2 / (3 + 5)
    pi[[0], 0] = 1
    pi[[1, 2, 10, 11, 12], 1] = 1
    # ... also when the larger pair comes first: g1 = {3, 4, 5}: column 2 gives 2 / 8, column 3 gives 1 / 4
    pi[[3, 4, 13, 14, 15], 2] = 1
    pi[[5], 3] = 1
    # the mirror image over g: column 4 = {20, 21, 22}: g2 = {20} gives 1 / (1 + 3), g3 = {21 .. 25} gives 2 / (5 + 3)
    pi[[20, 21, 22], 4] = 1
    # two identical columns: column 5 is column 0 again
    pi[:, 5] = pi[:, 0]
    # rationals closer than a binary32 ulp of their quotient.  g4 = {100 .. 4195}, t = 4096: column 6 holds 4095 of
    # them and nobody else, 4095 / (4096 + 4095); column 7 holds all 4096 and one outsider, 4096 / (4096 + 4097):
    # 4095 * 8193 = 33550335 < 33550336 = 4096 * 8191, so the higher column wins by one unit of the cross product
    pi[100:4195, 6] = 1
    pi[100:4196, 7] = 1
    pi[8999, 7] = 1
    # the mirror image: column 8 = {4300 .. 8395}, d = 4096: g5 = 4095 of them, 4095 / (4095 + 4096); g6 = all of them
    # and one outsider, 4096 / (4097 + 4096): the higher g wins
    pi[4300:4396 + 4000, 8] = 1
    lists = [[0, 1, 2], [3, 4, 5], [20], [21, 22, 23, 24, 25], list(range(100, 4196)), list(range(4300, 8395)),
             list(range(4300, 8396)) + [8998], [], [30]]
    want_tb = [0, 2, 4, 4, 7, 8, 8, -1, -1]
    want_db = [0, 0, 1, 1, 2, 0, 4, 4, 6]
    return pi, lists, want_tb, want_db


def exact_group(ks):
    b = Bench()
    rng = np.random.default_rng(51)
    for K in ks:
        N = {1: 4999, 3: 1237}.get(K, 600 if K >= 1024 else 911)
        host, kind = draw_rows(rng, N, K)
        pi = b.matrix(host)
        covers = {G: make_cover(rng, N, special_sizes(G, rng)) for G in (1, 7, 300)}
        for name, thr in thresholds():
            dsize = b.ro.sizes(pi, thr)
            for G, (off, mem) in covers.items():
                what = "K=%d G=%d thr=%s" % (K, G, name)
                ref = reference(host, thr, off, mem)
                assert np.array_equal(dsize.cpu().numpy(), ref["detected_size"]), what
                got = b.match(pi, thr, off, mem, dense=True, dsize=dsize)
                check(got, ref, what)
                if G > 1:
                    assert ref["skipped"] >= 3, what
                if name == "above":
                    assert (got["truth_best"] == -1).all() and (got["detected_best"] == -1).all(), what
                    assert not got["truth_overlap"].any() and not got["overlap"].any(), what
                if name == "0" and G == 7:
                    assert (got["truth_best"][ref["truth_size"] > 0] >= 0).all(), what
                if name == "planted" and G == 7:   # the tie is a member, the next float below is not
                    pc = planted_cols(K)
                    rows4, rows5 = np.flatnonzero(kind == 4), np.flatnonzero(kind == 5)
                    o2, m2 = b.cv.check_cover([rows4[:70], rows5[:70]])
                    g2 = b.match(pi, thr, o2, m2, dense=True, dsize=dsize)
                    check(g2, reference(host, thr, o2, m2), what + ": planted rows")
                    assert (g2["overlap"][0][pc] == 70).all() and not g2["overlap"][1][pc].any(), what
                if G in (7, 300) and name in ("0.05", "planted"):
                    # the dense output off gives the same other outputs; a second call is bit-equal
                    lean = b.match(pi, thr, off, mem, dense=False, dsize=dsize)
                    again = b.match(pi, thr, off, mem, dense=True, dsize=dsize)
                    for n in NAMES + ("skipped",):
                        assert np.array_equal(got[n], lean[n]), what + ": dense off: " + n
                        assert np.array_equal(got[n], again[n]), what + ": second call: " + n
                    assert np.array_equal(got["overlap"], again["overlap"]), what + ": second call"
        # the layer above: ops.CoverMatch over its own tensors, host arrays and device tensors
        off, mem = covers[300]
        ref = reference(host, 0.05, off, mem)
        dsize = b.ro.sizes(pi, 0.05)
        for o_arg, m_arg in ((off, mem), (b.ctx.from_numpy(off), b.ctx.from_numpy(mem))):
            tb, to, ts, db, do, sk, ov = b.api.match(pi, 0.05, o_arg, m_arg, dsize, dense=True)
            u = lambda x: x.cpu().numpy().view(np.uint32)   # noqa: E731
            check(dict(truth_best=tb.cpu().numpy(), truth_overlap=u(to), truth_size=u(ts), detected_best=db.cpu().numpy(),
                       detected_overlap=u(do), skipped=int(sk.item()), overlap=u(ov)), ref, "ops K=%d" % K)
        tb, to, ts, db, do, sk, ov = b.api.match(pi, 0.05, np.zeros(1, np.uint64), np.zeros(0, np.uint32), dsize)
        assert tb.numel() == 0 and (db == -1).all().item() and not do.any().item() and ov is None
        tb, to, ts, db, do, sk, ov = b.api.match(pi, 0.05, np.zeros(4, np.uint64), np.zeros(0, np.uint32), dsize, dense=True)
        assert (tb == -1).all().item() and (db == -1).all().item() and not ov.any().item() and tuple(ov.shape) == (3, K)
        print("exact K=%d ok (%s)" % (K, b.cv.last_kernel_name()), flush=True)
    if 3 in ks:
        host, lists, want_tb, want_db = tie_matrix()
        pi = b.matrix(host)
        off, mem = b.cv.check_cover(lists)
        ref = reference(host, 0.5, off, mem)
        assert ref["truth_best"].tolist() == want_tb and ref["detected_best"].tolist() == want_db, (ref["truth_best"], ref["detected_best"])
        # (what a binary32 quotient cannot tell apart)
        assert F32(4095) / F32(8191) == F32(4096) / F32(8193)
        got = b.match(pi, 0.5, off, mem)
        check(got, ref, "planted ties")
        assert got["truth_overlap"][4] == 4096 and got["detected_overlap"][8] == 4096 and got["detected_best"][5] == 0
        print("ties ok", flush=True)
    print("exact ok", flush=True)


def persistent_group(ks):
    """More units than the grid has waves: at K = 8192 a CU holds one block of four waves (256 x 4 units in flight), at
    K <= 1024 eight blocks (2048 x 4), so every wave takes several units and asks for the next unit's first row while
    a community is finished.  Rows repeat (N = 600), so the pass stays small."""
    b = Bench()
    rng = np.random.default_rng(55)
    N = 600
    for K in ks:
        units = {8192: 1024 + 300}.get(K, 8192 + 300)
        host, _ = draw_rows(rng, N, K)
        pi = b.matrix(host)
        sizes, total = [], 0
        while total < units * UNIT:
            sz = int(rng.choice([1, 2, 5, 17, 63, 64, 65, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT + 3, 4 * UNIT + 7, 300, 599]))
            sizes.append(sz)
            total += sz
        off, mem = make_cover(rng, N, sizes)
        assert mem.size > units * UNIT
        for name, thr in (("0.05", 0.05), ("planted", float(PLANTED))):
            what = "persistent K=%d thr=%s" % (K, name)
            ref = reference(host, thr, off, mem)
            got = b.match(pi, thr, off, mem, dense=False)
            assert b.cv.last_kernel_name() == ("cover_fast" if K % 256 == 0 else "cover_generic")
            check(got, ref, what)
        print("persistent K=%d ok: %d communities, %d members" % (K, off.size - 1, mem.size), flush=True)
    print("persistent ok", flush=True)


def layout_group():
    """pi as one, two and eleven-plus-a-ragged-one blocks, members from every block; a misaligned block base, which
    takes the generic form at K = 256 and gives the same results"""
    b = Bench()
    rng = np.random.default_rng(52)
    n, K = 4700, 256
    host, _ = draw_rows(rng, n, K)
    off, mem = make_cover(rng, n, special_sizes(300, rng) + [4000])
    for name, thr in (("0.05", 0.05), ("planted", float(PLANTED)), ("0", 0.0)):
        ref = reference(host, thr, off, mem)
        for rib in (0, (n + 1) // 2, 400):
            pi = b.matrix(host, rib)
            assert len(pi.blocks) == {0: 1, (n + 1) // 2: 2, 400: 12}[rib]
            check(b.match(pi, thr, off, mem), ref, "rows_in_block=%d thr=%s" % (rib, name))
            assert b.cv.last_kernel_name() == "cover_fast"
        raw = b.misaligned(host)
        dsize = b.ctx.from_numpy(ref["detected_size"])
        check(b.match(raw, thr, off, mem, dsize=dsize), ref, "misaligned base thr=%s" % name)
        assert b.cv.last_kernel_name() == "cover_generic"
    print("layout ok", flush=True)


def forms_group():
    """every counting form the dispatcher can select is reached and reported; the finishing passes are in the source,
    in the table and (test_cover_host.py) in the library as gfx950 kernels, and a community that crosses a unit boundary
    can only be right if cover_finish ran"""
    import re
    b = Bench()
    rng = np.random.default_rng(54)
    for K, form in ((100, "generic"), (256, "fast"), (768, "fast"), (1024, "fast"), (1100, "generic"), (4352, "fast"),
                    (8192, "fast"), (8191, "generic")):
        host, _ = draw_rows(rng, 300, K)
        off, mem = make_cover(rng, 300, [UNIT - 5, 200, 3, 2 * UNIT + 1, 7])
        got = b.match(b.matrix(host), 0.05, off, mem)
        assert b.cv.last_kernel_name() == "cover_" + form, (K, b.cv.last_kernel_name())
        ref = reference(host, 0.05, off, mem)
        check(got, ref, "forms K=%d" % K)
        assert ref["truth_overlap"][1] > 0 and ref["truth_overlap"][3] > 0      # the crossing communities matched
    src = open(os.path.join(ps.ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_cover.hip")).read()
    in_source = set(re.findall(r'"(cover_[a-z0-9_]+)"', src))
    assert in_source == set(b.cv.KERNEL_FORMS), in_source ^ set(b.cv.KERNEL_FORMS)
    print("forms seen: %s" % " ".join(sorted(SEEN)), flush=True)
    assert SEEN == {"cover_fast", "cover_generic"} == in_source - {"cover_finish", "cover_unpack"}
    print("forms ok", flush=True)


def big_group():
    """K = 8192 and a little over 2^32 elements in one block (17 GB), zeroed and then filled on the device where the
    members touch it: members among the last rows, against numpy over those rows only; then the same rows in a block whose
    base is 4 bytes past a 16-byte boundary, which takes the generic form: the same outputs"""
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
    rng = np.random.default_rng(53)
    off, local = make_cover(rng, tail, [UNIT + 3, 40, 1, 0, 200, tail], spoil=False)
    local[5], local[UNIT + 10] = tail, tail                     # two members == the number of rows
    mem = (local.astype(np.int64) + (n - tail)).astype(np.uint32)
    ref = reference(host_tail, thr, off, local)
    assert ref["skipped"] == 2 and ref["detected_size"].sum() >= 40 * tail
    dsize = b.ctx.from_numpy(ref["detected_size"])              # (the other rows are zero: no members there)
    got = b.match(pi, thr, off, mem, dsize=dsize)
    assert b.cv.last_kernel_name() == "cover_fast"
    check(got, ref, "beyond 2^32 elements")
    del pi, blk
    b.release()
    mis, blk = b.zeroed(n, K, misaligned=True)
    blk[n - tail:].copy_(r)
    got2 = b.match(mis, thr, off, mem, dsize=dsize)
    assert b.cv.last_kernel_name() == "cover_generic"
    check(got2, ref, "beyond 2^32 elements, misaligned base")
    assert all(np.array_equal(got[name], got2[name]) for name in got)
    print("big ok: %d x %d" % (n, K), flush=True)


def constructed_group():
    """pi built from a planted cover: each node's row puts 1 / cnt on its planted communities, the columns permuted by
    a known permutation: the match is the permutation and every F1 is exactly 1; with one community's members halved,
    its F1 is the hand-computed fraction"""
    from mcmc_ammsb_gpu_amd import hostlib
    b = Bench()
    rng = np.random.default_rng(56)
    N, G = 3000, 24
    off, mem = hostlib.generate_cover(N, G, seed=17)
    perm = rng.permutation(G)
    K = G
    host = np.zeros((N, K), dtype=F32)
    for g in range(G):
        host[mem[int(off[g]):int(off[g + 1])], perm[g]] = 1
    host /= host.sum(1, keepdims=True)                          # 1, 1/2 or 1/3 on the planted communities
    pi = b.matrix(host)
    dsize = b.ro.sizes(pi, 0.05)
    tb, to, ts, db, do, sk, _ = b.api.match(pi, 0.05, off, mem, dsize)
    u = lambda x: x.cpu().numpy().view(np.uint32)   # noqa: E731
    m = b.cv.Match(0.05, tb.cpu().numpy(), u(to), u(ts), db.cpu().numpy(), u(do), dsize.cpu().numpy(), int(sk.item()))
    assert np.array_equal(m.truth_best, perm) and np.array_equal(m.detected_best, np.argsort(perm))
    assert np.array_equal(m.truth_overlap, m.truth_size) and np.array_equal(m.truth_size, np.diff(off.astype(np.int64)))
    assert m.f1_truth == 1.0 and m.f1_detected == 1.0 and m.avg_f1 == 1.0 and (m.f1_truth_each == 1.0).all()
    assert (m.jaccard_truth_each == 1.0).all() and m.skipped == 0
    # community 5 loses every second member: overlap = t' = ceil(t / 2) against d = t, F1 = 2 t' / (t' + t)
    lists = [mem[int(off[g]):int(off[g + 1])] for g in range(G)]
    t5 = lists[5].size
    lists[5] = lists[5][::2]
    h5 = lists[5].size
    o2, m2 = b.cv.check_cover(lists)
    tb, to, ts, db, do, sk, _ = b.api.match(pi, 0.05, o2, m2, dsize)
    m = b.cv.Match(0.05, tb.cpu().numpy(), u(to), u(ts), db.cpu().numpy(), u(do), dsize.cpu().numpy(), int(sk.item()))
    assert np.array_equal(m.truth_best, perm) and m.truth_overlap[5] == h5 == (t5 + 1) // 2 and m.truth_size[5] == h5
    assert m.f1_truth_each[5] == 2.0 * h5 / (h5 + t5) and m.f1_detected_each[perm[5]] == 2.0 * h5 / (h5 + t5)
    assert abs(m.f1_truth - (G - 1 + 2.0 * h5 / (h5 + t5)) / G) <= 1e-15
    check(dict(truth_best=m.truth_best, truth_overlap=m.truth_overlap, truth_size=m.truth_size, detected_best=m.detected_best,
               detected_overlap=m.detected_overlap, skipped=m.skipped), reference(host, 0.05, o2, m2), "halved", dense=False)
    print("constructed ok", flush=True)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _cover, hostlib
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    off, mem = hostlib.generate_cover(N, k_true, seed=20260101)
    lrn = make()
    lrn.Run(30)
    ck = io.BytesIO()
    lrn.Serialize(ck)
    host, _ = ps.pi_beta_of_checkpoint(ck.getvalue(), N, K)
    assert np.array_equal(host.view(np.uint32), lrn.pi.host().view(np.uint32))
    lists = [mem[int(off[g]):int(off[g + 1])].tolist() for g in range(k_true)]
    for thr in (0.05, 0.01, 0.0, 2.0):
        ref = reference(host, F32(thr), off, mem)
        for truth, dense in (((off, mem), True), (lists, False)):
            r = lrn.CompareCover(truth, thr, dense=dense)
            assert isinstance(r, _cover.Match)
            got = {k: getattr(r, k) for k in NAMES + ("skipped", "overlap")}
            check(got, ref, "learner thr=%g" % thr, dense=dense)
            assert (r.overlap is not None) == dense
            assert np.array_equal(r.detected_size, ref["detected_size"])
            assert np.array_equal(r.detected_size, lrn.CommunitySizes(thr).cpu().numpy())
            want = _cover.Match(thr, ref["truth_best"], ref["truth_overlap"], ref["truth_size"], ref["detected_best"],
                                ref["detected_overlap"], ref["detected_size"], 0)
            assert np.array_equal(r.f1_truth_each, want.f1_truth_each) and np.array_equal(r.f1_detected_each, want.f1_detected_each)
            assert (r.f1_truth, r.f1_detected, r.avg_f1) == (want.f1_truth, want.f1_detected, want.avg_f1)
        print("thr=%g: f1_truth %.4f f1_detected %.4f avg_f1 %.4f" % (thr, r.f1_truth, r.f1_detected, r.avg_f1), flush=True)
    # members the graph does not have are skipped; an empty cover is a valid call at every layer
    spoiled = np.concatenate([mem[:50], [N, NONE]]).astype(np.uint32)
    r = lrn.CompareCover((np.array([0, 20, 52], np.uint64), spoiled), 0.05)
    check({k: getattr(r, k) for k in NAMES + ("skipped",)}, reference(host, F32(0.05), np.array([0, 20, 52], np.uint64), spoiled),
          "learner: spoiled", dense=False)
    assert r.skipped == 2
    for none in ([], [[], []], (np.zeros(1, np.uint64), np.zeros(0, np.uint32))):
        r = lrn.CompareCover(none, 0.05)
        assert (r.detected_best == -1).all() and (r.truth_best == -1).all() and r.f1_truth == -1.0 and r.avg_f1 == -1.0
        assert np.array_equal(r.detected_size, lrn.CommunitySizes(0.05).cpu().numpy())
    ps.rejects(AmmsbError, (lambda: lrn.CompareCover(lists, -1.0), lambda: lrn.CompareCover(lists, float("nan")),
                            lambda: lrn.CompareCover((np.array([0, 9]), mem[:3]))))
    lrn.close()
    # Run(20), the calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.CompareCover((off, mem))
        a.CompareCover(lists, 0.01, dense=True)
    ps.unperturbed_run(make, calls, "cover match")
    print("learner ok graph=%s" % graph, flush=True)


def _check_match_file(path, ckpt, K, thr, offsets, members, what):
    """a cover-match file against the statement over the pi of the checkpoint the same process wrote; the Python writer
    reproduces its bytes"""
    from mcmc_ammsb_gpu_amd import _cover
    fN, m, _ = _cover.read_cover_match(path)
    assert m.detected_best.size == K and F32(m.threshold) == F32(thr), (m.detected_best.size, m.threshold)
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    ref = reference(pi, F32(thr), offsets, members)
    got = {n: getattr(m, n) for n in NAMES}
    got["skipped"] = m.skipped
    check(got, ref, what)
    assert np.array_equal(m.detected_size, ref["detected_size"]), what
    want = _cover.Match(thr, ref["truth_best"], ref["truth_overlap"], ref["truth_size"], ref["detected_best"],
                        ref["detected_overlap"], ref["detected_size"], ref["skipped"])
    again = path + ".py"
    _cover.write_cover_match(again, fN, want)
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the Python writer's bytes differ" % what
    return fN, m


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import _cover, hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("cover_test", d, 240)
        lists = [[int(w) for w in ln.split()[1:]] for ln in open(os.path.join(d, "truth.txt"))]
        offsets, members = _cover.check_cover(lists)
        fN, m = _check_match_file(os.path.join(d, "match.txt"), os.path.join(d, "cpp.ckpt"), 64, 0.05, offsets, members,
                                  "cover_test")
        assert fN == 20000 and m.truth_best.size == 18 and m.skipped == 2
        print("cpp ok: Learner::WriteCoverMatch equals the statement over the checkpoint's pi", flush=True)
        # the command-line driver on a data-set dump: the ground truth speaks of dense ids
        N = 6000
        f = os.path.join(d, "g.bin.gz")
        edges = hostlib.generate_graph(N, 8, 12, seed=3)
        hostlib.dump_dataset(f, N, 0.02, edges)
        toff, tmem = hostlib.generate_cover(N, 8, seed=3)
        truth, out, ck = os.path.join(d, "truth.cmty"), os.path.join(d, "m.txt"), os.path.join(d, "main.ckpt")
        _cover.write_cover(truth, toff, tmem)
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--ground-truth", truth, "--cover-match-out", out,
                "--checkpoint-out", ck]
        for extra, thr in (([], 0.05), (["--cover-match-threshold", "0.01"], 0.01)):
            r = ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + extra, 240)
            assert "8 communities, %d members, 0 ids the graph never mentions dropped" % tmem.size in r.stderr
            fN, m = _check_match_file(out, ck, 48, thr, toff, tmem, "ammsb_main dump thr=%g" % thr)
            assert fN == N and m.truth_best.size == 8 and m.skipped == 0
        # ... and on a text graph whose ids are not dense: the ground truth speaks of the file's ids, which the driver
        # maps through the loader's table; the ids the graph never mentions are dropped and counted
        name = lambda v: 7 * int(v) + 100     # noqa: E731
        txt = os.path.join(d, "g.txt")
        with open(txt, "w") as fh:
            fh.write("# a\n# b\n# c\n# d\n")
            for e in edges.tolist():
                fh.write("%d\t%d\n" % (name(e >> 32), name(e & 0xFFFFFFFF)))
        fN, _, ids = hostlib.load_snap_ids(txt)   # (the same table: the same insertions into the same container)
        dense_of = {int(v): i for i, v in enumerate(ids.tolist())}
        with open(truth, "w") as fh:
            fh.write("# planted cover, in the graph file's ids\n")
            for g in range(8):
                mem = [name(a) for a in tmem[int(toff[g]):int(toff[g + 1])]]
                fh.write(" ".join("%d" % a for a in mem + [3, 5][:g % 3]) + "\n")     # (3 and 5 are nobody's id)
        woff, wmem, dropped = _cover.read_cover(truth, dense_of)
        assert dropped > 0 and woff.size == 9
        r = ps.run_ammsb_main(["-f", txt] + tail, 240)
        assert "8 communities, %d members, %d ids the graph never mentions dropped" % (wmem.size, dropped) in r.stderr
        gN, m = _check_match_file(out, ck, 48, 0.05, woff, wmem, "ammsb_main text graph")
        assert gN == fN and m.truth_best.size == 8 and m.skipped == 0 and int(m.truth_size.sum()) == wmem.size
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(k) for k in a) or (1, 3, 64, 65, 100, 256, 260, 1024, 2048, 8192)),
    "persistent": lambda a: persistent_group(tuple(int(k) for k in a) or (64, 256, 1024, 8192)),
    "layout": lambda a: layout_group(),
    "forms": lambda a: forms_group(),
    "big": lambda a: big_group(),
    "constructed": lambda a: constructed_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
