"""ctypes view of libammsb_reduce.so (include/ammsb_reduce.h): the fitted model at fewer communities; and the plan that says
which: old community -> new community, or dropped.  A signature table of its own, like the other post-fit libraries."""
import ctypes as C

import numpy as np

from ._capi import PostfitLibrary, Rpm

MAX_COLS = 8192    # AMMSB_REDUCE_MAX_COLS
KERNEL_FORMS = ("reduce_select_v4", "reduce_select_s1", "reduce_merge_v4", "reduce_merge_s1", "reduce_theta")

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_reduce_rows": (C.c_int, [_P(Rpm), _vp, _vp, _vp, _u32, _u32, _P(Rpm), _vp, _vp, _u64, _u64, _vp]),
    "ammsb_reduce_theta": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    "ammsb_reduce_last_kernel_name": (C.c_char_p, []),
    "ammsb_reduce_last_error": (C.c_char_p, []),
}

_LIBRARY = PostfitLibrary("reduce", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def group_lanes(K):
    """lanes that own a row: the smallest power of two >= ceil(K / 4), at most 64"""
    g = 1
    while g < (int(K) + 3) // 4 and g < 64:
        g *= 2
    return g


class Plan:
    """map[K] int32: map[k] = j sends the old community k to the new community j in [0, new_K), -1 drops it.  Every new
    community has at least one source.  A Plan is never changed: merge(), drop() and drop_smaller() return another one, whose
    new communities are numbered by their smallest source (what compact() does to a map numbered any other way); the ids
    they take are OLD communities, so the pair lists of RelatedCommunities(...).duplicates(x) and
    LinkedCommunities(...).bridged(x) and the vector of CommunitySizes(thr) go in as they are.  A bad id or map raises
    ValueError and names it."""

    def __init__(self, map):
        m = np.asarray(map.cpu().numpy() if hasattr(map, "cpu") else map)
        K = m.size
        if m.ndim == 1 and not 1 <= K <= MAX_COLS:
            raise ValueError("a plan covers 1..%d communities, not %d" % (MAX_COLS, K))
        if m.ndim != 1 or m.dtype.kind not in "iu":
            raise ValueError("a plan is a 1-D integer map, not %s %s" % (m.dtype, m.shape))
        m = m.astype(np.int64)
        bad = np.flatnonzero((m < -1) | (m >= K))
        if bad.size:
            raise ValueError("community %d is sent to %d: outside -1..%d" % (bad[0], m[bad[0]], K - 1))
        if (m < 0).all():
            raise ValueError("the plan drops every community (community 0 included): nothing would be left")
        new_K = int(m.max()) + 1
        empty = np.flatnonzero(np.bincount(m[m >= 0], minlength=new_K) == 0)
        if empty.size:
            raise ValueError("new community %d has no source" % empty[0])
        self.map = m.astype(np.int32)
        self.map.setflags(write=False)

    # ------------------------------------------------------------------ what a plan says
    @property
    def K(self):
        return int(self.map.size)

    @property
    def new_K(self):
        return int(self.map.max()) + 1

    @property
    def drops(self):
        return bool((self.map < 0).any())

    @property
    def dropped(self):
        """the dropped old communities, ascending"""
        return np.flatnonzero(self.map < 0).astype(np.int32)

    @property
    def selects(self):
        """every new community has exactly one source: a permutation or a pruning"""
        return int((self.map >= 0).sum()) == self.new_K

    def csr(self):
        """-> (src_off [new_K + 1] uint32, src uint32): the sources of each new community, ascending"""
        kept = np.flatnonzero(self.map >= 0)
        order = kept[np.argsort(self.map[kept], kind="stable")]     # by new community, old ids ascending within one
        off = np.zeros(self.new_K + 1, np.uint32)
        off[1:] = np.cumsum(np.bincount(self.map[kept], minlength=self.new_K))
        return off, order.astype(np.uint32)

    def sources(self, j):
        if not 0 <= int(j) < self.new_K:
            raise ValueError("new community %d: the plan has 0..%d" % (j, self.new_K - 1))
        return np.flatnonzero(self.map == int(j)).astype(np.int32)

    def __eq__(self, other):
        return isinstance(other, Plan) and np.array_equal(self.map, other.map)

    def __repr__(self):
        return "Plan(K=%d, new_K=%d, dropped=%d)" % (self.K, self.new_K, self.dropped.size)

    # ------------------------------------------------------------------ building one
    @classmethod
    def identity(cls, K):
        return cls(np.arange(int(K), dtype=np.int32))

    def _ids(self, ids, what):
        ids = np.asarray(ids.cpu().numpy() if hasattr(ids, "cpu") else ids)
        if ids.size and ids.dtype.kind not in "iu":
            raise ValueError("%s: community ids are integers, not %s" % (what, ids.dtype))
        ids = ids.astype(np.int64).reshape(-1)
        bad = np.flatnonzero((ids < 0) | (ids >= self.K))
        if bad.size:
            raise ValueError("%s: community %d is outside 0..%d" % (what, ids[bad[0]], self.K - 1))
        return ids

    def compact(self):
        """the same groups, numbered by their smallest source"""
        m = self.map.astype(np.int64)
        kept = np.flatnonzero(m >= 0)
        first = np.full(self.new_K, self.K, np.int64)
        np.minimum.at(first, m[kept], kept)
        rank = np.empty(self.new_K, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(self.new_K)
        out = np.full(self.K, -1, np.int64)
        out[kept] = rank[m[kept]]
        return Plan(out)

    def merge(self, pairs):
        """A union-find over pairs (k, l) of old communities: everything a chain of pairs connects becomes one new
        community, together with whatever the plan had merged with either already.  A dropped community cannot be merged."""
        pairs = self._ids(np.asarray(pairs, dtype=np.int64).reshape(-1) if len(pairs) else np.zeros(0, np.int64), "merge")
        if pairs.size % 2:
            raise ValueError("merge: pairs of communities, not %d ids" % pairs.size)
        gone = pairs[self.map[pairs] < 0]
        if gone.size:
            raise ValueError("merge: community %d is dropped by this plan" % gone[0])
        parent = np.arange(self.new_K, dtype=np.int64)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for a, b in self.map[pairs].reshape(-1, 2):
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        root = np.array([find(j) for j in range(self.new_K)], np.int64)
        _, dense = np.unique(root, return_inverse=True)
        out = self.map.astype(np.int64)
        out[out >= 0] = dense.reshape(-1)[out[out >= 0]]
        return Plan(out).compact()

    def drop(self, ids):
        """drop the old communities `ids` (out of whatever they were merged into)"""
        ids = self._ids(ids, "drop")
        out = self.map.astype(np.int64)
        out[ids] = -1
        if (out < 0).all():
            raise ValueError("drop: community %d is the last one left" % ids[-1])
        _, dense = np.unique(out[out >= 0], return_inverse=True)
        out[out >= 0] = dense.reshape(-1)
        return Plan(out).compact()

    def drop_smaller(self, sizes, min_size):
        """sizes: [K] per old community (CommunitySizes(thr)).  Drops every new community whose sources' sizes add up to
        less than min_size: the sum is at least the size of the merged community (members of two sources count twice), so
        what goes is too small however its sources overlap."""
        sizes = np.asarray(sizes.cpu().numpy() if hasattr(sizes, "cpu") else sizes).reshape(-1)
        if sizes.size != self.K:
            raise ValueError("drop_smaller: %d sizes for %d communities" % (sizes.size, self.K))
        kept = np.flatnonzero(self.map >= 0)
        total = np.bincount(self.map[kept], weights=sizes[kept].astype(np.float64), minlength=self.new_K)
        small = total < float(min_size)
        if small.all():
            raise ValueError("drop_smaller: every community (community %d included) is smaller than %s" % (kept[0], min_size))
        return self.drop(kept[small[self.map[kept]]])


# ---------------------------------------------------------------------------------------------- the text file
def plan_text(plan):
    """`# K new_K dropped`, then `j n k0 k1 ...` per new community and `x k` per dropped one: byte for byte what
    mcmc::WritePlan writes"""
    lines = ["# %d %d %d" % (plan.K, plan.new_K, plan.dropped.size)]
    off, src = plan.csr()
    for j in range(plan.new_K):
        s = src[off[j]:off[j + 1]]
        lines.append("%d %d %s" % (j, s.size, " ".join(str(int(k)) for k in s)))
    lines += ["x %d" % k for k in plan.dropped]
    return "\n".join(lines) + "\n"


def write_plan(path, plan):
    with open(path, "w") as f:
        f.write(plan_text(plan))


def read_plan(path):
    """-> Plan; ValueError for a file that is not one (the line is named)"""
    with open(path) as f:
        lines = f.read().split("\n")
    head = lines[0].split()
    if len(head) != 4 or head[0] != "#":
        raise ValueError("%s: line 1 is not `# K new_K dropped`" % path)
    no = 1
    try:
        K, new_K, dropped = (int(x) for x in head[1:])
        if not 1 <= K <= MAX_COLS:
            raise ValueError
        m = np.full(K, -2, np.int64)
        seen_new, seen_drop = 0, 0
        for no, ln in enumerate(lines[1:], 2):
            w = ln.split()
            if not w:
                continue
            if w[0] == "x":
                ks, j = [int(w[1])], -1
                if len(w) != 2:
                    raise ValueError
                seen_drop += 1
            else:
                j, n, ks = int(w[0]), int(w[1]), [int(x) for x in w[2:]]
                if j != seen_new or n != len(ks) or n < 1:
                    raise ValueError
                seen_new += 1
            for k in ks:
                if not 0 <= k < K or m[k] != -2:
                    raise ValueError
                m[k] = j
        if seen_new != new_K or seen_drop != dropped or (m == -2).any():
            no = len(lines)
            raise ValueError
    except (ValueError, IndexError):
        raise ValueError("%s: line %d does not belong to a plan over the header's communities" % (path, no)) from None
    return Plan(m)
