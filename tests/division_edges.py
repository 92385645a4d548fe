"""Inputs that put update_phi and the beta gradient on BOTH sides of the exact-division branch (ammsb_dev.h "exact
division", the one home of the guards' bounds and of the quotients on either side; every kernel form calls them from
its own branch), a host statement of that branch's guards, and the coverage conditions the inputs must meet.

Plain numpy: imports without torch and without a GPU.  The oracle module (oracle_lib) is handed in where the reference's
own generators are needed (host_state); nothing here touches a device.

A *state* is any object with the host attributes of test_gpu_parity.Problem: N, K, n, nodes_h, nb_h, pi_h, phi_sum_h,
beta_h, edges.  The case builders edit it in place (before upload).  The oracle defines the result for any input, so
rows that are no valid model state (unnormalised pi rows, exact zeros) are used where a guard cannot be reached otherwise.

Granularity.  The kernels take the branch per LANE: a lane is fast for a row when beta is in range for the columns it
owns, phi_sum and its den = pi_a * phi_sum are in range (node level), its smallest |probs| is at least 2^-100 and the
row's probs_sum is in range.  Every form gives lane l the columns k = l (mod 8) (lane strides are 16, 32, 64, ...), so:
  * the beta limits are planted by column class k % 8 (BETA_BAD_CLASSES fail, the rest pass) and the beta guard is
    stated per class: the lanes of a failing class are slow in every row of the launch;
  * every other guard is stated per (node, row) over the columns of the beta-safe classes: a row is decided-FAST when
    no guard fails on any of them (every lane of a safe class divides by reciprocal), decided-SLOW when one fails
    (at least the lane that owns the failing column divides with `/`).
The per-element guards (beta, phi_sum, den, lo) are evaluated in float32 exactly as the kernels compute them, so values
exactly at a limit are decidable; probs_sum is a sum whose order differs by form, so it is evaluated in float64 and a
row within a factor 2 of 2^-30 or of 4 is UNDECIDED and counts for neither side.
"""
import numpy as np

F = np.float32
PROBS_LO = F(2.0 ** -100)
PSUM_LO, PSUM_HI = F(2.0 ** -30), F(4.0)
DEN_LO, DEN_HI = F(2.0 ** -110), F(2.0 ** 40)
PHISUM_LO, PHISUM_HI = F(2.0 ** -20), F(2.0 ** 40)
BETA_HI = F(1.0) - F(2.0 ** -20)
FLOOR = F(1e-24)     # the clamp floor of phi (what most of a trained model's memberships sit at)
DENORMAL = F(3e-39)

CASES = ("trained", "denormal", "beta_limits", "phi_sum_limits", "den_lo_limits", "psum_limits", "mixed")
GRAD_CASES = ("trained", "denormal", "mixed")
GUARDS = ("beta", "phi_sum", "den", "lo", "psum")
BETA_BAD_CLASSES = (5, 6, 7)  # k % 8 of the columns whose planted beta is outside [EPSILON, kBetaHi]
BETA_SLOTS = 64               # the slot count the gradient lists are laid out for (AMMSB_BETA_SLOTS)
MAX_EDGES = 512


class State:
    pass


def host_state(orc, N, K, n, n_nodes, seed=5, deg=16, link_frac=0.5):
    """The host half of test_gpu_parity.Problem, value for value (the GPU child asserts the equality)."""
    st = State()
    rng = np.random.default_rng(seed)
    st.rng, st.N, st.K, st.n = rng, N, K, n
    st.pi_h, st.phi_sum_h = orc.pi_init_gamma(N, K)
    st.theta_h = rng.gamma(1.0, 1.0, size=2 * K).astype(np.float32)
    st.beta_h = np.zeros_like(st.theta_h)
    orc.lib().orc_beta_from_theta(st.theta_h, st.beta_h, K)
    st.edges = orc.random_graph_edges(rng, N, deg * N)
    st.nodes_h = rng.permutation(N)[:n_nodes].astype(np.uint32) if n_nodes <= N else \
        rng.integers(0, N, size=n_nodes, dtype=np.uint32)
    nb = rng.integers(0, N, size=(n_nodes, n), dtype=np.uint32)
    order = np.argsort(st.edges >> np.uint64(32), kind="stable")
    src = (st.edges >> np.uint64(32)).astype(np.uint32)[order]
    dst = (st.edges & np.uint64(0xFFFFFFFF)).astype(np.uint32)[order]
    lo = np.searchsorted(src, st.nodes_h, "left")
    hi = np.searchsorted(src, st.nodes_h, "right")
    for i in range(min(n_nodes, 4096)):
        k = min(int(n * link_frac), hi[i] - lo[i])
        nb[i, :k] = dst[lo[i]:lo[i] + k]
    same = nb == st.nodes_h[:, None]
    nb[same] = (nb[same] + 1) % N
    st.nb_h = nb
    return st


class Saved:
    """the host arrays the builders edit, to put them back between cases"""
    FIELDS = ("pi_h", "phi_sum_h", "beta_h", "nb_h")

    def __init__(self, st):
        self.copy = {f: getattr(st, f).copy() for f in self.FIELDS}

    def restore(self, st):
        for f, v in self.copy.items():
            getattr(st, f)[...] = v


def adjacency(st):
    """(offsets, targets): every node's neighbours in the graph, both directions"""
    u = (st.edges >> np.uint64(32)).astype(np.int64)
    v = (st.edges & np.uint64(0xFFFFFFFF)).astype(np.int64)
    a, b = np.concatenate([u, v]), np.concatenate([v, u])
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    return np.searchsorted(a, np.arange(st.N + 1), "left"), b


def link_flags(st):
    """y of every (mini-batch node, neighbour row): membership in the training graph, as the kernels' set probe gives"""
    key = lambda a, b: (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    have = np.sort(st.edges)
    q = key(st.nodes_h[:, None].astype(np.uint64), st.nb_h.astype(np.uint64))
    pos = np.clip(np.searchsorted(have, q), 0, have.size - 1)
    return have[pos] == q


# ------------------------------------------------------------------------------------------------- case builders

def mix_rows(st, rng):
    """Every node's neighbour row anew, half of it graph neighbours (both directions, as far as the node has them), the
    rest random nodes.  Problem puts the links first, which would make every 4-row step homogeneous; a uniform shuffle
    would make nearly every one mixed.  So the aligned groups of four rows are, in turn (shifted from node to node): link /
    non-link / non-link / link, all links, the reverse, all non-links -- every 2-row and 4-row step meets all
    three kinds, and at least every other node both link and non-link rows.  No nb == node."""
    off, tgt = adjacency(st)
    N, n = st.N, st.n
    kinds = ((1, 0, 0, 1), (1, 1, 1, 1), (0, 1, 1, 0), (0, 0, 0, 0))
    for i, node in enumerate(st.nodes_h):
        row = rng.integers(0, N, size=n).astype(np.uint32)
        mine = rng.permutation(tgt[off[node]:off[node + 1]])
        want = np.array([kinds[(q // 4 + i) % 4][q % 4] for q in range(n)], dtype=bool)
        at = np.flatnonzero(want)[:mine.size]
        for _ in range(64):  # (the random entries are to be non-links: at small N a good share of all nodes are neighbours)
            bad = np.isin(row, mine) | (row == node)
            if not bad.any():
                break
            row[bad] = rng.integers(0, N, size=int(bad.sum()))
        row[at] = mine[:at.size]
        row[row == node] = (node + 1) % N
        st.nb_h[i] = row


def _floor_rows(st, rng, rows, frac, denormal=0.0):
    """phi of `rows` (node ids): a share frac at the 1e-24 floor (and a share `denormal` at 3e-39), renormalised as
    test_update_phi_extreme_values does"""
    rows = np.asarray(rows, dtype=np.int64)
    phi = st.pi_h[rows] * st.phi_sum_h[rows, None]
    phi[rng.random(phi.shape) < frac] = FLOOR
    if denormal:
        phi[rng.random(phi.shape) < denormal] = DENORMAL
    s = phi.sum(1, dtype=np.float32)
    st.phi_sum_h[rows] = s
    st.pi_h[rows] = phi / s[:, None]


def trained(st, rng, rows=None):
    _floor_rows(st, rng, np.arange(st.N) if rows is None else rows, 0.7)


def denormal(st, rng, rows=None):
    _floor_rows(st, rng, np.arange(st.N) if rows is None else rows, 0.7, 0.01)


def beta_limits(st, rng=None, eps=F(1e-7)):
    """beta_k by column class k % 8: 1 -> EPSILON, 3 -> kBetaHi (both pass, on the edge); 5 -> one ulp below EPSILON,
    6 -> one ulp above kBetaHi, 7 -> 1 - 6e-8 and 5e-8 in turn (all fail); 0, 2, 4 unchanged"""
    b = st.beta_h.reshape(-1, 2)
    k = np.arange(st.K)
    eps = F(eps)
    b[k % 8 == 1, 1] = eps
    b[k % 8 == 3, 1] = BETA_HI
    b[k % 8 == 5, 1] = np.nextafter(eps, F(0))
    b[k % 8 == 6, 1] = np.nextafter(BETA_HI, F(2))
    b[(k % 8 == 7) & (k // 8 % 2 == 0), 1] = F(1.0) - F(6e-8)
    b[(k % 8 == 7) & (k // 8 % 2 == 1), 1] = F(5e-8)
    b[:, 0] = F(1.0) - b[:, 1]


def _phi_sum_values(orig):
    lo, hi = PHISUM_LO, PHISUM_HI
    return [np.nextafter(lo, F(0)), lo, np.nextafter(hi, F(np.inf)), hi, F(orig * F(2.0 ** -45)), np.nextafter(lo, F(1)),
            F(orig * F(2.0 ** 33)), np.nextafter(hi, F(0)), F(orig * F(2.0 ** -40)), F(orig * F(1e-9)),
            F(orig * F(2.0 ** 34)), F(orig * F(1e9))]


def phi_sum_limits(st, rng=None, rows=None):
    """phi_sum of the nodes by turn: one ulp below 2^-20, 2^-20, one ulp above 2^40, 2^40, x 2^-45, one ulp above 2^-20,
    x 2^33, one ulp below 2^40, x 2^-40, x 1e-9 (fails up to K of about 950), x 2^34, x 1e9 (fails from K of about 1100):
    every other value fails whatever K is (phi_sum is about K; x 2^34 still leaves den = phi x 2^34 below 2^40, so phi_sum
    fails alone)"""
    rows = np.unique(st.nodes_h) if rows is None else np.asarray(rows)
    for j, r in enumerate(rows):
        st.phi_sum_h[r] = _phi_sum_values(st.phi_sum_h[r])[j % 12]


def den_lo_limits(st, rng=None, rows=None):
    """Planted powers of two in three columns of the node's own pi row (beta-safe classes 0, 2 and 4), by turn of ten:
       1: pi_a 2^-99, 3: 2^-100, 7: 2^-101 with phi_sum untouched -- den legal, lo = pi_a * tt straddles 2^-100;
       5: pi_a 2^-90, phi_sum 2^-20 -- den exactly 2^-110 (passes);  0, 2, 4, 6, 8, 9: pi_a 2^-91, phi_sum 2^-20 -- den
       2^-111 (fails alone: lo = 2^-91 * tt stays legal on the non-link rows)."""
    rows = np.unique(st.nodes_h) if rows is None else np.asarray(rows)
    cols = [c for c in (8, 18, 36) if c < st.K] or [0]
    for j, r in enumerate(rows):
        t = j % 10
        if t in (1, 3, 7):
            st.pi_h[r, cols] = F(2.0 ** -{1: 99, 3: 100, 7: 101}[t])
        else:
            st.pi_h[r, cols] = F(2.0 ** -(90 if t == 5 else 91))
            st.phi_sum_h[r] = F(2.0 ** -20)


def psum_limits(st, rng=None, rows=None):
    """By turn: 0: the node's pi row x 2^-35 (probs_sum below 2^-30) with phi_sum x 2^20; 1: the row x 2^4 (probs_sum of
    a non-link row above 4) with phi_sum x 2^-4; 2: untouched.  (phi_sum x 2^35 would leave den unchanged but takes
    phi_sum, about K at initialisation, past 2^40 -- another guard; x 2^20 keeps phi_sum and den legal up to K = 32768.)"""
    rows = np.unique(st.nodes_h) if rows is None else np.asarray(rows)
    for j, r in enumerate(rows):
        t = j % 3
        if t == 0:
            st.pi_h[r] *= F(2.0 ** -35)
            st.phi_sum_h[r] *= F(2.0 ** 20)
        elif t == 1:
            st.pi_h[r] *= F(16.0)
            st.phi_sum_h[r] *= F(2.0 ** -4)


MIXED_TURNS = ("trained", "phi_sum", "den_lo", "trained", "psum", "phi_sum", "den_lo", "denormal", "trained", "psum")


def mixed(st, rng, eps=F(1e-7)):
    """All of the above on disjoint subsets of the mini-batch nodes (by turn, MIXED_TURNS); every node outside the
    mini-batch is `trained`, so a trained node's link rows meet floor neighbours; the beta limits hold for the launch."""
    mb = st.nodes_h[np.sort(np.unique(st.nodes_h, return_index=True)[1])]  # (in mini-batch order, like mix_rows' kinds)
    turn = np.arange(mb.size) % len(MIXED_TURNS)
    pick = lambda name: mb[np.array([MIXED_TURNS[t] == name for t in turn], dtype=bool)]
    rest = np.setdiff1d(np.arange(st.N), mb)
    trained(st, rng, np.concatenate([rest, pick("trained")]))
    denormal(st, rng, pick("denormal"))
    phi_sum_limits(st, rows=pick("phi_sum"))
    den_lo_limits(st, rows=pick("den_lo"))
    psum_limits(st, rows=pick("psum"))
    beta_limits(st, eps=eps)


def apply_case(st, case, eps=F(1e-7), seed=17):
    """edits st for `case` (every builder also re-deals and shuffles the neighbour rows)"""
    rng = np.random.default_rng(seed)
    mix_rows(st, rng)
    if case == "trained":
        trained(st, rng)
    elif case == "denormal":
        denormal(st, rng)
    elif case == "beta_limits":
        beta_limits(st, eps=eps)
    elif case == "phi_sum_limits":
        phi_sum_limits(st)
    elif case == "den_lo_limits":
        den_lo_limits(st)
    elif case == "psum_limits":
        psum_limits(st)
    elif case == "mixed":
        mixed(st, rng, eps=eps)
    else:
        raise ValueError(case)
    assert not (st.nb_h == st.nodes_h[:, None]).any()


# ------------------------------------------------------------------------------------------------- the guards, on the host

def in_range(v, lo, hi):
    return (v >= lo) & (v <= hi)


def beta_ok(st, eps):
    b = st.beta_h.reshape(-1, 2)[:, 1]
    return in_range(b, F(eps), BETA_HI)


class PhiClasses:
    """per (node, row) unless noted; *_fail over the columns of the beta-safe classes, *_all over every column"""

    def tally(self):
        slow, fast = self.slow, self.fast
        total = slow.size
        return {"fast": fast.sum() / total, "slow": slow.sum() / total, "undecided": self.undecided.sum() / total}


def classify_phi(st, eps, links=None, keep_operands=False):
    eps = F(eps)
    links = link_flags(st) if links is None else links
    K = st.K
    bok = beta_ok(st, eps)
    cls_bad = np.array([not bok[c::8].all() for c in range(8)])
    safe = ~cls_bad[np.arange(K) % 8]  # columns of the classes whose every beta passes
    bf = st.beta_h.reshape(-1, 2)[:, 1] - eps
    m, n = st.nb_h.shape
    c = PhiClasses()
    c.beta_bad_classes = tuple(int(i) for i in np.flatnonzero(cls_bad))
    c.phi_sum_fail = np.zeros(m, bool)
    c.den_fail, c.den_fail_all = np.zeros(m, bool), np.zeros(m, bool)
    c.lo_fail, c.lo_fail_all = np.zeros((m, n), bool), np.zeros((m, n), bool)
    c.psum = np.zeros((m, n), np.int8)  # 0 passes, 1 fails, -1 undecided
    c.operands = [] if keep_operands else None
    e_link, e_non = eps, F(1.0) - eps
    for i, node in enumerate(st.nodes_h):
        phi_sum = st.phi_sum_h[node]
        pi_a = st.pi_h[node]
        den = pi_a * phi_sum
        dok = in_range(den, DEN_LO, DEN_HI)
        c.phi_sum_fail[i] = not in_range(phi_sum, PHISUM_LO, PHISUM_HI)
        c.den_fail[i], c.den_fail_all[i] = not dok[safe].all(), not dok.all()
        tt0 = st.pi_h[st.nb_h[i]] * bf[None, :]
        y = links[i][:, None]
        with np.errstate(all="ignore"):
            tt = np.where(y, tt0 + e_link, e_non - tt0).astype(np.float32)
            probs = pi_a[None, :] * tt
        small = np.abs(probs) < PROBS_LO
        c.lo_fail[i], c.lo_fail_all[i] = small[:, safe].any(1), small.any(1)
        ps = probs.astype(np.float64).sum(1)
        ok = (ps >= 2.0 * float(PSUM_LO)) & (ps <= 0.5 * float(PSUM_HI))
        bad = (ps < 0.5 * float(PSUM_LO)) | (ps > 2.0 * float(PSUM_HI)) | ~np.isfinite(ps)
        c.psum[i] = np.where(ok, 0, np.where(bad, 1, -1))
        if keep_operands:
            c.operands.append((probs, probs.sum(1, dtype=np.float32), den))
    node_fail = (c.phi_sum_fail | c.den_fail)[:, None]
    c.slow = node_fail | c.lo_fail | (c.psum == 1)
    c.fast = ~node_fail & ~c.lo_fail & (c.psum == 0)
    c.undecided = ~c.slow & ~c.fast
    # the only failing guard: of a node for the node-level guards (with a row whose own guards pass), of a row otherwise
    rows_ok = ~c.lo_fail & (c.psum == 0)
    c.sole = {
        "beta": int((~(c.phi_sum_fail | c.den_fail_all)[:, None] & ~c.lo_fail_all & (c.psum == 0)).sum()) if cls_bad.any() else 0,
        "phi_sum": int((c.phi_sum_fail & ~c.den_fail & rows_ok.any(1)).sum()),
        "den": int((c.den_fail & ~c.phi_sum_fail & rows_ok.any(1)).sum()),
        "lo": int((~node_fail & c.lo_fail & (c.psum == 0)).sum()),
        "psum": int((~node_fail & ~c.lo_fail & (c.psum == 1)).sum()),
    }
    return c


def group_kinds(c, U):
    """(all fast, all slow, mixed, all) counts over the aligned groups of U consecutive rows (complete groups, no undecided row)"""
    m, n = c.fast.shape
    g = n // U
    if g == 0:
        return 0, 0, 0, 0
    f = c.fast[:, :g * U].reshape(m, g, U)
    s = c.slow[:, :g * U].reshape(m, g, U)
    decided = (f | s).all(2)
    af, as_ = f.all(2) & decided, s.all(2) & decided
    return int(af.sum()), int(as_.sum()), int((decided & ~af & ~as_).sum()), m * g


def need(total, kinds):
    """"at least 8 times": 8 wherever the launch can hold 8 of each of its `kinds` kinds with as much again to spare
    (total >= 16 kinds); a smaller launch (6 nodes x 3 neighbours has 6 two-row steps in all) owes its share of a half"""
    return min(8, total // (2 * kinds))


def check_phi_coverage(case, c):
    """the coverage conditions of a classified update_phi input; returns the tally"""
    t = c.tally()
    what = (case, c.fast.shape, t)
    assert t["undecided"] <= 0.05, what
    if case in ("trained", "mixed"):
        assert t["fast"] >= 0.25 and t["slow"] >= 0.25, what
        for U in (2, 4):
            af, as_, mx, total = group_kinds(c, U)
            assert min(af, as_, mx) >= need(total, 3), (what, U, af, as_, mx, total)
    if case == "trained":
        both = (c.fast.any(1) & c.slow.any(1)).mean()
        assert both >= 0.25, (what, both)
    if case == "mixed":
        m, n = c.fast.shape
        for g in GUARDS:
            total = m  # (nodes: a guard's subset is a share of the nodes, whether it fails per node or per row)
            assert c.sole[g] >= need(total, len(GUARDS)), (what, g, c.sole)
    if case in ("beta_limits", "mixed"):
        assert c.beta_bad_classes == BETA_BAD_CLASSES, (what, c.beta_bad_classes)
    return t


# ------------------------------------------------------------------------------------------------- the gradient

def grad_probs(st, u, partners, links):
    """float32 probs[k] of every edge (u, partner) as CALC_PROBS forms them, and pi_a . pi_b"""
    b = st.beta_h.reshape(-1, 2)[:, 1]
    with np.errstate(all="ignore"):
        f = st.pi_h[u][None, :] * st.pi_h[partners]
        coef = np.where(np.asarray(links)[:, None], b[None, :], (F(1.0) - b)[None, :]).astype(np.float32)
        return coef * f, f


def classify_grads(st, eps, u, partners, links):
    """per edge: 1 fast (every non-zero |probs| >= 2^-100 and probs_sum decidedly in range), 0 slow, -1 undecided"""
    probs, f = grad_probs(st, u, partners, links)
    mag = np.abs(probs)
    lo_fail = ((mag < PROBS_LO) & (mag != 0)).any(1)  # (an exact zero divides exactly on either path)
    w = np.where(links, float(F(eps)), float(F(1.0) - F(eps)))
    ps = probs.astype(np.float64).sum(1) + w * (1.0 - f.astype(np.float64).sum(1))
    ok = (ps >= 2.0 * float(PSUM_LO)) & (ps <= 0.5 * float(PSUM_HI))
    bad = (ps < 0.5 * float(PSUM_LO)) | (ps > 2.0 * float(PSUM_HI)) | ~np.isfinite(ps)
    out = np.where(lo_fail | bad, 0, np.where(ok, 1, -1)).astype(np.int8)
    return out


PAIR_CLASSES = ("pair1_fast", "pair1_slow", "pair2_fast", "pair2_slow", "single_fast", "single_slow")


def pair_classes(links, fast, P=BETA_SLOTS):
    """the six step classes of an edge list under the one-wave form's greedy pairing: slot s walks edges s, s + P, ...;
    two consecutive edges with the same link flag (and the same u: all of them) go through pair_step (mode 2 links,
    mode 1 non-links), `fast` when both are; any other edge is stepped alone.  Undecided edges count for no class."""
    count = dict.fromkeys(PAIR_CLASSES, 0)
    E = len(links)
    for s in range(min(P, E)):
        idx = list(range(s, E, P))
        t = 0
        while t < len(idx):
            a = idx[t]
            if t + 1 < len(idx) and links[idx[t + 1]] == links[a]:
                b = idx[t + 1]
                if fast[a] >= 0 and fast[b] >= 0:
                    count["pair%d_%s" % (2 if links[a] else 1, "fast" if fast[a] and fast[b] else "slow")] += 1
                t += 2
            else:
                if fast[a] >= 0:
                    count["single_fast" if fast[a] else "single_slow"] += 1
                t += 1
    return count


def _plan(E, P):
    """(link, fast) wanted at every position.  Per slot: pair steps of the four pair kinds in turn (both fast; one fast
    and one slow, either way round), a lone last edge as a single step; where few slots end in a lone edge, every fifth pair gives way to two edges of different link flags -- two single steps."""
    want = [None] * E
    pairs = [(True, (True, True)), (False, (True, True)), (True, (True, False)), (False, (False, True)),
             (True, (True, True)), (False, (True, True)), (True, (False, True)), (False, (True, False))]
    np_, ns = 0, 0
    split = 2 * P - E < 24  # (fewer than 24 slots with a lone last edge)
    for s in range(min(P, E)):
        idx = list(range(s, E, P))
        t = 0
        while t < len(idx):
            if len(idx) - t >= 2 and not (split and (np_ + ns) % 5 == 4):
                y, fs = pairs[np_ % len(pairs)]
                np_ += 1
                want[idx[t]], want[idx[t + 1]] = (y, fs[0]), (y, fs[1])
                t += 2
            elif len(idx) - t >= 2:
                y = ns % 2 == 0
                want[idx[t]], want[idx[t + 1]] = (y, ns % 4 < 2), (not y, ns % 4 >= 2)
                ns += 1
                # (the second edge pairs with a third of its own flag, if the slot has one: give it the other flag)
                t += 2
                if t < len(idx):
                    want[idx[t]] = (y, True)
                    t += 1
            else:
                want[idx[t]] = (ns % 2 == 0, ns % 4 < 2)
                ns += 1
                t += 1
    return want


def grad_edges(st, rng, eps):
    """The node-strategy edge list of the current pi state: every edge has the end u, the node of largest degree; its
    links and as many non-links (at most MAX_EDGES in all), placed so that a slot of BETA_SLOTS meets link-link,
    non-link-non-link and mixed neighbours, fast and slow.  A trained state alone makes every edge slow (1e-48 in some
    column), an untrained one every edge fast, so to have both sides among the links AND the non-links whatever the
    state, the partners' pi rows are edited: three in five get exact zeros in the columns whose product would fall below
    2^-99 (fast: a zero numerator is exempt from the guard), the others get 1e-10 where u is at the floor (slow: 1e-34; floor times floor, 1e-48, is an exact
    zero in binary32 and would be exempt).
    Returns (u, partners, links)."""
    off, tgt = adjacency(st)
    u = int(np.argmax(np.diff(off)))
    mine = np.unique(tgt[off[u]:off[u + 1]])
    mine = mine[mine != u]
    others = np.setdiff1d(np.arange(st.N), np.concatenate([mine, [u]]))
    k = min(MAX_EDGES // 2, mine.size, others.size)  # its links and as many non-links
    mine = rng.permutation(mine)[:k]
    non = rng.choice(others, size=k, replace=False)
    b = st.beta_h.reshape(-1, 2)[:, 1]
    pa = st.pi_h[u]
    low = pa < F(1e-18)
    if low.mean() < 0.25:  # (u itself dense: give it floor columns so that a slow edge can exist)
        pa[np.arange(st.K) % 3 == 0] = FLOOR
        low = pa < F(1e-18)
    pools = {}
    for y, nodes in ((True, mine), (False, non)):
        nodes = rng.permutation(nodes)
        coef = b if y else F(1.0) - b
        for j, v in enumerate(nodes):
            row = st.pi_h[v]
            fast = j % 5 in (0, 1, 3)
            with np.errstate(all="ignore"):
                if fast:
                    row[~(np.abs(coef * (pa * row)) >= F(2.0) * PROBS_LO)] = F(0)
                    if not (row > 0).any():
                        row[np.argmax(pa)] = F(0.5)
                else:
                    row[low] = F(1e-10)
            pools.setdefault((y, fast), []).append(int(v))
    E = sum(len(v) for v in pools.values())
    partners, links = [], []
    for y, fast in _plan(E, BETA_SLOTS):
        for key in ((y, fast), (y, not fast), (not y, fast), (not y, not fast)):
            if pools.get(key):
                partners.append(pools[key].pop())
                links.append(key[0])
                break
    return u, np.array(partners, dtype=np.uint32), np.array(links, dtype=bool)


def check_grad_coverage(case, links, fast):
    count = pair_classes(links, fast)
    E = len(links)
    assert BETA_SLOTS < E <= MAX_EDGES, (case, E)
    assert (np.asarray(fast) < 0).mean() <= 0.05, (case, "undecided", fast)
    for k in PAIR_CLASSES:
        assert count[k] >= need(E, len(PAIR_CLASSES)), (case, E, count)
    return count
