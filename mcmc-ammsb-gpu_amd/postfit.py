"""The post-fit analyses of a Learner: what reads a fitted model out -- memberships and communities, link prediction,
link communities, community quality, the three comparisons with a ground-truth cover (F1 match, overlapping NMI, Omega
index), how the detected communities relate to each other, how they are linked, the overlapping modularity of the cover, the role of every node in it, the triangles inside the communities and the connected components of each.  Each drives one ops class over (pi, beta) as they stand: drained first, local on any rank (every rank
holds all of pi, so none is a collective), and nothing of the iteration is touched -- no RNG stream, no counter, no
buffer.  There is no CPU path: without a device every one of them raises."""
import numpy as np
import torch

from ._capi import AmmsbError


class PostFit:
    """Base class of Learner.  Uses its ops, ctx, cfg, params, dataset, pi, beta, the training / held-out sets and
    drain(), and nothing else of it."""

    def _postfit_op(self, attr, cls_name, what):
        """the ops object of one analysis, built on first use and kept; `what` names the analysis in the error"""
        if not torch.cuda.is_available():
            raise AmmsbError("no HIP device visible: %s has no CPU path" % what)
        if getattr(self, attr, None) is None:
            setattr(self, attr, getattr(self.ops, cls_name)(self.ctx))
        return getattr(self, attr)

    # ---- reading the model out (include/ammsb_readout.h)
    READOUT_SLAB_BYTES = 64 << 20  # most output bytes (ids + weights + count) one library call writes

    def _readout(self):
        return self._postfit_op("_community_readout", "CommunityReadout", "the read-out")

    def Memberships(self, top=4, threshold=0.0, nodes=None, sizes=None):
        """-> (ids [n, top] int32, weights [n, top] float32, count [n] int32), device tensors: per node (all of them, or
        the list `nodes`) its `top` strongest communities, value descending and equal values by community ascending;
        a slot below `threshold` (or past K) holds id -1 (0xFFFFFFFF) and weight 0; count = communities >= threshold,
        not capped at `top`.  sizes: a zeroed [K] int64 device tensor that receives the community sizes of the same
        pass."""
        from . import _readout
        top, threshold = _readout.check_args(top, threshold)
        ro, c = self._readout(), self.ctx
        self.drain()
        if nodes is not None and not torch.is_tensor(nodes):
            nodes = c.from_numpy(np.ascontiguousarray(nodes, dtype=np.uint32))
        n = self.cfg.N if nodes is None else int(nodes.numel())
        slab = max(1, self.READOUT_SLAB_BYTES // (8 * top + 4))
        if n <= slab:
            return ro.top(self.pi, top, threshold, nodes=nodes, sizes=sizes)
        ids, weights = c.empty((n, top), torch.int32), c.empty((n, top), torch.float32)
        count = c.empty((n,), torch.int32)
        for lo in range(0, n, slab):
            hi = min(lo + slab, n)
            i, w, k = ro.top(self.pi, top, threshold, nodes=None if nodes is None else nodes[lo:hi],
                             rows=(lo, hi) if nodes is None else None, sizes=sizes)
            ids[lo:hi], weights[lo:hi], count[lo:hi] = i, w, k
        return ids, weights, count

    def CommunitySizes(self, threshold):
        """-> [K] int64 device tensor: nodes with pi[a, k] >= threshold."""
        from . import _readout
        _, threshold = _readout.check_args(1, threshold)
        ro = self._readout()
        self.drain()
        return ro.sizes(self.pi, threshold)

    def Communities(self, top=4, threshold=0.0):
        """-> host CSR (offsets [K+1] int64, members int32): the members of each community in ascending node order.  A
        node is a member of the communities in its non-empty Memberships slots, so `top` caps memberships per node."""
        from . import _readout
        ids, _, _ = self.Memberships(top, threshold)
        return _readout.communities_csr(ids.cpu().numpy(), self.cfg.K)

    # ---- predicting links (include/ammsb_linkpred.h)
    LINKPRED_SLAB_BYTES = 64 << 20  # most output bytes (ids + scores) one library call writes

    def _linkpred(self):
        return self._postfit_op("_link_predictor", "LinkPredictor", "link prediction")

    def LinkProbabilities(self, edges):
        """-> [n] float32 device tensor: p(a, b) = eps + sum_k pi_ak pi_bk (beta_k - eps) per edge key (host array or
        device tensor of (a << 32) | b, either order of the ends); -1 for a pair with an end >= N."""
        lp = self._linkpred()
        self.drain()
        return lp.pairs(self.pi, self.beta, self.params.epsilon, edges)

    def PredictLinks(self, nodes, top=10, exclude=("training", "heldout")):
        """-> (ids [Q, top] int32, scores [Q, top] float32), device tensors: per node of `nodes` the `top` most probable
        partners among all N nodes that are not the node itself and whose pair is not in the excluded edge sets
        (`exclude`: any subset of "training", "heldout"); score descending, equal scores by id ascending; a slot past
        the eligible nodes holds id -1 and score 0."""
        from . import _linkpred
        top = _linkpred.check_top(top)
        names = _linkpred.check_exclude(exclude)
        lp = self._linkpred()
        self.drain()
        c = self.ctx
        sets = [{"training": self.trainingSet, "heldout": self.heldoutSet}[n] for n in names]
        if not torch.is_tensor(nodes):
            nodes = c.from_numpy(np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1))
        Q = int(nodes.numel())
        # The workspace does not grow with Q: the library aims at a fixed grid, so a call holds about 2048 x 128 partial
        # lists whatever Q is (2 MiB x top).  What grows is the output, and that is what a slab bounds (whole tiles of
        # 128 queries).
        slab = max(128, self.LINKPRED_SLAB_BYTES // (8 * top) // 128 * 128)
        if Q <= slab:
            return lp.top(self.pi, self.beta, self.params.epsilon, nodes, top, exclude=sets)
        ids, scores = c.empty((Q, top), torch.int32), c.empty((Q, top), torch.float32)
        for lo in range(0, Q, slab):
            hi = min(lo + slab, Q)
            ids[lo:hi], scores[lo:hi] = lp.top(self.pi, self.beta, self.params.epsilon, nodes[lo:hi].contiguous(),
                                               top, exclude=sets)
        return ids, scores

    def HeldoutAUC(self):
        """Area under the ROC curve of LinkProbabilities over the held-out list; label = membership in the held-out
        set, as the perplexity pass decides is_edge.  Rank statistic with average ranks for ties, float64 on the host
        (_linkpred.auc); raises when the list lacks links or non-links."""
        from . import _linkpred
        self._linkpred()
        scores = self.LinkProbabilities(self.heldoutEdges)
        labels = self.heldoutSet.Has(self.heldoutEdges)
        return _linkpred.auc(scores.cpu().numpy(), labels.cpu().numpy() != 0)

    # ---- the communities that explain a link (include/ammsb_linkcomm.h)
    LINKCOMM_SLAB_BYTES = 64 << 20  # most output bytes (ids + terms + prob) one library call writes

    def _linkcomm(self):
        return self._postfit_op("_link_communities", "LinkCommunities", "the link-community read-out")

    def TrainingLinks(self):
        """-> [E] uint64 (as int64) device tensor: every training link once as (min << 32) | max, ascending.  Built
        from the data set's training adjacency on first use and kept."""
        lc = self._linkcomm()
        if getattr(self, "_training_links", None) is None:
            off, tgt = self.dataset.training_csr()
            src = np.repeat(np.arange(self.cfg.N, dtype=np.uint64), np.diff(off.astype(np.int64)))
            tgt = tgt[:src.size].astype(np.uint64)
            keep = src < tgt                      # each link sits in both ends' rows: take it from the lower end
            keys = np.sort((src[keep] << np.uint64(32)) | tgt[keep])
            self._training_links = lc.ctx.from_numpy(keys)
        return self._training_links

    def _linkcomm_edges(self, edges):
        if edges is None:
            return self.TrainingLinks()
        if not torch.is_tensor(edges):
            edges = self.ctx.from_numpy(np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1))
        return edges

    def LinkCommunities(self, edges=None, top=1, min_term=0.0):
        """-> (ids [n, top] int32, share [n, top] float32, prob [n] float32), device tensors: per edge key of `edges`
        (host array or device tensor of (a << 32) | b, either order of the ends; default: TrainingLinks()) the `top`
        communities with the largest terms t_k = (pi_ak pi_bk) beta_k that are > 0 and >= min_term, term descending and
        equal terms by community ascending, and the link's probability p.  share = t_k / p, the posterior that the link
        is a community-k link: ONE torch division of the kernel's exact terms by its p (so it carries p's rounding),
        and +0 in an empty slot, whose id is -1 (0xFFFFFFFF); a filled slot has p >= its term > 0.  An edge with an end
        >= N has empty slots and p = -1.  An empty list gives empty tensors."""
        from . import _linkcomm
        top, min_term = _linkcomm.check_args(top, min_term)
        lc = self._linkcomm()
        self.drain()
        edges = self._linkcomm_edges(edges)
        c, n, eps = self.ctx, int(edges.numel()), self.params.epsilon
        slab = max(1, self.LINKCOMM_SLAB_BYTES // (8 * top + 4))
        if n <= slab:
            ids, terms, prob = lc.edges(self.pi, self.beta, eps, edges, top, min_term)
        else:
            ids, terms = c.empty((n, top), torch.int32), c.empty((n, top), torch.float32)
            prob = c.empty((n,), torch.float32)
            for lo in range(0, n, slab):
                hi = min(lo + slab, n)
                ids[lo:hi], terms[lo:hi], prob[lo:hi] = lc.edges(self.pi, self.beta, eps, edges[lo:hi], top, min_term)
        share = torch.where(ids < 0, torch.zeros((), dtype=torch.float32, device=terms.device), terms / prob.unsqueeze(1))
        return ids, share, prob

    def LinkCommunitySizes(self, min_term=0.0, edges=None):
        """-> [K + 1] int64 device tensor: per community the links (default: the training links) whose largest term it
        holds; entry K counts the links no community explains at min_term."""
        from . import _linkcomm
        _, min_term = _linkcomm.check_args(1, min_term)
        lc = self._linkcomm()
        self.drain()
        return lc.sizes(self.pi, self.beta, self.params.epsilon, self._linkcomm_edges(edges), min_term)

    # ---- scoring communities against the graph (include/ammsb_quality.h)
    def _quality(self):
        return self._postfit_op("_community_quality", "CommunityQuality", "the community-quality read-out")

    def CommunityQuality(self, threshold=0.05, edges=None):
        """-> _quality.Quality: per community its size (CommunitySizes(threshold)), the links of `edges` (host array or
        device tensor of (a << 32) | b, either order of the ends; default: TrainingLinks()) with both ends in it
        (internal) and with exactly one end in it (boundary), membership being pi[a, k] >= threshold; the links no
        community covers (uncovered), the keys with an end >= N (skipped), links = the others; and, in float64 on the
        host, conductance and density per community and the coverage of the cover (-1 where undefined).  Counts are
        exact."""
        from . import _quality
        threshold = _quality.check_threshold(threshold)
        cq = self._quality()
        self.drain()
        edges = self._linkcomm_edges(edges)
        N, K = self.cfg.N, self.cfg.K
        counts = cq.edges(cq.mask(self.pi, threshold), N, K, edges).cpu().numpy()
        size = self._readout().sizes(self.pi, threshold).cpu().numpy()
        skipped = int(counts[2 * K + 1])
        return _quality.Quality(threshold, size, counts[:K], counts[K:2 * K], int(edges.numel()) - skipped,
                                int(counts[2 * K]), skipped)

    def SharedCommunities(self, edges=None, threshold=0.05):
        """-> [n] int32 device tensor: per edge key the number of communities that hold both its ends (pi >= threshold
        at both), -1 for a key with an end >= N.  An empty list gives an empty tensor."""
        from . import _quality
        threshold = _quality.check_threshold(threshold)
        cq = self._quality()
        self.drain()
        edges = self._linkcomm_edges(edges)
        _, shared = cq.edges(cq.mask(self.pi, threshold), self.cfg.N, self.cfg.K, edges, shared=True, counts=False)
        return shared

    # ---- comparing with a ground-truth cover (include/ammsb_cover.h)
    def _cover(self):
        return self._postfit_op("_cover_match", "CoverMatch", "the cover match")

    def CompareCover(self, truth, threshold=0.05, dense=False):
        """-> _cover.Match: the detected cover D_k = {a : pi[a, k] >= threshold} against the ground-truth cover `truth`,
        (offsets [G + 1], members [M]) host arrays or a list of id lists (taken as written: a duplicate counts twice; a
        member >= N reads nothing and is counted in .skipped).  Per ground-truth community the detected community of the
        best F1 = 2 overlap / (t_g + d_k) among those it overlaps (equal F1 -> the lower k, none -> -1), with the overlap
        and t_g; the same per detected community over the ground-truth ones; d_k = CommunitySizes(threshold) counts all
        N nodes, also those no ground-truth community holds.  In float64 on the host: the F1 of every best match and
        f1_truth, f1_detected, avg_f1 (-1 where a mean is over nothing).  dense=True also returns overlap [G, K].  The
        integers are exact."""
        from . import _cover
        threshold = _cover.check_threshold(threshold)
        offsets, members = _cover.check_cover(truth)
        cm = self._cover()
        self.drain()
        size = self._readout().sizes(self.pi, threshold)
        tb, to, ts, db, do, sk, ov = cm.match(self.pi, threshold, offsets, members, size, dense)
        u32 = lambda x: x.cpu().numpy().view(np.uint32)   # noqa: E731
        return _cover.Match(threshold, tb.cpu().numpy(), u32(to), u32(ts), db.cpu().numpy(), u32(do),
                            size.cpu().numpy(), int(sk.item()), None if ov is None else u32(ov))

    # ---- the overlapping NMI against a ground-truth cover (include/ammsb_nmi.h)
    def _nmi(self):
        return self._postfit_op("_cover_nmi", "CoverNMI", "the cover NMI")

    def CoverNMI(self, truth, threshold=0.05, slab_bytes=256 << 20):
        """-> _nmi.NMI: the overlapping NMI of the detected cover D_k = {a : pi[a, k] >= threshold} against the
        ground-truth cover `truth`, in the forms CompareCover takes (a member >= N reads nothing and is counted in
        .skipped; a node listed twice inside one community is a ValueError: NMI is defined on sets).  The dense overlap
        is made slab by slab, Gs communities with Gs K 4 <= slab_bytes (Gs >= 1), by the cover match, and folded on the
        device into H(X_g | Y) and H(Y_k | X); every float comes from the device.  On the host, in float64: nmi_lfk
        (Lancichinetti, Fortunato, Kertesz) and nmi_max (McDaid, Greene, Hurley), -1 where undefined.  The results do
        not depend on slab_bytes."""
        from . import _cover, _nmi
        threshold = _cover.check_threshold(threshold)
        offsets, members = _cover.check_cover(truth)
        _nmi.check_sets(offsets, members)
        nm, cm = self._nmi(), self._cover()
        self.drain()
        N, K, G = self.cfg.N, self.cfg.K, offsets.size - 1
        size = self._readout().sizes(self.pi, threshold)
        off = offsets.astype(np.int64)
        valid = np.concatenate([[0], np.cumsum(members < N, dtype=np.int64)])
        tsize = (valid[off[1:]] - valid[off[:-1]]).astype(np.uint32)     # t_g: the members < N
        st = nm.begin(N, tsize, size)
        rows = max(1, int(slab_bytes) // (4 * K))
        for g0 in range(0, G, rows):
            g1 = min(g0 + rows, G)
            ov = cm.match(self.pi, threshold, (off[g0:g1 + 1] - off[g0]).astype(np.uint64),
                          members[off[g0]:off[g1]], size, dense=True)[6]
            nm.accumulate(st, ov, g0)
        return _nmi.NMI(threshold, tsize, size.cpu().numpy(), members.size - int(valid[-1]), st.H_truth.cpu().numpy(),
                        st.c_truth.cpu().numpy(), st.H_detected.cpu().numpy(), st.c_detected.cpu().numpy())

    # ---- the Omega index against a ground-truth cover (include/ammsb_omega.h)
    def _omega(self):
        return self._postfit_op("_cover_omega", "CoverOmega", "the cover Omega index")

    def CoverOmega(self, truth, threshold=0.05, universe="covered", launch_pairs=1 << 31, max_bytes=4 << 30):
        """-> _omega.Omega: the Omega index (Collins & Dent) of the detected cover D(a) = {k : pi[a, k] >= threshold}
        against the ground-truth cover `truth`, in the forms CompareCover takes, over the pairs of a universe of nodes:
        "all", "covered" (the nodes with at least one valid ground-truth membership) or an ascending array of distinct
        ids < N.  A member >= N is counted in .skipped, a valid member outside the universe in .outside; a node listed
        twice inside one community is a ValueError.  Per level j the pairs that share j communities in both covers
        alike (.agree), in the detected cover (.detected) and in the ground truth (.truth), counted on the device, at
        most launch_pairs pairs per launch; the score in exact integers on the host (.omega, NaN where undefined).  The
        two bit matrices, n (ceil(K / 32) + ceil(G / 32)) 4 bytes, must fit max_bytes.  The results do not depend on
        launch_pairs."""
        from . import _cover, _omega
        threshold = _cover.check_threshold(threshold)
        offsets, members = _cover.check_cover(truth)
        _omega.check_sets(offsets, members)
        N, K, G = self.cfg.N, self.cfg.K, offsets.size - 1
        U = _omega.check_universe(universe, N, members)
        n = int(U.size)
        if G > _omega.MAX_TRUTH:
            raise AmmsbError("cover omega: %d ground-truth communities; the bit rows hold at most %d" % (G, _omega.MAX_TRUTH))
        need = n * ((K + 31) // 32 + (G + 31) // 32) * 4
        if need > int(max_bytes):
            raise AmmsbError("cover omega: the bit rows of %d nodes take %d bytes, more than max_bytes = %d; "
                             "universe=\"covered\" keeps only the nodes the ground truth holds" % (n, need, int(max_bytes)))
        if int(launch_pairs) < 1:
            raise AmmsbError("cover omega: launch_pairs must be at least 1")
        om = self._omega()
        self.drain()
        c = self.ctx
        position = np.full(N, -1, dtype=np.int32)
        position[U] = np.arange(n, dtype=np.int32)
        nodes = c.from_numpy(U) if n else None
        dbits, dcount = om.detected_bits(self.pi, threshold, nodes=nodes, n=n)
        tbits, tcount, tally = om.truth_bits(c.from_numpy(offsets), c.from_numpy(members), N, c.from_numpy(position), n)
        L = 1 + (max(int(dcount.max().item()), int(tcount.max().item())) if n else 0)
        if L > _omega.MAX_LEVELS:
            raise AmmsbError("cover omega: a node of the universe is in %d communities; the pair pass counts up to %d"
                             % (L - 1, _omega.MAX_LEVELS - 1))
        hist = c.zeros((3 * L + 1,), torch.int64)
        total = _omega.tiles(n)
        step = min(_omega.MAX_LAUNCH_TILES, max(1, int(launch_pairs) // (_omega.TILE * _omega.TILE)))
        for t0 in range(0, total, step):
            om.pairs(dbits, K, tbits, G, n, L, hist, t0, min(step, total - t0))
        h, tally = hist.cpu().numpy(), tally.cpu().numpy()
        if n == 0:   # (nothing walked the CSR: every member is skipped or outside, as mcmc::Learner::CoverOmega counts)
            tally = np.array([int((members >= N).sum()), int((members < N).sum())], dtype=np.int64)
        if int(h[3 * L]):
            raise AmmsbError("cover omega: %d pairs at or past level %d, which no node reaches" % (int(h[3 * L]), L))
        return _omega.Omega(threshold, n, h[:L], h[L:2 * L], h[2 * L:3 * L], int(tally[0]), int(tally[1]), K, G)

    # ---- how the detected communities relate to each other (include/ammsb_relate.h)
    def _relate(self):
        return self._postfit_op("_community_relations", "CommunityRelations", "the community relations")

    def CommunityOverlap(self, threshold=0.05, max_bytes=1 << 30):
        """-> [K, K] int32 device tensor that holds uint32 bits (view it as uint32 on the host): overlap[k, l] = the nodes
        a with pi[a, k] >= threshold and pi[a, l] >= threshold; symmetric, the diagonal is CommunitySizes(threshold).  The
        nodes are cut into slabs of a multiple of 64 rows whose membership bits, K rows / 8 bytes, fit max_bytes (at
        least 64 rows).  Integer adds: exact, and the result does not depend on max_bytes."""
        from . import _relate
        threshold = _relate.check_threshold(threshold)
        if int(max_bytes) < 1:
            raise AmmsbError("community relations: max_bytes must be at least 1")
        N, K = self.cfg.N, self.cfg.K
        step = _relate.slab_rows(K, max_bytes)
        cr = self._relate()
        self.drain()
        overlap = self.ctx.zeros((K, K), torch.int32)
        for lo in range(0, N, step):
            hi = min(lo + step, N)
            cr.pairs(cr.bits(self.pi, threshold, rows=(lo, hi)), K, hi - lo, overlap)
        return overlap

    def RelatedCommunities(self, threshold=0.05, top=4, by="jaccard", min_overlap=1, max_bytes=1 << 30, dense=False):
        """-> _relate.Related: per community k the `top` other communities l that share at least max(1, min_overlap)
        nodes with it, ranked by `by` -- "overlap" (the shared nodes o), "jaccard" (o / (d_k + d_l - o)) or "contained"
        (o / d_l, the share of l inside k) -- as exact rationals, equal values by id ascending: .size, .partner (-1 in
        an empty slot), .overlap, and in float64 on the host .jaccard, .inside and .contained; .matrix (the whole
        CommunityOverlap, on the host) with dense=True; .duplicates() and .nested() list the pairs that reach a bound.
        The integers are exact and do not depend on max_bytes."""
        from . import _relate
        threshold = _relate.check_threshold(threshold)
        _, top, min_overlap = _relate.check_args(by, top, min_overlap)
        overlap = self.CommunityOverlap(threshold, max_bytes)
        partner, shared = self._relate().top(overlap, by, top, min_overlap)
        matrix = overlap.cpu().numpy().view(np.uint32)
        return _relate.Related(threshold, by, min_overlap, np.diagonal(matrix).astype(np.int64), partner.cpu().numpy(),
                               shared.cpu().numpy().view(np.uint32), matrix if dense else None, N=self.cfg.N)

    # ---- how the detected communities are linked to each other (include/ammsb_connect.h)
    def _connect(self):
        return self._postfit_op("_community_links_op", "CommunityLinks", "the community links")

    def _community_links(self, threshold, edges):
        """-> (links [K, K] int64, counts [2] int64) on the device"""
        cl = self._connect()
        self.drain()
        edges = self._linkcomm_edges(edges)
        N, K = self.cfg.N, self.cfg.K
        directed, counts = cl.edges(cl.mask(self.pi, threshold), N, K, edges)
        return cl.finish(directed), counts

    def CommunityLinks(self, threshold=0.05, edges=None):
        """-> [K, K] int64 device tensor: links[k, l] = directed[k, l] + directed[l, k], directed[k, l] being the keys
        (a << 32) | b of `edges` (host array or device tensor, either order of the ends, duplicates and a == b as
        written, a key with an end >= N left out; default: TrainingLinks()) with pi[a, k] >= threshold and pi[b, l] >=
        threshold.  Symmetric; the diagonal is twice CommunityQuality's internal.  Integer adds: exact."""
        from . import _connect
        threshold = _connect.check_threshold(threshold)
        return self._community_links(threshold, edges)[0]

    def LinkedCommunities(self, threshold=0.05, top=4, by="density", min_links=1, edges=None, max_bytes=1 << 30, dense=False):
        """-> _connect.Linked: per community k the `top` other communities l with at least max(1, min_links) links of
        `edges` (as CommunityLinks takes them) between them, ranked by `by` -- "links" (the count w) or "density" (w over
        the d_k d_l - overlap[k, l] ordered pairs of distinct nodes, overlap from CommunityOverlap(threshold, max_bytes);
        a pair of communities without such a node pair is no partner) -- as exact rationals, equal values by id
        ascending: .size, .internal, .partner (-1 in an empty slot), .links, .shared, .valid, .skipped, and in float64 on
        the host .density and .within; .matrix (the whole CommunityLinks, on the host) with dense=True; .bridged() lists
        the pairs linked as densely as one of them is inside.  The integers are exact."""
        from . import _connect
        threshold = _connect.check_threshold(threshold)
        _, top, min_links = _connect.check_args(by, top, min_links)
        overlap = self.CommunityOverlap(threshold, max_bytes)
        links, counts = self._community_links(threshold, edges)
        partner, plinks, pshared = self._connect().top(links, overlap, by, top, min_links)
        matrix = links.cpu().numpy().view(np.uint64)
        size = np.diagonal(overlap.cpu().numpy().view(np.uint32)).astype(np.int64)
        valid, skipped = (int(v) for v in counts.cpu().numpy())
        return _connect.Linked(threshold, by, min_links, size, (np.diagonal(matrix) // np.uint64(2)).astype(np.int64),
                               partner.cpu().numpy(), plinks.cpu().numpy().view(np.uint64),
                               pshared.cpu().numpy().view(np.uint32), valid, skipped, matrix if dense else None, N=self.cfg.N)

    # ---- is the cover better than chance? (include/ammsb_modularity.h)
    def _modularity(self):
        return self._postfit_op("_modularity_op", "Modularity", "the modularity")

    def Modularity(self, threshold=0.05, edges=None, degree=False):
        """-> _modularity.Modularity: the overlapping modularity (EQ of Shen et al.) of the cover pi[a, k] >= threshold
        against `edges` (host array or device tensor of (a << 32) | b, either order of the ends, duplicates and a == b as
        written, a key with an end >= N left out; default: TrainingLinks()), fewer than 2^31 keys: .q and .q_each [K] in
        float64, derived on the host from .internal and .volume, the device's 128-bit sums of floor(2^62 / (O_a O_b)) over
        the links inside k and of deg[a] floor(2^62 / O_a) over the members of k, as Python ints; .in_each, .s_each,
        .links, .skipped, and .degree [N] uint32 with degree=True.  The integers are exact and the same from run to
        run."""
        from . import _modularity
        threshold = _modularity.check_threshold(threshold)
        md = self._modularity()
        self.drain()
        edges = self._linkcomm_edges(edges)
        _modularity.check_keys(edges.numel())
        internal, volume, counts, deg = md.run(self.pi, threshold, edges)
        valid, skipped = (int(v) for v in counts.cpu().numpy())
        return _modularity.Modularity(threshold, _modularity.wide(internal.cpu().numpy()), _modularity.wide(volume.cpu().numpy()),
                                      valid, skipped, deg.cpu().numpy().view(np.uint32) if degree else None, N=self.cfg.N)

    # ---- how does a single node sit in the cover? (include/ammsb_roles.h)
    def _roles(self):
        return self._postfit_op("_roles_op", "NodeRoles", "the node roles")

    def _training_adjacency(self):
        """-> (offsets [N + 1] int64, targets int32) device tensors: the data set's training adjacency, uploaded on first
        use and kept"""
        from . import _roles
        if getattr(self, "_training_csr_dev", None) is None:
            off, tgt = self.dataset.training_csr()
            _roles.check_rows(np.diff(off.astype(np.int64)).max() if off.size > 1 else 0)
            self._training_csr_dev = (self.ctx.from_numpy(off), self.ctx.from_numpy(tgt))
        return self._training_csr_dev

    def _symmetric_csr(self, edges):
        """keys (a << 32) | b -> (offsets, targets, keys with an end >= N): each valid key puts b in a's row and a in b's
        row (a key a == a puts a twice in a's row), in the order of the list, built on the device"""
        from . import _roles
        N = self.cfg.N
        keys = self._linkcomm_edges(edges)
        if keys.dtype != torch.int64 or keys.dim() != 1:
            raise AmmsbError("node roles: edges must be 1-d uint64 keys (a << 32) | b")
        a, b = (keys >> 32) & 0xFFFFFFFF, keys & 0xFFFFFFFF
        ok = (a < N) & (b < N)
        a, b = a[ok], b[ok]
        src, dst = torch.cat((a, b)), torch.cat((b, a))
        order = torch.sort(src, stable=True).indices
        rows = torch.bincount(src, minlength=N)
        _roles.check_rows(int(rows.max()) if N else 0)
        offsets = torch.zeros(N + 1, dtype=torch.int64, device=keys.device)
        offsets[1:] = torch.cumsum(rows, 0)
        return offsets, dst[order].to(torch.int32).contiguous(), int(keys.numel() - a.numel())

    def NodeRoles(self, threshold=0.05, edges=None, nodes=None, top=4, among="all", min_count=0):
        """-> _roles.Roles: how every node (or the range nodes=(first, count)) sits in the cover pi[a, k] >= threshold
        against an adjacency: the training adjacency of the data set (edges=None), or the symmetric one of `edges` (host
        array or device tensor of (a << 32) | b; duplicates and a == b as written, a key with an end >= N counted in
        .skipped).  With c[a, k] the neighbours of a in k: .degree, .own, .embedded, .reached, .votes, .squares per node,
        .home / .hcount / .hflags the `top` (1..16) communities with the largest c (among="all": every k with c >= max(1,
        min_count); among="own": a's own communities with c >= min_count), .ksum / .ksq / .kmembers per community, all exact
        integers; .embeddedness, .participation and .z in float64 on the host; .hubs(), .connectors(), .misplaced().  A row
        of more than 2^25 targets is refused."""
        from . import _roles
        threshold, top = _roles.check_threshold(threshold), _roles.check_top(top)
        _roles.check_among(among)
        min_count = _roles.check_min_count(min_count)
        first, count = _roles.check_nodes(nodes, self.cfg.N)
        op = self._roles()
        self.drain()
        if edges is None:
            (offsets, targets), lost = self._training_adjacency(), 0
        else:
            offsets, targets, lost = self._symmetric_csr(edges)
        st = op.run(self.pi, threshold, offsets, targets, first=first, count=count, among=among, top=top, min_count=min_count)
        part = lambda name, dt: st[name][first:first + count].cpu().numpy().view(dt)   # noqa: E731
        whole = lambda name: st[name].cpu().numpy().view(np.uint64)                    # noqa: E731
        valid, skipped = (int(v) for v in st["counts"].cpu().numpy())
        return _roles.Roles(threshold, among, top, min_count, part("degree", np.uint32), part("own", np.uint32),
                            part("embedded", np.uint32), part("reached", np.uint32), part("votes", np.uint64),
                            part("squares", np.uint64), part("home", np.int32), part("hcount", np.uint32),
                            part("hflags", np.uint32), whole("ksum"), whole("ksq"), whole("kmembers"), valid, skipped + lost,
                            N=self.cfg.N, first=first)

    # ---- do the communities hold triangles? (include/ammsb_triangles.h)
    def _triangles(self):
        return self._postfit_op("_triangles_op", "Triangles", "the triangles")

    def _simple_csr(self, edges, row_limit=True):
        """keys (a << 32) | b, or None for the training links -> (offsets [N + 1] int64, targets int32, M, skipped,
        dropped): the simple symmetric adjacency of the list, built on the device -- both directions of every key with both
        ends < N as 64-bit keys, sorted, made unique, loops removed; skipped counts the keys with an end >= N, dropped the
        repeats (in either order) and loops.  That of the training links is built once and kept.  row_limit: refuse a row
        longer than the triangles library takes."""
        from . import _triangles
        if edges is None and getattr(self, "_training_simple_csr", None) is not None:
            if row_limit:
                _triangles.check_rows(self._training_simple_longest)
            return self._training_simple_csr
        N = self.cfg.N
        if N >= 2 ** 31:
            raise AmmsbError("triangles: the simplification sorts signed 64-bit keys and takes N < 2^31")
        keys = self._linkcomm_edges(edges)
        if keys.dtype != torch.int64 or keys.dim() != 1:
            raise AmmsbError("triangles: edges must be 1-d uint64 keys (a << 32) | b")
        a, b = (keys >> 32) & 0xFFFFFFFF, keys & 0xFFFFFFFF
        ok = (a < N) & (b < N)
        a, b = a[ok], b[ok]
        both = torch.unique(torch.cat(((a << 32) | b, (b << 32) | a)))   # (sorted)
        both = both[(both >> 32) != (both & 0xFFFFFFFF)]
        src = both >> 32
        rows = torch.bincount(src, minlength=N)
        longest = int(rows.max()) if N else 0
        if row_limit:
            _triangles.check_rows(longest)
        offsets = torch.zeros(N + 1, dtype=torch.int64, device=keys.device)
        offsets[1:] = torch.cumsum(rows, 0)
        M = int(both.numel())
        out = (offsets, (both & 0xFFFFFFFF).to(torch.int32).contiguous(), M, int(keys.numel() - a.numel()),
               int(a.numel()) - M // 2)
        if edges is None:
            self._training_simple_csr, self._training_simple_longest = out, longest
        return out

    def Triangles(self, threshold=0.05, edges=None, nodes=None):
        """-> _triangles.Triangles: the triangles of every node (or of the range nodes=(first, count)) and of every
        community of the cover pi[a, k] >= threshold in a simple adjacency: that of the training links (edges=None), or
        that of `edges` (host array or device tensor of (a << 32) | b; repeats and loops counted in .dropped, a key with an
        end >= N in .skipped).  .degree, .tri, .tri_in (the triangles whose three corners share a community), .tri_comms
        per node; .ktri3 (three times the triangles inside k), .kpart (the members that are a corner of one), .kmembers,
        .wedges per community, all exact integers; .tpr, .triangles, .clustering [K], .local_clustering, .inside [n],
        .total, .transitivity, .avg_clustering on the host; .without_triangles().  A row of more than 65535 targets is
        refused."""
        from . import _triangles
        threshold = _triangles.check_threshold(threshold)
        first, count = _triangles.check_nodes(nodes, self.cfg.N)
        op, roles = self._triangles(), self._roles()
        self.drain()
        offsets, targets, M, skipped, dropped = self._simple_csr(edges)
        N, K = self.cfg.N, int(self.pi.cols)
        mask = op.links.mask(self.pi, threshold)
        st = op.nodes(mask, N, K, offsets, targets, first=first, count=count)
        # degree, kmembers and the wedges: the node roles without a selection over the same rows
        rs = roles.nodes(mask, N, K, offsets, targets, first=first, count=count, top=0)
        part = lambda s, name: s[name][first:first + count].cpu().numpy().view(np.uint32)   # noqa: E731
        whole = lambda s, name: s[name].cpu().numpy().view(np.uint64)                       # noqa: E731
        ksum, ksq = whole(rs, "ksum"), whole(rs, "ksq")
        return _triangles.Triangles(threshold, part(rs, "degree"), part(st, "tri"), part(st, "tri_in"), part(st, "tri_comms"),
                                    whole(st, "ktri3"), whole(st, "kpart"), whole(rs, "kmembers"), (ksq - ksum) // np.uint64(2),
                                    M, skipped, dropped, N=N, first=first)

    # ---- is each community one piece? (include/ammsb_components.h)
    def _components(self):
        return self._postfit_op("_components_op", "CommunityComponents", "the community components")

    def CommunityComponents(self, threshold=0.05, edges=None):
        """-> _components.Components: the connected components of every community of the cover pi[a, k] >= threshold inside
        the graph of `edges` (host array or device tensor of (a << 32) | b, either order of the ends, duplicates and a == a
        valid, a key with an end >= N counted in .skipped; default: TrainingLinks()), fewer than 2^31 keys: two members of k
        are connected iff a path of keys joins them through members of k.  .members, .components, .largest, .largest_root,
        .singletons per community; the memberships as a CSR over the nodes, .offsets [N + 1] and .community, .root, .size [M]
        (the root of a component is its smallest node); .stray [N], the memberships outside their community's largest
        component; .links, .skipped, .shared, .M, all exact integers; .giant, .fragmentation [K] and .connected in float64 on
        the host; .disconnected(), .cover(), .trimmed().  A cover of 2^32 memberships or more is refused."""
        from . import _components
        threshold = _components.check_threshold(threshold)
        op = self._components()
        self.drain()
        edges = self._linkcomm_edges(edges)
        _components.check_keys(edges.numel())
        st, base, M = op.run(self.pi, threshold, edges)
        valid, skipped, shared, giveups = (int(v) for v in st["counts"].cpu().numpy().view(np.uint64))
        _components.check_giveups(giveups)
        h = lambda name, dt: st[name].cpu().numpy().view(dt)   # noqa: E731
        return _components.Components(threshold, h("members", np.uint64), h("components", np.uint64), h("largest", np.uint32),
                                      h("largest_root", np.int32), h("singletons", np.uint64), base.cpu().numpy().view(np.uint64),
                                      h("slot_comm", np.uint16), h("root", np.uint32), h("size", np.uint32), h("stray", np.uint32),
                                      valid, skipped, shared)

    # ---- where does a node sit inside a community? (include/ammsb_cores.h)
    def _cores(self):
        return self._postfit_op("_cores_op", "CommunityCores", "the community cores")

    def CommunityCores(self, threshold=0.05, edges=None, max_bytes=4 << 30):
        """-> _cores.Cores: the k-core decomposition of the subgraph every community of the cover pi[a, k] >= threshold
        induces in a simple adjacency: that of the training links (edges=None), or that of `edges` (host array or device
        tensor of (a << 32) | b; repeats and loops counted in .dropped, a key with an end >= N in .skipped; a row may have
        any length).  .members, .inlinks2, .degeneracy, .nucleus, .isolated per community; the memberships as a CSR over the
        nodes, .offsets [N + 1] and .community, .indeg, .core [M]; .best_core, .best_comm, .in_nucleus [N]; .M, .L, .skipped,
        .dropped, all exact integers, and the launch counts .scans and .rounds; .coreness [M], .nucleus_share, .mean_core
        [K] in float64 on the host; .shells(k), .cover(c), .nuclei(), .fringe(c).  A cover of 2^32 memberships or more, and
        induced subgraphs whose neighbour lists take 2^32 entries or more than max_bytes, are refused before the peel."""
        from . import _cores
        threshold = _cores.check_threshold(threshold)
        _cores.check_nodes(self.cfg.N)
        op = self._cores()
        self.drain()
        offsets, targets, _, skipped, dropped = self._simple_csr(edges, row_limit=False)
        st, base, M, slot_comm, indeg, _, _ = op.run(self.pi, threshold, offsets, targets, max_bytes)
        counts = [int(v) for v in st["counts"].cpu().numpy().view(np.uint64)]
        h = lambda t, dt: t.cpu().numpy().view(dt)   # noqa: E731
        r = _cores.Cores(threshold, h(st["members"], np.uint64), h(st["inlinks2"], np.uint64), h(st["degeneracy"], np.uint32),
                         h(st["nucleus"], np.uint64), h(st["isolated"], np.uint64), h(base, np.uint64), h(slot_comm, np.uint16),
                         h(indeg, np.uint32), h(st["deg"], np.uint32), h(st["best_core"], np.uint32), h(st["best_comm"], np.int32),
                         h(st["in_nucleus"], np.uint32), skipped, dropped, counts[2], counts[3])
        if (counts[0], counts[1]) != (r.M, r.L):
            raise AmmsbError("cores: the device counted %d slots and %d neighbour entries, the arrays hold %d and %d"
                             % (counts[0], counts[1], r.M, r.L))
        return r
