"""Host-side mirror of the reference's operator interface on top of the C ABI.

Same names, argument meaning and error behaviour as the C++ functors of the reference, so that the
parity tests read like the reference's own tests:

    PhiUpdater            mcmc/phi.h:10-61      operator()(nodes, neighbors, n)
    BetaUpdater           mcmc/beta.h:15-72     operator()(edges, n, scale), GetThetaSum(), GetGrads()
    PerplexityCalculator  mcmc/perplexity.h:23-114   operator()()
    NeighborSampler       mcmc/sample.h:16-49   operator()(n, nodes), GetData(), GetHash()
    Random                mcmc/random.h:22-47   OpenClRandom (seed array)
    DeviceSet             mcmc/cuckoo.h:69-86   OpenClSet
    RowPartitionedMatrix  mcmc/partitioned-alloc.h:73-140

torch is used for device memory and streams only.  Every method enqueues on the current torch HIP
stream and returns without synchronising (the reference calls queue.Finish() after each launch; a
caller that wants that behaviour calls torch.cuda.synchronize()).
"""
import ctypes as C
import os
import threading

import numpy as np
import torch

from . import _capi
from ._capi import AmmsbError, NOISE_OFF, PHI_STREAMING, Params, PpxSums, Rpm, SetDesc, check

SEED_DT = np.dtype([("x", np.uint64), ("y", np.uint64)])


# torch.cuda.current_stream() costs ~3 us and every launch needs the handle (a dozen per iteration, a third of
# the host time of a step).  The streams this module switches to itself (`stream(s)` below) are tracked per
# thread, and a caller that owns a loop can pin the ambient stream for its duration (`pin_current_stream`);
# anything else falls back to asking torch.
_tls = threading.local()


def _stream():
    stack = getattr(_tls, "stack", None)
    if stack:
        return stack[-1]
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _torch_stream():
    """The torch.cuda.Stream object of the same cache (events are recorded on / waited for by stream OBJECTS: an
    Event.record() without one asks torch for the current stream, ~8 us, six times per iteration of the multi-GPU
    schedule)."""
    stack = getattr(_tls, "tstack", None)
    if stack:
        return stack[-1]
    return torch.cuda.current_stream()


class pin_current_stream:
    """with pin_current_stream(): ...  -- the stream that is current on entry is used for every launch of this
    thread inside the block (unless `stream(s)` switches), without asking torch again."""

    def __enter__(self):
        if not hasattr(_tls, "stack"):
            _tls.stack, _tls.tstack = [], []
        cur = torch.cuda.current_stream()
        _tls.stack.append(C.c_void_p(cur.cuda_stream))
        _tls.tstack.append(cur)
        return self

    def __exit__(self, *exc):
        _tls.stack.pop()
        _tls.tstack.pop()
        return False


class _StreamScope:
    """torch.cuda.stream(s) plus the handle cache above."""

    def __init__(self, s):
        self.s = s
        self.tc = torch.cuda.stream(s)

    def __enter__(self):
        self.tc.__enter__()
        if not hasattr(_tls, "stack"):
            _tls.stack, _tls.tstack = [], []
        _tls.stack.append(C.c_void_p(self.s.cuda_stream))
        _tls.tstack.append(self.s)
        return self

    def __exit__(self, *exc):
        _tls.stack.pop()
        _tls.tstack.pop()
        return self.tc.__exit__(*exc)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def make_params(N, K, E=0, num_node_sample=32, alpha=0.0, a=0.0315, b=1024.0, c=0.5, epsilon=1e-7,
                eta0=1.0, eta1=1.0, quantize=True):
    """mcmc::Config numeric fields (config.h:25-102) with main.cc's rule alpha == 0 -> 1/K
    (main.cc:153).  quantize applies MakeCompileFlags' "%e" round trip (config.cc:57-83)."""
    if alpha == 0:
        alpha = float(np.float32(1.0) / np.float32(K))
    p = Params(N, K, E, num_node_sample, alpha, a, b, c, epsilon, eta0, eta1)
    if quantize:
        check(_capi.load().ammsb_params_quantize(C.byref(p)))
    return p


class Context:
    """One per device; owns the C-ABI context (replaces clcuda::Queue + the JIT-built programs)."""

    def __init__(self, params, device=None):
        if not torch.cuda.is_available():
            raise AmmsbError("no HIP device visible: the MI355X path has no CPU fallback")
        self.lib = _capi.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.params = params
        self._ctx = C.c_void_p()
        check(self.lib.ammsb_ctx_create(self.device.index, C.byref(params), C.byref(self._ctx)))

    @property
    def handle(self):
        return self._ctx

    def check(self, rc):
        check(rc, self._ctx)

    KERNELS = ("update_phi", "update_pi", "beta_grads", "perplexity", "update_phi_small", "sample_neighbors",
               "grads_sum")

    def kernel_names(self):
        """Names of the kernels the last update_phi / update_pi / gradient / perplexity / sampler calls on this context
        dispatched to, spelled as in a rocprofv3 kernel trace (ammsb_last_kernel_name).  "update_phi" is the form large
        launches take, "update_phi_small" the several-waves-per-node form of launches of at most 512 groups (link
        mini-batches); a context that has only ever made small launches reports that one under both keys."""
        names = {k: self.lib.ammsb_last_kernel_name(self.handle, i).decode() for i, k in enumerate(self.KERNELS)}
        if not names["update_phi"]:
            names["update_phi"] = names["update_phi_small"]
        return names

    def close(self):
        if self._ctx:
            self.lib.ammsb_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- small allocation helpers (device memory comes from torch's caching allocator)
    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def from_numpy(self, arr):
        a = np.ascontiguousarray(arr)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        elif a.dtype == SEED_DT:
            a = a.view(np.int64).reshape(-1, 2)
        return torch.from_numpy(a).to(self.device)


def to_numpy(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a.view(dtype) if dtype is not None else a


class Random:
    """OpenClRandom: `size` xorshift128+ streams, stream i seeded {sx+i, sy+i} (random.cc:31-43)."""

    def __init__(self, ctx, size, seed, mixed=False):
        self.ctx = ctx
        self.size = int(size)
        self.mixed = bool(mixed)  # SplitMix64-scrambled states (streams the reference does not have)
        self.seeds = ctx.empty((self.size, 2), torch.int64)
        self.SetSeed(seed)

    def SetSeed(self, seed):
        sx, sy = seed
        fn = self.ctx.lib.ammsb_rng_init_mixed if self.mixed else self.ctx.lib.ammsb_rng_init
        self.ctx.check(fn(self.ctx.handle, _ptr(self.seeds), self.size, int(sx), int(sy), _stream()))

    def GetSeeds(self):
        return self.seeds

    def host(self):
        return to_numpy(self.seeds).view(np.uint64).reshape(-1, 2).copy().view(SEED_DT).reshape(-1)

    def load(self, seeds):
        self.seeds.copy_(self.ctx.from_numpy(seeds))


class DeviceSet:
    """OpenClSet: device image of a host cuckoo Set (cuckoo.cc:222-239).  `slots` is the array
    Set::Serialize() returns; num_bins = BinsPerBucket(); prime_idx = PrimeIdx()."""

    def __init__(self, ctx, slots, num_bins, prime_idx):
        slots = np.ascontiguousarray(slots, dtype=np.uint64)
        if slots.size != 2 * int(num_bins) * 4:
            raise AmmsbError("set image has %d slots, expected 2*%d*4" % (slots.size, num_bins))
        self.ctx = ctx
        self.data = ctx.from_numpy(slots)
        self.num_bins = int(num_bins)
        self.prime_idx = int(prime_idx)
        self.desc = SetDesc(self.data.data_ptr(), self.num_bins, self.prime_idx)

    @classmethod
    def build_on_device(cls, ctx, keys):
        """Opt-in parallel construction on the GPU (ammsb_set_build): same layout and hash pairs, exact membership,
        a different (interleaving-dependent) image than the host's rand_r random-walk build, which stays the
        default and is what parity runs use.  `keys`: distinct u64 keys, a device tensor or a host array."""
        k = keys if torch.is_tensor(keys) else ctx.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64))
        n = int(k.numel())
        self = cls.__new__(cls)
        self.ctx = ctx
        self.num_bins = int(ctx.lib.ammsb_set_num_bins(n))
        self.data = ctx.empty((2 * self.num_bins * 4,), torch.int64)
        scratch = ctx.zeros((1,), torch.int32)
        pidx = C.c_uint32(0)
        ctx.check(ctx.lib.ammsb_set_build(ctx.handle, _ptr(k), n, _ptr(self.data), self.num_bins, C.byref(pidx),
                                          _ptr(scratch), _stream()))
        self.prime_idx = int(pidx.value)
        self.desc = SetDesc(self.data.data_ptr(), self.num_bins, self.prime_idx)
        return self

    def Has(self, keys):
        """The `find` kernel of cuckoo-test.cc:45-53 over a device or host key array."""
        k = keys if torch.is_tensor(keys) else self.ctx.from_numpy(np.asarray(keys, dtype=np.uint64))
        out = self.ctx.empty((k.numel(),), torch.uint8)
        self.ctx.check(self.ctx.lib.ammsb_set_has(self.ctx.handle, C.byref(self.desc), _ptr(k), k.numel(),
                                                  _ptr(out), _stream()))
        return out


class RowPartitionedMatrix:
    """RowPartitionedMatrix<float> (partitioned-alloc.h:73-140): rows split into <= 32 blocks of
    rows_in_block rows.  On a 288 GB MI355X one block holds any configuration of interest, so
    rows_in_block defaults to all rows; a smaller value reproduces the reference's multi-block
    layout (tests use 11+1 blocks)."""

    def __init__(self, ctx, rows, cols, rows_in_block=0, dtype=torch.float32):
        self.ctx = ctx
        self.rows, self.cols = int(rows), int(cols)
        self.rows_in_block = int(rows_in_block) if rows_in_block else self.rows
        nfull, rem = divmod(self.rows, self.rows_in_block)
        sizes = [self.rows_in_block] * nfull + ([rem] if rem else [])
        if len(sizes) > _capi.RPM_MAX_BLOCKS:
            raise AmmsbError("more than 32 blocks")
        self.blocks = [ctx.empty((s, self.cols), dtype) for s in sizes]
        self.desc = Rpm()
        for i, b in enumerate(self.blocks):
            self.desc.blocks[i] = b.data_ptr()
        self.desc.rows_in_block = self.rows_in_block
        self.desc.num_rows = self.rows
        self.desc.num_cols = self.cols
        self.desc.num_blocks = len(self.blocks)

    def adopt(self, other):
        """Take over `other`'s storage (same shape): every holder of this object then works on the new blocks."""
        if (other.rows, other.cols, other.rows_in_block) != (self.rows, self.cols, self.rows_in_block):
            raise AmmsbError("adopt: shapes differ")
        self.blocks, self.desc = other.blocks, other.desc

    def Rows(self):
        return self.rows

    def Cols(self):
        return self.cols

    def RowsPerBlock(self):
        return self.rows_in_block

    def Blocks(self):
        return self.blocks

    def load(self, host):
        host = np.ascontiguousarray(host).reshape(self.rows, self.cols)
        r = 0
        for b in self.blocks:
            b.copy_(self.ctx.from_numpy(host[r:r + b.shape[0]]))
            r += b.shape[0]

    def host(self):
        return np.concatenate([to_numpy(b) for b in self.blocks], axis=0)

    def gather_rows(self, rows):
        """rows (device int64 tensor) -> [len, cols] tensor; single-block fast path."""
        if len(self.blocks) == 1:
            return self.blocks[0][rows]
        return torch.cat(self.blocks, 0)[rows]


def RandomGammaAndNormalize(ctx, eta0, eta1, pi, phi_sum, seed=(11, 113)):
    """random.cc:159-167: N*32 streams seeded {11,113}; pi rows ~ Gamma, normalised; phi_sum = sums."""
    rnd = Random(ctx, pi.Rows() * 32, seed)
    ctx.check(ctx.lib.ammsb_pi_init_gamma(ctx.handle, C.byref(pi.desc), _ptr(phi_sum), eta0, eta1,
                                          _ptr(rnd.seeds), _stream()))
    return rnd


class NeighborSampler:
    """sample.h:16-49.  max_nodes = max(2*mini_batch, 1+MaxFanOut) sizes the buffers (sample.cc:88-97)."""

    def __init__(self, ctx, max_nodes, neighbor_seed=(56, 57), wg=32):
        self.ctx = ctx
        self.n = ctx.params.num_node_sample
        self.capacity = 2 * self.n
        self.local = int(wg)
        self.hash = ctx.empty((max_nodes, self.capacity), torch.int32)
        self.data = ctx.empty((max_nodes, self.n), torch.int32)
        self.rand = Random(ctx, max_nodes * self.capacity, neighbor_seed)
        self.max_nodes = int(max_nodes)

    def __call__(self, num_samples, nodes):
        if num_samples > self.max_nodes:
            raise AmmsbError("%d samples > buffer for %d" % (num_samples, self.max_nodes))
        self.ctx.check(self.ctx.lib.ammsb_sample_neighbors(
            self.ctx.handle, _ptr(self.rand.seeds), _ptr(nodes), int(num_samples), self.local,
            _ptr(self.hash), _ptr(self.data), _stream()))

    def GetHash(self):
        return self.hash

    def GetData(self):
        return self.data

    def HashCapacityPerSample(self):
        return self.capacity

    def DataSizePerSample(self):
        return self.n


class PhiUpdater:
    """phi.h:10-61 / phi.cc:608-763.  mode is always the work-group form on this hardware."""

    def __init__(self, ctx, beta, pi, phi, training_set, max_nodes, phi_seed=(42, 43), phi_wg_size=64,
                 phi_disable_noise=False, streaming_only=False):
        self.ctx, self.beta, self.pi, self.phi, self.set = ctx, beta, pi, phi, training_set
        self.local = int(phi_wg_size)
        # streaming_only: small launches too go through the one-wave-per-node kernels (AMMSB_PHI_STREAMING)
        self.flags = (NOISE_OFF if phi_disable_noise else 0) | (PHI_STREAMING if streaming_only else 0)
        self.max_nodes = int(max_nodes)
        self.phi_vec = ctx.empty((self.max_nodes, ctx.params.K), torch.float32)
        # phi.cc:625-629: max(2m, 1+maxdeg) * wg streams
        self.rand = Random(ctx, self.max_nodes * self.local, phi_seed)
        self.count_calls = 0

    def update_phi(self, nodes, neighbors, n, group_begin=0, group_end=0xFFFFFFFF):
        if n == 0:
            raise AmmsbError("mini-batch nodes size = 0!")  # phi.cc:732
        if n > self.max_nodes:
            raise AmmsbError("grads too small")  # phi.cc:734-737 analogue
        c = self.ctx
        c.check(c.lib.ammsb_update_phi(c.handle, _ptr(self.beta), C.byref(self.pi.desc), _ptr(self.phi),
                                       C.byref(self.set.desc), _ptr(nodes), _ptr(neighbors), int(n),
                                       self.count_calls, _ptr(self.rand.seeds), self.local, self.flags,
                                       int(group_begin), int(group_end), _ptr(self.phi_vec), _stream()))

    def update_pi(self, nodes, n, phi_vec=None):
        c = self.ctx
        pv = self.phi_vec if phi_vec is None else phi_vec
        c.check(c.lib.ammsb_update_pi(c.handle, C.byref(self.pi.desc), _ptr(self.phi), _ptr(pv),
                                      _ptr(nodes), int(n), self.local, _stream()))

    def __call__(self, mini_batch_nodes, neighbors, num_mini_batch_nodes):
        self.count_calls += 1  # phi.cc:739
        self.update_phi(mini_batch_nodes, neighbors, num_mini_batch_nodes)
        self.update_pi(mini_batch_nodes, num_mini_batch_nodes)


class BetaUpdater:
    """beta.h:15-72 / beta.cc:236-384 (EDGE_PER_WORKGROUP)."""

    def __init__(self, ctx, theta, beta, pi, training_set, beta_seed=(44, 45), beta_wg_size=256,
                 disable_noise=False):
        self.ctx, self.theta, self.beta, self.pi, self.set = ctx, theta, beta, pi, training_set
        self.local = int(beta_wg_size)
        self.flags = NOISE_OFF if disable_noise else 0
        self.rand = Random(ctx, ctx.params.K, beta_seed)  # beta.cc:251-252
        self.grads = ctx.zeros((2 * ctx.params.K,), torch.float32)
        self.count_calls = 0

    def calculate_grads(self, edges, num_edges, edge_begin=0, edge_end=0xFFFFFFFF, out=None):
        c = self.ctx
        g = self.grads if out is None else out
        c.check(c.lib.ammsb_beta_grads(c.handle, _ptr(self.theta), _ptr(self.beta), C.byref(self.pi.desc),
                                       C.byref(self.set.desc), _ptr(edges), int(num_edges), int(edge_begin),
                                       int(min(edge_end, num_edges)), self.local, _ptr(g), _stream()))
        return g

    def can_fuse_update_pi(self, phi_updater):
        """Whether update_pi_and_grads takes this context's (K, work-group sizes)."""
        c = self.ctx
        return bool(c.lib.ammsb_can_fuse_pi_beta(c.handle, int(phi_updater.local), self.local))

    def update_pi_and_grads(self, phi_updater, nodes, edges, num_edges, out=None):
        """phi_updater.update_pi(nodes, num_edges + 1) and calculate_grads(edges, num_edges) as one launch
        (ammsb_update_pi_beta_grads): node-stratified mini-batches only -- edge t = (nodes[0], nodes[t + 1])."""
        c = self.ctx
        g = self.grads if out is None else out
        c.check(c.lib.ammsb_update_pi_beta_grads(c.handle, _ptr(self.theta), _ptr(self.beta), C.byref(self.pi.desc),
                                                 _ptr(phi_updater.phi), _ptr(phi_updater.phi_vec), _ptr(nodes),
                                                 C.byref(self.set.desc), _ptr(edges), int(num_edges), self.local,
                                                 _ptr(g), _stream()))
        return g

    def update_theta(self, scale, grads=None):
        c = self.ctx
        g = self.grads if grads is None else grads
        c.check(c.lib.ammsb_update_theta(c.handle, _ptr(self.theta), _ptr(self.beta), _ptr(g),
                                         self.count_calls, float(scale), _ptr(self.rand.seeds), self.flags,
                                         _stream()))

    def __call__(self, edges, num_edges, scale):
        self.count_calls += 1  # beta.cc:336
        self.calculate_grads(edges, num_edges)
        self.update_theta(scale)

    def GetGrads(self):
        return self.grads

    def GetThetaSum(self):
        """theta_sum of the last gradient launch (beta.h:27), as a device tensor [K]."""
        c = self.ctx
        out = c.empty((c.params.K,), torch.float32)
        c.check(c.lib.ammsb_theta_sum(c.handle, _ptr(out), _stream()))
        return out


def sum_rows(ctx, rows, out):
    """out[c] = rows[0, c] + rows[1, c] + ... in ascending row order (the multi-GPU gradient reduction)."""
    ctx.check(ctx.lib.ammsb_sum_rows_f32(ctx.handle, _ptr(rows), int(rows.shape[0]), int(rows.shape[1]), _ptr(out),
                                         _stream()))
    return out


def beta_from_theta(ctx, theta, beta):
    ctx.check(ctx.lib.ammsb_beta_from_theta(ctx.handle, _ptr(theta), _ptr(beta), _stream()))


class PerplexityCalculator:
    """perplexity.h:23-114 / perplexity.cc:184-274 (EDGE_PER_WORKGROUP)."""

    def __init__(self, ctx, beta, pi, edges, edge_set, ppx_wg_size=64):
        self.ctx, self.beta, self.pi, self.edges, self.set = ctx, beta, pi, edges, edge_set
        self.local = int(ppx_wg_size)
        self.num_edges = int(edges.numel())
        self.ppx_per_edge = ctx.zeros((max(self.num_edges, 1),), torch.float32)  # perplexity.cc:204-205
        self.dev_sums = ctx.zeros((4,), torch.int64)  # ammsb_ppx_sums
        # the same 32 bytes in host-mapped pinned memory: the kernel writes its result where the host reads it, so a
        # call is one launch and one stream synchronisation (no device-to-host copy)
        self.host_sums = torch.zeros((4,), dtype=torch.int64, pin_memory=True)
        self.sums = self.dev_sums  # where the last pass put its result (device tensor, or host_sums after operator())
        self.count_calls = 0

    def partial(self, edge_begin=0, edge_end=0xFFFFFFFF, out=None):
        """Enqueue one pass over edges [edge_begin, edge_end); returns the sums tensor (device memory unless `out`)."""
        c = self.ctx
        out = self.dev_sums if out is None else out
        self.sums = out
        c.check(c.lib.ammsb_perplexity(c.handle, _ptr(self.beta), C.byref(self.pi.desc), C.byref(self.set.desc),
                                       _ptr(self.edges), self.num_edges, int(edge_begin),
                                       int(min(edge_end, self.num_edges)), self.count_calls, self.local,
                                       _ptr(self.ppx_per_edge), _ptr(out), _stream()))
        return out

    def partial_host(self, edge_begin=0, edge_end=0xFFFFFFFF):
        """One pass with the sums written straight into pinned host memory; waits for the stream and returns
        (link_ll, nonlink_ll, link_cnt, nonlink_cnt)."""
        self.partial(edge_begin, edge_end, out=self.host_sums)
        torch.cuda.current_stream().synchronize()
        raw = self.host_sums.numpy()
        ll = raw[:2].view(np.float64)
        cnt = raw[2:].view(np.uint64)
        return float(ll[0]), float(ll[1]), int(cnt[0]), int(cnt[1])

    @staticmethod
    def unpack(sums):
        raw = to_numpy(sums)
        ll = raw[:2].view(np.float64)
        cnt = raw[2:].view(np.uint64)
        return float(ll[0]), float(ll[1]), int(cnt[0]), int(cnt[1])

    @staticmethod
    def value(link_ll, nonlink_ll, link_cnt, nonlink_cnt):
        avg = 0.0
        if link_cnt + nonlink_cnt != 0:  # perplexity.cc:264-268
            avg = (link_ll + nonlink_ll) / (link_cnt + nonlink_cnt)
        return -avg

    def __call__(self):
        self.count_calls += 1  # perplexity.cc:252
        return self.value(*self.partial_host())


MB_CHOICE_DT = np.dtype([("link", np.uint32), ("u", np.uint32), ("n", np.uint32), ("n_candidates", np.uint32)])


class DeviceMiniBatchSampler:
    """Device-side replacement for sampleNode + ExtractNodesFromMiniBatch (sample.cc:249-303,
    learner.cc:162-173).  The coin flip and the choice of u stay on the host (a numpy Generator), so
    the sizes of the mini-batch are known without reading anything back; the m distinct non-links /
    the edges of u are produced on the device straight into the caller's edge and node buffers.

    A mini-batch is first CHOSEN (`choose`: link?, u, deg(u), candidate draws) and then ENQUEUED
    (`enqueue`, eager) or handed to the captured-graph loop (GraphLoop.run), so both paths consume the
    same host stream of choices.  The number of candidate draws of a non-link batch follows the vertex:
    enough for m + 1 + deg_training(u) + deg_heldout(u) distinct values (every invalid partner of u
    could be drawn) plus the 8 % + 1024 margin, so a hub vertex cannot come up short.  A shortfall by
    sheer bad luck is still detected: the device keeps a sticky counter that `check()` reads at the
    learner's synchronisation points."""

    BLOCK = 64  # choices drawn from the host generator at a time

    def __init__(self, ctx, csr_offsets, csr_targets, training_set, heldout_set, mini_batch, seed=(1234, 5678),
                 host_seed=20260101, heldout_degree=None):
        self.ctx = ctx
        self.m = int(mini_batch)
        self.N, self.E = int(ctx.params.N), int(ctx.params.E)
        self.training_set, self.heldout_set = training_set, heldout_set
        off = np.ascontiguousarray(csr_offsets, dtype=np.uint64)
        self.degree = np.diff(off.astype(np.int64))
        if not (self.degree > 0).any():
            raise AmmsbError("training graph has no edges")
        self.max_fan_out = int(self.degree.max())
        self.excluded = self.degree + 1  # invalid partners of u: itself and its neighbours in both graphs
        if heldout_degree is not None:
            self.excluded = self.excluded + np.asarray(heldout_degree, dtype=np.int64)
        self.offsets = ctx.from_numpy(off)
        self.targets = ctx.from_numpy(np.ascontiguousarray(csr_targets, dtype=np.uint32))
        self._cand = {}
        self.C = self._candidates_for(int(self.excluded.max()))  # capacity: streams and workspace
        if self.C == 0:
            raise AmmsbError("device sampling needs N >= 2 * mini_batch with room for the largest degree "
                             "(N=%d, m=%d, max excluded=%d)" % (self.N, self.m, int(self.excluded.max())))
        self.rand = Random(ctx, self.C, seed, mixed=True)
        # 0xFF once: every call leaves the de-duplication table empty again (include/ammsb.h)
        self.workspace = torch.full((int(ctx.lib.ammsb_minibatch_workspace_bytes(self.C)),), 255, dtype=torch.uint8,
                                    device=ctx.device)
        self.count = ctx.zeros((2,), torch.int32)  # [0] distinct candidates of the last call, [1] sticky shortfalls
        self.host_rng = np.random.default_rng(host_seed)
        self.queue = []  # choices drawn ahead, BLOCK at a time: (coin, u) pairs not yet consumed
        self.w_link = float(np.float32(self.N))                               # sample.cc:268
        self.w_nonlink = float(np.float32(2 * self.E) / np.float32(self.m))   # sample.cc:292
        # The candidate streams, the workspace and the counter are shared by successive calls, which the learner
        # issues on two alternating streams: each call waits for the previous one's kernels before it starts.
        self._done = torch.cuda.Event()
        self._done_valid = False

    def _candidates_for(self, excluded):
        key = (int(excluded) + 31) // 32 * 32  # few distinct values
        c = self._cand.get(key)
        if c is None:
            c = self._cand[key] = int(self.ctx.lib.ammsb_minibatch_candidates_for(self.N, self.m, key))
        return c

    def _refill(self):
        coins = self.host_rng.integers(0, 2, size=self.BLOCK)  # rand_r(seed) % 2, sample.cc:297
        us = self.host_rng.integers(0, self.N, size=self.BLOCK)
        self.queue = list(zip(coins.tolist(), us.tolist()))[::-1]

    def choose(self, strategy):
        """The next mini-batch: (link, u, n, n_candidates)."""
        link = {"Node": None, "NodeLink": True, "NodeNonLink": False}.get(strategy, "bad")
        if link == "bad":
            raise AmmsbError("device sampling implements Node / NodeLink / NodeNonLink only")
        while True:
            if not self.queue:
                self._refill()
            coin, u = self.queue.pop()
            is_link = bool(coin) if link is None else link
            if is_link:
                n = int(self.degree[u])
                if n == 0:  # sampleNodeLink retries until the vertex has an edge (sample.cc:254-263)
                    while True:
                        if not self.queue:
                            self._refill()
                        u = self.queue.pop()[1]
                        n = int(self.degree[u])
                        if n > 0:
                            break
                return (1, u, n, 0)
            return (0, u, 0, self._candidates_for(self.excluded[u]))

    def choose_many(self, strategy, n):
        """n consecutive choices as a structured array (link, u, n, n_candidates) -- the same host stream and the same
        results as n calls of choose(), drawn a block at a time and assembled with numpy (the graph loop hands
        hundreds of choices to the library per call; a Python loop per choice would be most of its host time)."""
        out = np.zeros(n, dtype=MB_CHOICE_DT)
        link_mode = {"Node": None, "NodeLink": True, "NodeNonLink": False}.get(strategy, "bad")
        if link_mode == "bad":
            raise AmmsbError("device sampling implements Node / NodeLink / NodeNonLink only")
        done = 0
        while done < n:
            if not self.queue:
                self._refill()
            take = min(len(self.queue), n - done)
            blk = np.array(self.queue[len(self.queue) - take:][::-1], dtype=np.int64)   # pop order
            coins, us = blk[:, 0], blk[:, 1]
            is_link = coins.astype(bool) if link_mode is None else np.full(take, link_mode)
            bad = is_link & (self.degree[us] == 0)
            if bad.any():   # a link choice on a vertex without edges consumes further queue entries: scalar path
                first = int(np.flatnonzero(bad)[0])
                take = first
            if take:
                del self.queue[len(self.queue) - take:]
                seg = out[done:done + take]
                lk = is_link[:take]
                seg["link"] = lk
                seg["u"] = us[:take]
                seg["n"] = np.where(lk, self.degree[us[:take]], 0)
                seg["n_candidates"] = np.where(lk, 0, self._cand_table()[(self.excluded[us[:take]] + 31) // 32])
                done += take
            if bad.any() and done < n:
                out[done] = self.choose(strategy)
                done += 1
        return out

    def _cand_table(self):
        """n_candidates by excluded-count bucket (32 per bucket), for choose_many."""
        t = getattr(self, "_cand_tab", None)
        if t is None:
            top = (int(self.excluded.max()) + 31) // 32
            t = self._cand_tab = np.array([self._candidates_for(32 * b) if b else self._candidates_for(1)
                                           for b in range(top + 1)], dtype=np.int64)
        return t

    def sizes(self, choice):
        """(n_edges, n_nodes, weight) of a choice."""
        link, u, n, _ = choice
        if link:
            return n, n + 1, self.w_link
        return self.m, self.m + 1, self.w_nonlink

    def enqueue(self, choice, dev_edges, dev_nodes):
        """Eager form: enqueue the kernels of one chosen mini-batch on the current stream."""
        c = self.ctx
        if self._done_valid:
            self._done.wait()
        link, u, n, n_cand = choice
        if link:
            c.check(c.lib.ammsb_minibatch_link(c.handle, _ptr(self.offsets), _ptr(self.targets), u, n,
                                               _ptr(dev_edges), _ptr(dev_nodes), _stream()))
        else:
            hs = C.byref(self.heldout_set.desc) if self.heldout_set is not None else None
            c.check(c.lib.ammsb_minibatch_nonlink(c.handle, _ptr(self.rand.seeds), n_cand, self.C, u, self.m,
                                                  C.byref(self.training_set.desc), hs, _ptr(self.workspace),
                                                  _ptr(dev_edges), _ptr(dev_nodes), _ptr(self.count), _stream()))
        self._done.record()
        self._done_valid = True
        return self.sizes(choice)

    def __call__(self, strategy, dev_edges, dev_nodes):
        """Choose and enqueue one mini-batch; returns (n_edges, n_nodes, weight)."""
        return self.enqueue(self.choose(strategy), dev_edges, dev_nodes)

    def mark_used(self):
        """The shared sampler state was just used by work queued on the current stream (a graph run)."""
        self._done.record()
        self._done_valid = True

    def check(self):
        """Raise if any non-link mini-batch since the last check found fewer than m distinct valid partners
        (its tail then repeats earlier entries: not a valid sample).  Synchronises; call at sync points."""
        short = int(self.count[1].item())
        if short:
            self.count[1].zero_()
            raise AmmsbError("device mini-batch sampler: %d mini-batch(es) found fewer than %d distinct non-links "
                             "(last count %d)" % (short, self.m, int(self.count[0].item())))

    def state(self):
        return dict(rng=self.host_rng.bit_generator.state, queue=[[int(a), int(b)] for a, b in self.queue])

    def load_state(self, st):
        self.host_rng.bit_generator.state = st["rng"]
        self.queue = [(int(a), int(b)) for a, b in st.get("queue", [])]


class ReferenceStreamSampler:
    """The reference's own mini-batch stream on the device (include/ammsb_refsample.h): from a Sample::seed exactly
    the edges, the node list (both in the reference's std::unordered_set iteration order), the weight and the seed
    afterwards that mcmc::sampleNode / sampleNodeLink / sampleNodeNonLink + ExtractNodesFromMiniBatch produce on the
    host (host/sample.cc), with no host-to-device copy of edges or nodes.  The host draws the coin and u (a few rand_r
    calls); candidates, de-duplication, both orders run on the device; 16 result bytes come back through host-mapped
    pinned memory.  Calls are serialised by the read of that result: one sampler serves both Samples."""

    def __init__(self, ctx, csr_offsets, csr_targets, training_set, heldout_set, mini_batch, heldout_degree=None,
                 capacity=None):
        from . import _refsample
        self.ctx = ctx
        self.rs = _refsample
        self.lib = _refsample.load()
        self.N = int(ctx.params.N)
        self.E = int(ctx.params.E)
        self.m = int(mini_batch)
        off = np.ascontiguousarray(csr_offsets, dtype=np.uint64)
        tgt = np.ascontiguousarray(csr_targets, dtype=np.uint32)
        self.degree = np.ascontiguousarray(np.diff(off.astype(np.int64)), dtype=np.uint32)
        if tgt.size and (tgt == np.repeat(np.arange(self.N, dtype=np.uint32), self.degree)).any():
            raise AmmsbError("reference-stream sampling: the training graph holds a self-loop")
        self.excluded = self.degree.astype(np.int64) + 1
        if heldout_degree is not None:
            self.excluded = self.excluded + np.asarray(heldout_degree, dtype=np.int64)
        self.max_fan_out = int(self.degree.max()) if self.degree.size else 0
        self.offsets = ctx.from_numpy(off.view(np.int64))
        self.targets = ctx.from_numpy(tgt.view(np.int32))
        self.training_set, self.heldout_set = training_set, heldout_set
        self._cand = {}
        # candidate capacity: the existing device sampler's sizing rule (ammsb_minibatch_candidates_for)
        self.C = int(capacity) if capacity is not None else self._candidates_for(int(self.excluded.max()))
        if self.C == 0:
            raise AmmsbError("device sampling needs N >= 2 * mini_batch with room for the largest degree "
                             "(N=%d, m=%d, max excluded=%d)" % (self.N, self.m, int(self.excluded.max())))
        # the longest list the ordering kernel may write: Dataset.max_edges(m) edges, one node more -- buffers handed to
        # enqueue() must hold that many (the Learner's Sample buffers do)
        self.max_items = max(self.m, self.max_fan_out) + 1
        self._h = C.c_void_p()
        rc = self.lib.ammsb_refsample_create(ctx.device.index, self.N, self.m, self.C, self.max_items,
                                             C.byref(self._h))
        if rc != 0:
            raise AmmsbError("ammsb_refsample_create failed: %d (N=%d, m=%d, capacity=%d)" % (rc, self.N, self.m, self.C))
        self.result = self.lib.ammsb_refsample_result_ptr(self._h)
        self.num_epochs = int(self.lib.ammsb_refsample_num_epochs(self._h))
        self.w_link = float(np.float32(self.N))                               # sample.cc:268
        self.w_nonlink = float(np.float32(2 * self.E) / np.float32(self.m))   # sample.cc:292
        self.shortfalls = 0   # sticky: mini-batches that found fewer than m distinct non-links among their candidates
        self.last_consumed = 0
        self._done = torch.cuda.Event()

    def _candidates_for(self, excluded):
        key = (int(excluded) + 31) // 32 * 32
        c = self._cand.get(key)
        if c is None:
            c = self._cand[key] = int(self.ctx.lib.ammsb_minibatch_candidates_for(self.N, self.m, key))
        return c

    def candidates(self, u):
        """Candidates a non-link mini-batch around u draws (never more than the capacity)."""
        return min(self._candidates_for(self.excluded[u]), self.C)

    def choose(self, strategy, seed):
        """The host's share: (link, u, seed once u is known)."""
        code = self.rs.STRATEGIES.get(strategy)
        if code is None:
            raise AmmsbError("device sampling implements Node / NodeLink / NodeNonLink only")
        s, link, u = C.c_uint32(int(seed)), C.c_uint32(0), C.c_uint32(0)
        rc = self.lib.ammsb_refsample_choose(code, self.N, self.degree.ctypes.data, C.byref(s), C.byref(link),
                                             C.byref(u))
        if rc != 0:
            raise AmmsbError("reference-stream sampling: no vertex with a training edge (rc %d)" % rc)
        return bool(link.value), int(u.value), int(s.value)

    def enqueue(self, strategy, seed, dev_edges, dev_nodes):
        """Draw one mini-batch from `seed` on the current stream and wait for its 16 result bytes (this stream only).
        Returns (n_edges, n_nodes, weight, seed afterwards)."""
        link, u, state = self.choose(strategy, seed)
        if int(dev_edges.numel()) < self.max_items - 1 or int(dev_nodes.numel()) < self.max_items:
            raise AmmsbError("reference-stream sampling: the buffers hold %d edges / %d nodes, a mini-batch may have %d / %d"
                             % (dev_edges.numel(), dev_nodes.numel(), self.max_items - 1, self.max_items))
        if link:
            rc = self.lib.ammsb_refsample_link(self._h, _ptr(self.offsets), _ptr(self.targets), u, int(self.degree[u]),
                                               _ptr(dev_edges), _ptr(dev_nodes), _stream())
        else:
            hs = C.byref(self.heldout_set.desc) if self.heldout_set is not None else None
            rc = self.lib.ammsb_refsample_nonlink(self._h, u, state, self.candidates(u),
                                                  C.byref(self.training_set.desc), hs, _ptr(dev_edges),
                                                  _ptr(dev_nodes), _stream())
        if rc != 0:
            raise AmmsbError("reference-stream sampling failed: %d (%s)"
                             % (rc, self.lib.ammsb_refsample_last_error(self._h).decode()))
        self._done.record(_torch_stream())
        self._done.synchronize()
        r = self.result.contents
        ne, nv, consumed, short = int(r.n_edges), int(r.n_nodes), int(r.consumed), int(r.shortfall)
        self.last_consumed = consumed
        if short:
            self.shortfalls += 1
            raise AmmsbError("device mini-batch sampler: %d mini-batch(es) found fewer than %d distinct non-links "
                             "(last count %d)" % (self.shortfalls, self.m, ne))
        return ne, nv, (self.w_link if link else self.w_nonlink), self.rs.jump(state, consumed)

    __call__ = enqueue

    def check(self):
        """Raise if a mini-batch since the last check came up short (enqueue raises at once; this is for a caller that
        caught that and went on)."""
        if self.shortfalls:
            n, self.shortfalls = self.shortfalls, 0
            raise AmmsbError("device mini-batch sampler: %d mini-batch(es) found fewer than %d distinct non-links"
                             % (n, self.m))

    def close(self):
        if self._h:
            self.lib.ammsb_refsample_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _edge_keys(ctx, edges, what):
    """edge keys (a << 32) | b, a host array or a contiguous 1-d int64 (uint64 bits) device tensor -> the device tensor"""
    if not torch.is_tensor(edges):
        edges = ctx.from_numpy(np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1))
    if edges.dtype != torch.int64 or edges.dim() != 1 or not edges.is_contiguous():
        raise AmmsbError("%s: edges must be a contiguous 1-d int64 (uint64 bits) device tensor" % what)
    return edges


def _u32_vector(ctx, x, what):
    """uint32 values, a host array or a contiguous 1-d int32 (uint32 bits) device tensor -> the device tensor"""
    if not torch.is_tensor(x):
        x = ctx.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).reshape(-1))
    if x.dtype != torch.int32 or x.dim() != 1 or not x.is_contiguous():
        raise AmmsbError("%s must be a contiguous 1-d int32 (uint32 bits) device tensor" % what)
    return x


def _check_mask(mask, N, K, who):
    """the node-major membership bits CommunityLinks.mask() makes of an N x K pi: a contiguous int64 [N, ceil(K / 64)]"""
    if mask.dtype != torch.int64 or not mask.is_contiguous() or mask.numel() != N * ((K + 63) // 64):
        raise AmmsbError("%s: not the mask of a %d x %d pi" % (who, N, K))


class CommunityReadout:
    """The read-out of a fitted pi (include/ammsb_readout.h): per row the T strongest communities with their weights
    (value descending, equal values by column ascending), the number of columns >= thr, and per community the number of
    rows >= thr.  Exact: weights are the stored values.  Owns nothing but the output tensors it returns; ids come back
    as int32 (torch has no arithmetic on uint32), so the empty slot 0xFFFFFFFF reads -1."""

    def __init__(self, ctx):
        from . import _readout
        self.ctx = ctx
        self.ro = _readout
        self.lib = _readout.load()

    def top(self, pi, T, thr, nodes=None, rows=None, sizes=None):
        """-> (ids [n, T] int32, weights [n, T] float32, count [n] int32) on the device, for rows `rows` = (lo, hi) of
        pi (default: all) or for the device / host list `nodes`.  sizes: a [K] int64 device tensor to accumulate the
        community sizes of these rows into (the caller zeroes it)."""
        T, thr = self.ro.check_args(T, thr)
        if nodes is not None:
            if rows is not None:
                raise AmmsbError("read-out: give nodes or rows, not both")
            if not torch.is_tensor(nodes):
                nodes = self.ctx.from_numpy(np.ascontiguousarray(nodes, dtype=np.uint32))
            if nodes.dtype != torch.int32 or not nodes.is_contiguous():
                raise AmmsbError("read-out: nodes must be a contiguous int32 (uint32 bits) device tensor")
            lo, n = 0, int(nodes.numel())
        else:
            lo, hi = (0, pi.rows) if rows is None else (int(rows[0]), int(rows[1]))
            if not 0 <= lo <= hi <= pi.rows:
                raise AmmsbError("read-out: rows (%d, %d) outside 0..%d" % (lo, hi, pi.rows))
            n = hi - lo
        if sizes is not None and (sizes.dtype != torch.int64 or sizes.numel() != pi.cols or not sizes.is_contiguous()):
            raise AmmsbError("read-out: sizes must be a contiguous [K] int64 device tensor")
        ids = self.ctx.empty((n, T), torch.int32)
        weights = self.ctx.empty((n, T), torch.float32)
        count = self.ctx.empty((n,), torch.int32)
        self.ro.check(self.lib.ammsb_readout_top(C.byref(pi.desc), _ptr(nodes), lo, n, T, thr, _ptr(ids),
                                                 _ptr(weights), _ptr(count), _ptr(sizes), _stream()))
        return ids, weights, count

    def sizes(self, pi, thr, out=None):
        """-> [K] int64: rows of pi with pi[a, k] >= thr (one pass, nothing else written)."""
        _, thr = self.ro.check_args(1, thr)
        out = self.ctx.zeros((pi.cols,), torch.int64) if out is None else out
        self.ro.check(self.lib.ammsb_readout_top(C.byref(pi.desc), None, 0, pi.rows, 1, thr, None, None, None,
                                                 _ptr(out), _stream()))
        return out

    def kernel_name(self):
        return self.ro.last_kernel_name()


class LinkPredictor:
    """Link probabilities from a fitted (pi, beta) (include/ammsb_linkpred.h): p(a, b) = eps + sum_k pi_ak pi_bk
    (beta_k - eps) as a dense block, as the T best candidates per query, or per pair of a list.  Owns the workspace of
    `top` (the partial lists of the blocks), which only ever grows: reserve() it outside a timed path.  Ids come back as
    int32, so the empty slot 0xFFFFFFFF reads -1."""

    def __init__(self, ctx):
        from . import _linkpred
        self.ctx = ctx
        self.lp = _linkpred
        self.lib = _linkpred.load()
        self.workspace = None

    def _nodes(self, nodes):
        return _u32_vector(self.ctx, nodes, "link prediction: nodes")

    def _range(self, pi, cand):
        lo, hi = (0, pi.rows) if cand is None else (int(cand[0]), int(cand[1]))
        if not 0 <= lo <= hi <= pi.rows:
            raise AmmsbError("link prediction: candidates (%d, %d) outside 0..%d" % (lo, hi, pi.rows))
        return lo, hi - lo

    def workspace_bytes(self, Q, T, cand_n, K):
        return int(self.lib.ammsb_linkpred_top_workspace_bytes(int(Q), int(T), int(cand_n), int(K)))

    def reserve(self, nbytes):
        """Grow the workspace to nbytes (torch's allocator: not for a timed path)."""
        if self.workspace is None or self.workspace.numel() < nbytes:
            self.workspace = self.ctx.empty((int(nbytes),), torch.uint8)
        return self.workspace

    def block(self, pi, beta, epsilon, nodes, cand=None):
        """-> [Q, n] float32: p(nodes[i], lo + j) for the candidate rows cand = (lo, hi) of pi (default: all)."""
        nodes = self._nodes(nodes)
        lo, n = self._range(pi, cand)
        out = self.ctx.empty((int(nodes.numel()), n), torch.float32)
        self.lp.check(self.lib.ammsb_linkpred_block(C.byref(pi.desc), _ptr(beta), float(epsilon), _ptr(nodes),
                                                    int(nodes.numel()), lo, n, _ptr(out), _stream()))
        return out

    def top(self, pi, beta, epsilon, nodes, T, exclude=(), cand=None):
        """-> (ids [Q, T] int32, scores [Q, T] float32): per query its T most probable candidates that are not the
        query itself and whose pair is in none of the DeviceSets `exclude` (at most two); score descending, equal
        scores by id ascending; -1 / 0 in the slots past the eligible candidates."""
        T = self.lp.check_top(T)
        nodes = self._nodes(nodes)
        lo, n = self._range(pi, cand)
        exclude = [s for s in exclude if s is not None]
        if len(exclude) > 2:
            raise AmmsbError("link prediction: at most two exclusion sets")
        ex = [C.byref(s.desc) for s in exclude] + [None, None]
        Q = int(nodes.numel())
        nbytes = self.workspace_bytes(Q, T, n, pi.cols)
        ws = self.reserve(nbytes)
        ids, scores = self.ctx.empty((Q, T), torch.int32), self.ctx.empty((Q, T), torch.float32)
        self.lp.check(self.lib.ammsb_linkpred_top(C.byref(pi.desc), _ptr(beta), float(epsilon), _ptr(nodes), Q, T,
                                                  ex[0], ex[1], lo, n, _ptr(ids), _ptr(scores), _ptr(ws), nbytes,
                                                  _stream()))
        return ids, scores

    def pairs(self, pi, beta, epsilon, edges):
        """-> [n] float32: p(a, b) per edge key (a << 32 | b, either order of the ends); -1 for an end >= N."""
        edges = _edge_keys(self.ctx, edges, "link prediction")
        out = self.ctx.empty((int(edges.numel()),), torch.float32)
        self.lp.check(self.lib.ammsb_linkpred_pairs(C.byref(pi.desc), _ptr(beta), float(epsilon), _ptr(edges),
                                                    int(edges.numel()), _ptr(out), _stream()))
        return out

    def kernel_name(self):
        return self.lp.last_kernel_name()


class LinkCommunities:
    """The communities that explain a link (include/ammsb_linkcomm.h): per edge key the T largest terms
    (pi[a,k] * pi[b,k]) * beta_k with their communities (term descending, equal terms by community ascending), the
    link's probability, and per community the number of edges whose largest term it holds.  Exact: ids and terms are
    the stable argsort of the float32 statement.  Owns nothing but the tensors it returns; ids come back as int32, so
    the empty slot 0xFFFFFFFF reads -1."""

    def __init__(self, ctx):
        from . import _linkcomm
        self.ctx = ctx
        self.lc = _linkcomm
        self.lib = _linkcomm.load()

    def _edges(self, edges):
        return _edge_keys(self.ctx, edges, "link communities")

    def _sizes(self, pi, sizes):
        if sizes is not None and (sizes.dtype != torch.int64 or sizes.numel() != pi.cols + 1
                                  or not sizes.is_contiguous()):
            raise AmmsbError("link communities: sizes must be a contiguous [K + 1] int64 device tensor")
        return sizes

    def edges(self, pi, beta, epsilon, edges, top, min_term=0.0, sizes=None):
        """-> (ids [n, top] int32, terms [n, top] float32, prob [n] float32) on the device.  sizes: a [K + 1] int64
        device tensor to accumulate into (the caller zeroes it): sizes[k] counts the edges whose slot 0 holds k,
        sizes[K] the edges with valid ends and no term >= min_term."""
        top, min_term = self.lc.check_args(top, min_term)
        edges = self._edges(edges)
        sizes = self._sizes(pi, sizes)
        n = int(edges.numel())
        ids, terms = self.ctx.empty((n, top), torch.int32), self.ctx.empty((n, top), torch.float32)
        prob = self.ctx.empty((n,), torch.float32)
        if n == 0:  # a valid no-op; the empty tensors have no address, which the library would read as "no output"
            return ids, terms, prob
        self.lc.check(self.lib.ammsb_linkcomm_edges(C.byref(pi.desc), _ptr(beta), float(epsilon), _ptr(edges), n, top,
                                                    min_term, _ptr(ids), _ptr(terms), _ptr(prob), _ptr(sizes),
                                                    _stream()))
        return ids, terms, prob

    def sizes(self, pi, beta, epsilon, edges, min_term=0.0, out=None):
        """-> [K + 1] int64: the sizes-only pass (nothing else is written)."""
        _, min_term = self.lc.check_args(1, min_term)
        edges = self._edges(edges)
        out = self.ctx.zeros((pi.cols + 1,), torch.int64) if out is None else self._sizes(pi, out)
        self.lc.check(self.lib.ammsb_linkcomm_edges(C.byref(pi.desc), _ptr(beta), float(epsilon), _ptr(edges),
                                                    int(edges.numel()), 1, min_term, None, None, None, _ptr(out),
                                                    _stream()))
        return out

    def kernel_name(self):
        return self.lc.last_kernel_name()


class CommunityQuality:
    """Scoring communities against a graph (include/ammsb_quality.h): one membership bit per (node, community) from one
    streaming pass over pi, then per edge of a list two rows of bits: per community the edges inside it and the edges
    that leave it, the edges no community covers, and per edge the communities its ends share.  Integer counts over
    binary32 compares: exact.  Owns nothing but the tensors it returns."""

    def __init__(self, ctx):
        from . import _quality
        self.ctx = ctx
        self.q = _quality
        self.lib = _quality.load()

    def mask(self, pi, thr):
        """-> the membership bits of (pi, thr): an opaque int64 device tensor for edges() (its layout is the library's)"""
        thr = self.q.check_threshold(thr)
        words = int(self.lib.ammsb_quality_mask_bytes(pi.desc.num_rows, pi.cols)) // 8
        if words == 0:
            raise AmmsbError("community quality: no mask for a %d x %d pi" % (pi.desc.num_rows, pi.cols))
        out = self.ctx.empty((words,), torch.int64)
        self.q.check(self.lib.ammsb_quality_mask(C.byref(pi.desc), thr, _ptr(out), _stream()))
        return out

    def edges(self, mask, N, K, edges, shared=False, counts=True):
        """mask: what mask() returned for an N x K pi; edges: keys (a << 32) | b, a host array or a contiguous 1-d int64
        (uint64 bits) device tensor.  -> counts [2K + 2] int64 on the device (internal[0..K), boundary[K..2K),
        uncovered, skipped), or (counts, shared [n] int32) with shared=True; counts=False leaves the counters out
        (-> None in their place)."""
        edges = _edge_keys(self.ctx, edges, "community quality")
        N, K, n = int(N), int(K), int(edges.numel())
        if mask.dtype != torch.int64 or not mask.is_contiguous() or \
                not mask.numel() or mask.numel() * 8 != int(self.lib.ammsb_quality_mask_bytes(N, K)):
            raise AmmsbError("community quality: not the mask of a %d x %d pi" % (N, K))
        if not counts and not shared:
            raise AmmsbError("community quality: no output asked for")
        cnt = self.ctx.zeros((2 * K + 2,), torch.int64) if counts else None
        sh = self.ctx.empty((n,), torch.int32) if shared else None
        if n:  # (an empty list is a valid no-op; its empty tensors have no address)
            self.q.check(self.lib.ammsb_quality_edges(_ptr(mask), N, K, _ptr(edges), n, _ptr(cnt), _ptr(sh), _stream()))
        return (cnt, sh) if shared else cnt

    def kernel_name(self):
        return self.q.last_kernel_name()


class CoverMatch:
    """Matching the detected cover to a ground-truth cover (include/ammsb_cover.h): per ground-truth community the
    detected community of the best F1 and per detected community the ground-truth one, from one gather pass over the
    rows of pi that the members name.  Integer counts over binary32 compares and integer compares of rationals: exact.
    Owns its workspace, which only ever grows: reserve() it outside a timed path."""

    def __init__(self, ctx):
        from . import _cover
        self.ctx = ctx
        self.cv = _cover
        self.lib = _cover.load()
        self.workspace = None

    def workspace_bytes(self, M, K):
        return int(self.lib.ammsb_cover_workspace_bytes(int(M), int(K)))

    def reserve(self, nbytes):
        """Grow the workspace to nbytes (torch's allocator: not for a timed path)."""
        if self.workspace is None or self.workspace.numel() * 8 < nbytes:
            self.workspace = self.ctx.empty(((int(nbytes) + 7) // 8,), torch.int64)
        return self.workspace

    def match(self, pi, threshold, offsets, members, detected_size, dense=False):
        """offsets [G + 1] (uint64 bits) and members [M] (uint32 bits): host arrays or contiguous int64 / int32 device
        tensors; detected_size: the [K] int64 device tensor CommunityReadout.sizes gives at the same threshold.
        -> (truth_best [G] int32, truth_overlap [G] int32, truth_size [G] int32, detected_best [K] int32,
        detected_overlap [K] int32, skipped [1] int64, overlap [G, K] int32 or None) on the device; the uint32 outputs
        come back as int32 bits.  With nothing to compare (G == 0 or M == 0) every community is unmatched."""
        thr = self.cv.check_threshold(threshold)
        if not torch.is_tensor(offsets):
            offsets = self.ctx.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1))
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise AmmsbError("cover match: offsets must be a contiguous 1-d int64 (uint64 bits) device tensor [G + 1]")
        members = _u32_vector(self.ctx, members, "cover match: members")
        if detected_size.dtype != torch.int64 or detected_size.numel() != pi.cols or not detected_size.is_contiguous():
            raise AmmsbError("cover match: detected_size must be a contiguous [K] int64 device tensor")
        G, M, K = int(offsets.numel()) - 1, int(members.numel()), int(pi.cols)
        c = self.ctx
        tb, to, ts = c.empty((G,), torch.int32).fill_(-1), c.zeros((G,), torch.int32), c.zeros((G,), torch.int32)
        db, do = c.empty((K,), torch.int32).fill_(-1), c.zeros((K,), torch.int32)
        sk = c.zeros((1,), torch.int64)
        ov = c.zeros((G, K), torch.int32) if dense else None
        if G and M:  # (with nothing to compare the library launches nothing: the presets stand)
            nbytes = self.workspace_bytes(M, K)
            if nbytes == 0:
                raise AmmsbError("cover match: no workspace for %d members against %d communities" % (M, K))
            ws = self.reserve(nbytes)
            self.cv.check(self.lib.ammsb_cover_match(C.byref(pi.desc), thr, _ptr(offsets), G, _ptr(members), M,
                                                     _ptr(detected_size), _ptr(tb), _ptr(to), _ptr(ts), _ptr(db),
                                                     _ptr(do), _ptr(sk), _ptr(ov), _ptr(ws), ws.numel() * 8,
                                                     _stream()))
        return tb, to, ts, db, do, sk, ov

    def kernel_name(self):
        return self.cv.last_kernel_name()


class CoverNMI:
    """The pair pass of the overlapping NMI (include/ammsb_nmi.h): begin() writes the entropies of both covers and
    presets the running minima, accumulate() folds one slab of the dense overlap that CoverMatch.match(dense=True)
    gives for a slice of the ground truth.  float64 from the device; a minimum does not depend on the order of arrival,
    so the results do not depend on the slabs.  Owns nothing but the tensors it returns."""

    class State:
        """the arrays of one comparison, on the device"""

        def __init__(self, N, truth_size, detected_size, H_truth, H_detected, c_truth, c_detected):
            self.N, self.truth_size, self.detected_size = N, truth_size, detected_size
            self.H_truth, self.H_detected, self.c_truth, self.c_detected = H_truth, H_detected, c_truth, c_detected

    def __init__(self, ctx):
        from . import _nmi
        self.ctx = ctx
        self.nm = _nmi
        self.lib = _nmi.load()

    def begin(self, N, truth_size, detected_size):
        """truth_size [G] (uint32 bits): a host array or a contiguous int32 device tensor; detected_size: the [K] int64
        device tensor CommunityReadout.sizes gives.  -> State: H_truth [G], H_detected [K] written, c_truth [G] and
        c_detected [K] at +inf."""
        truth_size = _u32_vector(self.ctx, truth_size, "cover NMI: truth_size")
        if detected_size.dtype != torch.int64 or detected_size.dim() != 1 or not detected_size.is_contiguous():
            raise AmmsbError("cover NMI: detected_size must be a contiguous [K] int64 device tensor")
        G, K, c = int(truth_size.numel()), int(detected_size.numel()), self.ctx
        st = self.State(int(N), truth_size, detected_size, c.empty((G,), torch.float64), c.empty((K,), torch.float64),
                        c.empty((G,), torch.float64), c.empty((K,), torch.float64))
        self.nm.check(self.lib.ammsb_nmi_begin(st.N, _ptr(truth_size), G, _ptr(detected_size), K, _ptr(st.H_truth),
                                               _ptr(st.H_detected), _ptr(st.c_truth), _ptr(st.c_detected), _stream()))
        return st

    def accumulate(self, st, overlap, g0):
        """overlap: the [Gs, K] int32 (uint32 bits) device tensor of rows g0 .. g0 + Gs - 1"""
        K = int(st.detected_size.numel())
        if overlap.dtype != torch.int32 or overlap.dim() != 2 or int(overlap.shape[1]) != K or not overlap.is_contiguous():
            raise AmmsbError("cover NMI: overlap must be a contiguous [Gs, K] int32 (uint32 bits) device tensor")
        Gs = int(overlap.shape[0])
        if Gs == 0:  # (an empty tensor has no address)
            return
        self.nm.check(self.lib.ammsb_nmi_accumulate(_ptr(overlap), int(g0), Gs, st.N, _ptr(st.truth_size),
                                                    int(st.truth_size.numel()), _ptr(st.detected_size), K,
                                                    _ptr(st.H_truth), _ptr(st.H_detected), _ptr(st.c_truth),
                                                    _ptr(st.c_detected), _stream()))

    def kernel_name(self):
        return self.nm.last_kernel_name()


class CoverOmega:
    """The node-pair pass of the Omega index (include/ammsb_omega.h): bit rows of both covers over a universe of nodes,
    then per pair of positions the communities shared in each cover, as three histograms.  Integer counts over binary32
    compares: exact, and independent of how the tile range is cut into launches.  Owns nothing but the tensors it
    returns."""

    def __init__(self, ctx):
        from . import _omega
        self.ctx = ctx
        self.om = _omega
        self.lib = _omega.load()

    def detected_bits(self, pi, thr, nodes=None, n=None):
        """nodes: [n] int32 (uint32 bits) device tensor, or None for rows 0 .. n - 1 -> (bits [n, ceil(K / 32)] int32,
        counts [n] int32) on the device"""
        n = int(nodes.numel()) if nodes is not None else int(pi.desc.num_rows if n is None else n)
        W = (int(pi.cols) + 31) // 32
        bits, counts = self.ctx.empty((n, W), torch.int32), self.ctx.empty((n,), torch.int32)
        if n:  # (an empty tensor has no address)
            self.om.check(self.lib.ammsb_omega_detected_bits(C.byref(pi.desc), float(thr), _ptr(nodes), n, _ptr(bits),
                                                             _ptr(counts), _stream()))
        return bits, counts

    def truth_bits(self, offsets, members, N, position, n):
        """offsets [G + 1] int64 (uint64 bits), members [M] int32 (uint32 bits), position [N] int32: device tensors
        -> (bits [n, ceil(G / 32)] int32, counts [n] int32, tally [2] int64 = skipped, outside) on the device"""
        G, M, n = int(offsets.numel()) - 1, int(members.numel()), int(n)
        if G > self.om.MAX_TRUTH:
            raise AmmsbError("cover omega: %d ground-truth communities; the bit rows hold at most %d (a sparse "
                             "representation of the ground truth is not built)" % (G, self.om.MAX_TRUTH))
        c = self.ctx
        bits, counts = c.zeros((n, (G + 31) // 32), torch.int32), c.zeros((n,), torch.int32)
        tally = c.zeros((2,), torch.int64)
        if n and G:
            self.om.check(self.lib.ammsb_omega_truth_bits(_ptr(offsets), G, _ptr(members) if M else None, M, int(N),
                                                          _ptr(position), n, _ptr(bits), _ptr(counts), _ptr(tally),
                                                          C.c_void_p(tally.data_ptr() + 8), _stream()))
        return bits, counts, tally

    def pairs(self, dbits, K, tbits, G, n, L, hist, tile_begin, tile_count):
        """adds tiles tile_begin .. tile_begin + tile_count - 1 to hist [3 L + 1] int64"""
        if hist.dtype != torch.int64 or hist.numel() != 3 * int(L) + 1 or not hist.is_contiguous():
            raise AmmsbError("cover omega: hist must be a contiguous [3 L + 1] int64 device tensor")
        if int(n) == 0 or int(tile_count) == 0:
            return
        self.om.check(self.lib.ammsb_omega_pairs(_ptr(dbits), int(K), _ptr(tbits) if int(G) else None, int(G), int(n),
                                                 int(L), int(tile_begin), int(tile_count), _ptr(hist), _stream()))

    def kernel_name(self):
        return self.om.last_kernel_name()


class CommunityRelations:
    """How the detected communities relate to each other (include/ammsb_relate.h): community-major membership bits from
    one streaming pass over a slab of pi, the K x K matrix of shared nodes by AND + population count over those bits,
    and per community the partners it overlaps most.  Integer counts over binary32 compares and integer compares of
    rationals: exact, and independent of how the nodes are cut into slabs.  Owns nothing but the tensors it returns."""

    def __init__(self, ctx):
        from . import _relate
        self.ctx = ctx
        self.rl = _relate
        self.lib = _relate.load()

    def bits(self, pi, thr, rows=None):
        """rows: (lo, hi) with lo a multiple of 64, default all of pi -> the bits of rows lo .. hi - 1: a [K, ceil((hi -
        lo) / 64)] int64 device tensor, bit (a - lo) & 63 of word (a - lo) >> 6 of row k set iff pi[a, k] >= thr"""
        thr = self.rl.check_threshold(thr)
        lo, hi = (0, int(pi.desc.num_rows)) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi:
            raise AmmsbError("community relations: rows (%d, %d) is not a range" % (lo, hi))
        K, n = int(pi.cols), hi - lo
        out = self.ctx.empty((K, (n + 63) // 64), torch.int64)
        if n:  # (an empty tensor has no address)
            self.rl.check(self.lib.ammsb_relate_bits(C.byref(pi.desc), thr, lo, n, _ptr(out), _stream()))
        return out

    def pairs(self, bits, K, rows, overlap):
        """adds the shared nodes of one slab -- bits as bits() gives them for `rows` rows -- to overlap, a [K, K] int32
        (uint32 bits) device tensor that the caller zeroed before the first slab"""
        K, rows = int(K), int(rows)
        if bits.dtype != torch.int64 or not bits.is_contiguous() or bits.numel() != K * ((rows + 63) // 64):
            raise AmmsbError("community relations: not the bits of %d rows and %d communities" % (rows, K))
        if overlap.dtype != torch.int32 or not overlap.is_contiguous() or tuple(overlap.shape) != (K, K):
            raise AmmsbError("community relations: overlap must be a contiguous [K, K] int32 (uint32 bits) device tensor")
        if rows:
            self.rl.check(self.lib.ammsb_relate_pairs(_ptr(bits), K, rows, _ptr(overlap), _stream()))

    def top(self, overlap, by="jaccard", top=4, min_overlap=1):
        """overlap: the finished [K, K] int32 (uint32 bits) device tensor -> (partner [K, top] int32, shared [K, top]
        int32 (uint32 bits)) on the device: per community the `top` others that share at least max(1, min_overlap) nodes
        with it, ranked by `by` (overlap, jaccard or contained), equal values by id ascending; -1 and 0 in empty slots"""
        measure, top, min_overlap = self.rl.check_args(by, top, min_overlap)
        if overlap.dtype != torch.int32 or not overlap.is_contiguous() or overlap.dim() != 2 or \
                overlap.shape[0] != overlap.shape[1] or not overlap.numel():
            raise AmmsbError("community relations: overlap must be a contiguous [K, K] int32 (uint32 bits) device tensor")
        K = int(overlap.shape[0])
        partner, shared = self.ctx.empty((K, top), torch.int32), self.ctx.empty((K, top), torch.int32)
        self.rl.check(self.lib.ammsb_relate_top(_ptr(overlap), K, measure, top, min_overlap, _ptr(partner), _ptr(shared),
                                                _stream()))
        return partner, shared

    def kernel_name(self):
        return self.rl.last_kernel_name()


class CommunityLinks:
    """How the detected communities are linked to each other (include/ammsb_connect.h): node-major membership bits in
    community order from one streaming pass over pi, the K x K matrix of the links of an edge list between every two
    communities by walking the two bit rows of every edge, and per community the partners it is linked to most.  Integer
    counts over binary32 compares and integer compares of rationals: exact, and independent of the kernel form and of how
    the edge list is cut into calls.  Owns nothing but the tensors it returns."""

    def __init__(self, ctx):
        from . import _connect
        self.ctx = ctx
        self.cn = _connect
        self.lib = _connect.load()

    def mask(self, pi, thr):
        """-> the membership bits of (pi, thr): a [N, ceil(K / 64)] int64 device tensor, bit k & 63 of word k >> 6 of row
        a set iff pi[a, k] >= thr"""
        thr = self.cn.check_threshold(thr)
        N, K = int(pi.desc.num_rows), int(pi.cols)
        if N and not int(self.lib.ammsb_connect_mask_bytes(N, K)):
            raise AmmsbError("community links: no mask for a %d x %d pi" % (N, K))
        out = self.ctx.empty((N, (K + 63) // 64), torch.int64)
        if N:  # (an empty tensor has no address)
            self.cn.check(self.lib.ammsb_connect_mask(C.byref(pi.desc), thr, _ptr(out), _stream()))
        return out

    def edges(self, mask, N, K, edges, directed=None, counts=None):
        """mask: what mask() returned for an N x K pi; edges: keys (a << 32) | b, a host array or a contiguous 1-d int64
        (uint64 bits) device tensor.  Adds them to directed, a [K, K] int64 (uint64 bits) device tensor, and to counts
        [2] int64 (valid, skipped); either is made and zeroed where none is given -> (directed, counts)"""
        edges = _edge_keys(self.ctx, edges, "community links")
        N, K, n = int(N), int(K), int(edges.numel())
        _check_mask(mask, N, K, "community links")
        directed = self.ctx.zeros((K, K), torch.int64) if directed is None else directed
        counts = self.ctx.zeros((2,), torch.int64) if counts is None else counts
        if directed.dtype != torch.int64 or not directed.is_contiguous() or tuple(directed.shape) != (K, K):
            raise AmmsbError("community links: directed must be a contiguous [K, K] int64 (uint64 bits) device tensor")
        if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.numel() != 2:
            raise AmmsbError("community links: counts must be a contiguous [2] int64 device tensor")
        if n:  # (an empty list is a valid no-op; its empty tensor has no address)
            self.cn.check(self.lib.ammsb_connect_edges(_ptr(mask), N, K, _ptr(edges), n, _ptr(directed), _ptr(counts),
                                                       _stream()))
        return directed, counts

    def finish(self, directed):
        """-> links [K, K] int64 (uint64 bits) = directed + its transpose"""
        if directed.dtype != torch.int64 or not directed.is_contiguous() or directed.dim() != 2 or \
                directed.shape[0] != directed.shape[1] or not directed.numel():
            raise AmmsbError("community links: directed must be a contiguous [K, K] int64 (uint64 bits) device tensor")
        links = self.ctx.empty(tuple(directed.shape), torch.int64)
        self.cn.check(self.lib.ammsb_connect_finish(_ptr(directed), int(directed.shape[0]), _ptr(links), _stream()))
        return links

    def top(self, links, overlap, by="density", top=4, min_links=1):
        """links: the finished [K, K] int64 device tensor; overlap: CommunityRelations' finished [K, K] int32 (uint32 bits)
        -> (partner [K, top] int32, plinks [K, top] int64 (uint64 bits), pshared [K, top] int32 (uint32 bits)) on the
        device: per community the `top` others with at least max(1, min_links) links to it, ranked by `by` (links or
        density), equal values by id ascending; -1, 0 and 0 in empty slots"""
        measure, top, min_links = self.cn.check_args(by, top, min_links)
        if links.dtype != torch.int64 or not links.is_contiguous() or links.dim() != 2 or \
                links.shape[0] != links.shape[1] or not links.numel():
            raise AmmsbError("community links: links must be a contiguous [K, K] int64 (uint64 bits) device tensor")
        if overlap.dtype != torch.int32 or not overlap.is_contiguous() or tuple(overlap.shape) != tuple(links.shape):
            raise AmmsbError("community links: overlap must be a contiguous [K, K] int32 (uint32 bits) device tensor")
        K = int(links.shape[0])
        partner, pshared = self.ctx.empty((K, top), torch.int32), self.ctx.empty((K, top), torch.int32)
        plinks = self.ctx.empty((K, top), torch.int64)
        self.cn.check(self.lib.ammsb_connect_top(_ptr(links), _ptr(overlap), K, measure, top, min_links, _ptr(partner),
                                                 _ptr(plinks), _ptr(pshared), _stream()))
        return partner, plinks, pshared

    def kernel_name(self):
        return self.cn.last_kernel_name()


class Modularity:
    """The overlapping modularity of the detected cover (include/ammsb_modularity.h): over CommunityLinks' node-major
    membership bits, an edge pass that adds floor(2^62 / (O_a O_b)) per community that holds both ends of an edge and
    counts the degrees, and a node pass that adds deg[a] floor(2^62 / O_a) per membership, both into 128-bit integers
    (two int64 words each, uint64 bits: low, high).  Integer adds: exact, and independent of the kernel form and of how
    the edge list is cut into calls.  Owns nothing but the tensors it returns."""

    def __init__(self, ctx):
        from . import _modularity
        self.ctx = ctx
        self.md = _modularity
        self.lib = _modularity.load()
        self.links = CommunityLinks(ctx)

    def edges(self, mask, N, K, edges, state=None):
        """mask: what CommunityLinks.mask() returned for an N x K pi; edges: keys (a << 32) | b, a host array or a
        contiguous 1-d int64 (uint64 bits) device tensor, fewer than 2^31.  Adds them to state = (degree [N] int32 (uint32
        bits), internal [2 K] int64, counts [2] int64 (valid, skipped)), which is made and zeroed where none is given
        -> state"""
        edges = _edge_keys(self.ctx, edges, "modularity")
        N, K, n = int(N), int(K), self.md.check_keys(edges.numel())
        _check_mask(mask, N, K, "modularity")
        if state is None:
            state = (self.ctx.zeros((N,), torch.int32), self.ctx.zeros((2 * K,), torch.int64), self.ctx.zeros((2,), torch.int64))
        degree, internal, counts = state
        if degree.dtype != torch.int32 or not degree.is_contiguous() or degree.numel() != N:
            raise AmmsbError("modularity: degree must be a contiguous [N] int32 (uint32 bits) device tensor")
        if internal.dtype != torch.int64 or not internal.is_contiguous() or internal.numel() != 2 * K:
            raise AmmsbError("modularity: internal must be a contiguous [2 K] int64 (uint64 bits) device tensor")
        if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.numel() != 2:
            raise AmmsbError("modularity: counts must be a contiguous [2] int64 device tensor")
        if n:  # (an empty list is a valid no-op; its empty tensor has no address)
            self.md.check(self.lib.ammsb_modularity_edges(_ptr(mask), N, K, _ptr(edges), n, _ptr(degree), _ptr(internal),
                                                          _ptr(counts), _stream()))
        return state

    def nodes(self, mask, N, K, degree):
        """after the last edges(): -> volume [2 K] int64 (uint64 bits)"""
        N, K = int(N), int(K)
        _check_mask(mask, N, K, "modularity")
        if degree.dtype != torch.int32 or not degree.is_contiguous() or degree.numel() != N:
            raise AmmsbError("modularity: degree must be a contiguous [N] int32 (uint32 bits) device tensor")
        volume = self.ctx.zeros((2 * K,), torch.int64)
        if N:
            self.md.check(self.lib.ammsb_modularity_nodes(_ptr(mask), N, K, _ptr(degree), _ptr(volume), _stream()))
        return volume

    def run(self, pi, thr, edges):
        """-> (internal [2 K], volume [2 K], counts [2], degree [N]) device tensors for the cover (pi, thr) and the edge
        list"""
        N, K = int(pi.desc.num_rows), int(pi.cols)
        mask = self.links.mask(pi, self.md.check_threshold(thr))
        degree, internal, counts = self.edges(mask, N, K, edges)
        return internal, self.nodes(mask, N, K, degree), counts, degree

    def kernel_name(self):
        return self.md.last_kernel_name()


class NodeRoles:
    """How a single node sits in the detected cover (include/ammsb_roles.h): over CommunityLinks' node-major membership
    bits and a CSR adjacency, a wave per node counts the node's neighbours per community in LDS and reduces them to the
    node's degree, embedded, reached, votes, squares and top slots, and to the per-community sums ksum, ksq, kmembers.
    Integer adds and compares: exact, and independent of the kernel form and of how the node range is cut into calls.
    Owns nothing but the tensors it returns."""

    PER_NODE = (("degree", torch.int32), ("own", torch.int32), ("embedded", torch.int32), ("reached", torch.int32),
                ("votes", torch.int64), ("squares", torch.int64))
    PER_COMMUNITY = ("ksum", "ksq", "kmembers")

    def __init__(self, ctx):
        from . import _roles
        self.ctx = ctx
        self.rl = _roles
        self.lib = _roles.load()
        self.links = CommunityLinks(ctx)

    def state(self, N, K, top):
        """-> the zeroed outputs of nodes() for an N x K pi: name -> device tensor (uint32 as int32, uint64 as int64);
        degree, own, embedded, reached, votes, squares [N]; home, hcount [N, top] and hflags [N] where top > 0; ksum, ksq,
        kmembers [K]; counts [2] (valid, skipped)"""
        out = {name: self.ctx.zeros((N,), dtype) for name, dtype in self.PER_NODE}
        if top:
            out["home"], out["hcount"] = self.ctx.zeros((N, top), torch.int32), self.ctx.zeros((N, top), torch.int32)
            out["hflags"] = self.ctx.zeros((N,), torch.int32)
        for name in self.PER_COMMUNITY:
            out[name] = self.ctx.zeros((K,), torch.int64)
        out["counts"] = self.ctx.zeros((2,), torch.int64)
        return out

    def nodes(self, mask, N, K, offsets, targets, first=0, count=None, among="all", top=4, min_count=0, state=None):
        """mask: what CommunityLinks.mask() returned for an N x K pi; offsets [N + 1] int64 (uint64 bits) and targets int32
        (uint32 bits): contiguous device tensors, the CSR of the header.  Handles the nodes first .. first + count - 1
        (default: through N - 1) into `state`, which is made and zeroed where none is given; calls over disjoint ranges
        fill one state.  top = 0 skips the selection -> state"""
        N, K, top = int(N), int(K), int(top)
        first, count = self.rl.check_nodes((first, N - int(first) if count is None else count), N)
        code, min_count = self.rl.check_among(among), self.rl.check_min_count(min_count)
        if top:
            self.rl.check_top(top)
        _check_mask(mask, N, K, "node roles")
        if offsets.dtype != torch.int64 or not offsets.is_contiguous() or offsets.numel() != N + 1:
            raise AmmsbError("node roles: offsets must be a contiguous [N + 1] int64 (uint64 bits) device tensor")
        if targets.dtype != torch.int32 or not targets.is_contiguous() or targets.dim() != 1:
            raise AmmsbError("node roles: targets must be a contiguous 1-d int32 (uint32 bits) device tensor")
        if state is None:
            state = self.state(N, K, top)
        for name, dtype in self.PER_NODE + ((("home", torch.int32), ("hcount", torch.int32), ("hflags", torch.int32)) if top else ()):
            t = state[name]
            if t.dtype != dtype or not t.is_contiguous() or t.numel() != N * (top if name in ("home", "hcount") else 1):
                raise AmmsbError("node roles: %s of the state does not fit N = %d, top = %d" % (name, N, top))
        for name in self.PER_COMMUNITY + ("counts",):
            t = state[name]
            if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != (2 if name == "counts" else K):
                raise AmmsbError("node roles: %s of the state does not fit K = %d" % (name, K))
        if count:  # (an empty range is a valid no-op; an empty tensor has no address)
            slot = [_ptr(state[n]) if top else None for n in ("home", "hcount", "hflags")]
            # an adjacency without a target still needs an address for `targets`: the offsets are read, no target is
            tgt = targets if targets.numel() else self.ctx.zeros((1,), torch.int32)
            self.rl.check(self.lib.ammsb_roles_nodes(
                _ptr(mask), N, K, _ptr(offsets), _ptr(tgt), first, count, code, top, min_count, _ptr(state["degree"]),
                _ptr(state["own"]), _ptr(state["embedded"]), _ptr(state["reached"]), _ptr(state["votes"]),
                _ptr(state["squares"]), slot[0], slot[1], slot[2], _ptr(state["ksum"]), _ptr(state["ksq"]),
                _ptr(state["kmembers"]), _ptr(state["counts"]), _stream()))
        return state

    def run(self, pi, thr, offsets, targets, **how):
        """-> the state of nodes() for the cover (pi, thr) and the CSR"""
        N, K = int(pi.desc.num_rows), int(pi.cols)
        return self.nodes(self.links.mask(pi, self.rl.check_threshold(thr)), N, K, offsets, targets, **how)

    def kernel_name(self):
        return self.rl.last_kernel_name()


class Triangles:
    """The triangles inside the detected communities (include/ammsb_triangles.h): over CommunityLinks' node-major
    membership bits and a simple CSR adjacency, a wave per node intersects the node's sorted row with its neighbours' rows
    and counts the node's triangles, those whose corners share a community, and per community the triangles inside it
    (three times) and the members that are a corner of one.  Integer adds and compares: exact, and independent of the
    kernel form and of how the node range is cut into calls.  Owns nothing but the tensors it returns."""

    PER_NODE = ("tri", "tri_in", "tri_comms")
    PER_COMMUNITY = ("ktri3", "kpart")

    def __init__(self, ctx):
        from . import _triangles
        self.ctx = ctx
        self.tr = _triangles
        self.lib = _triangles.load()
        self.links = CommunityLinks(ctx)

    def state(self, N, K):
        """-> the zeroed outputs of nodes() for an N x K pi: name -> device tensor (uint32 as int32, uint64 as int64); tri,
        tri_in, tri_comms [N]; ktri3, kpart [K]; counts [2] (the sum of tri, targets >= N)"""
        out = {name: self.ctx.zeros((N,), torch.int32) for name in self.PER_NODE}
        for name in self.PER_COMMUNITY:
            out[name] = self.ctx.zeros((K,), torch.int64)
        out["counts"] = self.ctx.zeros((2,), torch.int64)
        return out

    def verify(self, N, offsets, targets):
        """the rows are what the header asks of them, as far as a few statements can tell: offsets ascend inside
        targets, and every row is strictly ascending, holds no loop and no target >= N (symmetry is the caller's).  Waits
        for the answer -> the longest row"""
        if not N:
            return 0
        lengths = offsets[1:] - offsets[:-1]
        lo, hi = int(offsets[0]), int(offsets[-1])
        if lo < 0 or hi > targets.numel() or int(lengths.min()) < 0:
            raise AmmsbError("triangles: the offsets do not ascend inside the targets")
        t = targets[lo:hi].to(torch.int64) & 0xFFFFFFFF
        src = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=t.device), lengths)
        if bool((t >= N).any()):
            raise AmmsbError("triangles: a target is not below N = %d" % N)
        if bool((t == src).any()):
            raise AmmsbError("triangles: a row holds its own node")
        if bool(((src[1:] == src[:-1]) & (t[1:] <= t[:-1])).any()):
            raise AmmsbError("triangles: a row is not strictly ascending")
        return self.tr.check_rows(int(lengths.max()))

    def nodes(self, mask, N, K, offsets, targets, first=0, count=None, state=None):
        """mask: what CommunityLinks.mask() returned for an N x K pi; offsets [N + 1] int64 (uint64 bits) and targets int32
        (uint32 bits): contiguous device tensors, the simple CSR of the header, which is verified on the device before
        anything is launched.  Handles the nodes first .. first + count - 1 (default: through N - 1) into `state`, which is
        made and zeroed where none is given; calls over disjoint ranges fill one state -> state"""
        N, K = int(N), int(K)
        first, count = self.tr.check_nodes((first, N - int(first) if count is None else count), N)
        _check_mask(mask, N, K, "triangles")
        if offsets.dtype != torch.int64 or not offsets.is_contiguous() or offsets.numel() != N + 1:
            raise AmmsbError("triangles: offsets must be a contiguous [N + 1] int64 (uint64 bits) device tensor")
        if targets.dtype != torch.int32 or not targets.is_contiguous() or targets.dim() != 1:
            raise AmmsbError("triangles: targets must be a contiguous 1-d int32 (uint32 bits) device tensor")
        self.verify(N, offsets, targets)
        if state is None:
            state = self.state(N, K)
        for name in self.PER_NODE:
            t = state[name]
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != N:
                raise AmmsbError("triangles: %s of the state does not fit N = %d" % (name, N))
        for name in self.PER_COMMUNITY + ("counts",):
            t = state[name]
            if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != (2 if name == "counts" else K):
                raise AmmsbError("triangles: %s of the state does not fit K = %d" % (name, K))
        if count:  # (an empty range is a valid no-op; an empty tensor has no address)
            # an adjacency without a target still needs an address for `targets`: the offsets are read, no target is
            tgt = targets if targets.numel() else self.ctx.zeros((1,), torch.int32)
            self.tr.check(self.lib.ammsb_triangles_nodes(
                _ptr(mask), N, K, _ptr(offsets), _ptr(tgt), first, count, _ptr(state["tri"]), _ptr(state["tri_in"]),
                _ptr(state["tri_comms"]), _ptr(state["ktri3"]), _ptr(state["kpart"]), _ptr(state["counts"]), _stream()))
        return state

    def run(self, pi, thr, offsets, targets, first=0, count=None):
        """-> the state of nodes() for the cover (pi, thr) and the simple CSR"""
        N, K = int(pi.desc.num_rows), int(pi.cols)
        return self.nodes(self.links.mask(pi, self.tr.check_threshold(thr)), N, K, offsets, targets, first=first, count=count)

    def kernel_name(self):
        return self.tr.last_kernel_name()


class CommunityComponents:
    """The connected components of every detected community (include/ammsb_components.h): over CommunityLinks' node-major
    membership bits, the memberships are numbered ("slots": node by node, communities ascending), an edge pass unites the
    two slots of every community both ends of a key share in a lock-free union-find, and a finish pass reduces the forest
    to the root and size per slot, the counts per community and the stray memberships per node.  Integers that the
    partition alone determines: exact, and independent of the kernel form, the order of the keys and how the list is cut
    into calls.  Owns nothing but the tensors it returns."""

    PER_COMMUNITY = (("members", torch.int64), ("components", torch.int64), ("singletons", torch.int64), ("best", torch.int64),
                     ("largest", torch.int32), ("largest_root", torch.int32))
    PER_SLOT = (("slot_node", torch.int32), ("slot_comm", torch.int16), ("parent", torch.int32), ("root", torch.int32),
                ("size", torch.int32))

    def __init__(self, ctx):
        from . import _components
        self.ctx = ctx
        self.cc = _components
        self.lib = _components.load()
        self.links = CommunityLinks(ctx)

    def own(self, mask, N, K):
        """-> own [N] int32 (uint32 bits): the memberships of every node"""
        N, K = int(N), int(K)
        _check_mask(mask, N, K, "components")
        own = self.ctx.empty((N,), torch.int32)
        if N:
            self.cc.check(self.lib.ammsb_components_own(_ptr(mask), N, K, _ptr(own), _stream()))
        return own

    def base(self, own, threshold=None):
        """own -> (base [N + 1] int64, the exclusive prefix sum by a torch cumsum in int64, M = base[N]); waits for M and
        refuses M >= 2^32"""
        base = torch.zeros(own.numel() + 1, dtype=torch.int64, device=own.device)
        if own.numel():
            torch.cumsum(own.to(torch.int64) & 0xFFFFFFFF, 0, out=base[1:])
        return base, self.cc.check_slots(int(base[-1]), threshold)

    def state(self, N, K, M):
        """-> the buffers of one run for an N x K pi with M slots: name -> device tensor (uint32 as int32, uint16 as int16,
        uint64 as int64); slot_node, slot_comm, parent, root, size [M]; members, components, singletons, best, largest,
        largest_root [K]; stray [N]; counts [4] (valid, skipped, shared, give-ups).  What the library adds to is zeroed."""
        out = {name: self.ctx.empty((M,), dtype) for name, dtype in self.PER_SLOT}
        out.update({name: self.ctx.zeros((K,), dtype) for name, dtype in self.PER_COMMUNITY})
        out["stray"] = self.ctx.zeros((N,), torch.int32)
        out["counts"] = self.ctx.zeros((4,), torch.int64)
        return out

    def _check(self, mask, N, K, base, M, state):
        _check_mask(mask, N, K, "components")
        if base.dtype != torch.int64 or not base.is_contiguous() or base.numel() != N + 1:
            raise AmmsbError("components: base must be a contiguous [N + 1] int64 (uint64 bits) device tensor")
        for names, n in ((self.PER_SLOT, M), (self.PER_COMMUNITY, K), ((("stray", torch.int32),), N), ((("counts", torch.int64),), 4)):
            for name, dtype in names:
                t = state[name]
                if t.dtype != dtype or not t.is_contiguous() or t.numel() != n:
                    raise AmmsbError("components: %s of the state does not fit N = %d, K = %d, M = %d" % (name, N, K, M))

    def slots(self, mask, N, K, base, M, state, first=0, count=None):
        """numbers the slots of the nodes first .. first + count - 1 (default: through N - 1): slot_node, slot_comm and
        parent[s] = s of the state -> state"""
        N, K, M, first = int(N), int(K), self.cc.check_slots(M), int(first)
        count = N - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > N:
            raise AmmsbError("components: the nodes %d .. %d are not inside 0 .. %d" % (first, first + count, N))
        self._check(mask, N, K, base, M, state)
        if count and M:
            self.cc.check(self.lib.ammsb_components_slots(_ptr(mask), N, K, _ptr(base), M, first, count, _ptr(state["slot_node"]),
                                                          _ptr(state["slot_comm"]), _ptr(state["parent"]), _stream()))
        return state

    def edges(self, mask, N, K, base, M, edges, state):
        """edges: keys (a << 32) | b, a host array or a contiguous 1-d int64 (uint64 bits) device tensor, fewer than 2^31.
        Unites the slots they join in parent and adds to counts; any number of calls on pieces of the list -> state"""
        edges = _edge_keys(self.ctx, edges, "components")
        N, K, M, n = int(N), int(K), self.cc.check_slots(M), self.cc.check_keys(edges.numel())
        self._check(mask, N, K, base, M, state)
        if n:  # (an empty list is a valid no-op; its empty tensor has no address)
            self.cc.check(self.lib.ammsb_components_edges(_ptr(mask) if N else None, N, K, _ptr(base), M, _ptr(edges), n,
                                                          _ptr(state["parent"]) if M else None, _ptr(state["counts"]), _stream()))
        return state

    def finish(self, N, K, base, M, state):
        """after the last edges(): root and size per slot, the K-sized arrays and stray of the state -> state"""
        N, K, M = int(N), int(K), self.cc.check_slots(M)
        slot = lambda name: _ptr(state[name]) if M else None   # noqa: E731  (an empty tensor has no address)
        self.cc.check(self.lib.ammsb_components_finish(
            N, K, _ptr(base), M, slot("slot_node"), slot("slot_comm"), slot("parent"), slot("root"), slot("size"),
            _ptr(state["members"]), _ptr(state["components"]), _ptr(state["singletons"]), _ptr(state["best"]),
            _ptr(state["largest"]), _ptr(state["largest_root"]), _ptr(state["stray"]) if N else None, _ptr(state["counts"]),
            _stream()))
        return state

    def run(self, pi, thr, edges, mask=None):
        """-> (state, base, M) for the cover (pi, thr) and the edge list"""
        N, K = int(pi.desc.num_rows), int(pi.cols)
        thr = self.cc.check_threshold(thr)
        mask = self.links.mask(pi, thr) if mask is None else mask
        base, M = self.base(self.own(mask, N, K), thr)
        state = self.state(N, K, M)
        self.slots(mask, N, K, base, M, state)
        self.edges(mask, N, K, base, M, edges, state)
        return self.finish(N, K, base, M, state), base, M

    def kernel_name(self):
        return self.cc.last_kernel_name()


class CommunityCores:
    """The k-core decomposition of every detected community (include/ammsb_cores.h): over CommunityLinks' node-major
    membership bits, the slot numbering of CommunityComponents and a simple CSR adjacency, two passes build the induced slot
    graph (the inner degree of every membership, then its neighbours' slots in row order), a level-synchronous peel lowers
    the degrees to the core numbers -- one launch per sub-round, 12 bytes read back between launches, no lane ever waiting
    for another -- and a finish pass reduces them per community and per node.  Integers that the cover and the adjacency
    alone determine: exact, and independent of the kernel form, the order in which the queue fills and how the node range of
    the build passes is cut into calls.  Owns nothing but the tensors it returns."""

    PER_COMMUNITY = (("members", torch.int64), ("inlinks2", torch.int64), ("degeneracy", torch.int32), ("nucleus", torch.int64),
                     ("isolated", torch.int64))
    PER_NODE = (("best_core", torch.int32), ("best_comm", torch.int32), ("in_nucleus", torch.int32))

    def __init__(self, ctx):
        from . import _cores
        self.ctx = ctx
        self.co = _cores
        self.lib = _cores.load()
        self.comp = CommunityComponents(ctx)
        self.links = self.comp.links

    def _check(self, mask, N, K, base, M, offsets, targets):
        _check_mask(mask, N, K, "cores")
        if base.dtype != torch.int64 or not base.is_contiguous() or base.numel() != N + 1:
            raise AmmsbError("cores: base must be a contiguous [N + 1] int64 (uint64 bits) device tensor")
        if offsets.dtype != torch.int64 or not offsets.is_contiguous() or offsets.numel() != N + 1:
            raise AmmsbError("cores: offsets must be a contiguous [N + 1] int64 (uint64 bits) device tensor")
        if targets.dtype != torch.int32 or not targets.is_contiguous() or targets.dim() != 1:
            raise AmmsbError("cores: targets must be a contiguous 1-d int32 (uint32 bits) device tensor")
        if N and int(offsets[-1]) > targets.numel():
            raise AmmsbError("cores: the offsets end past the targets")

    @staticmethod
    def _range(N, first, count):
        first = int(first)
        count = N - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > N:
            raise AmmsbError("cores: the nodes %d .. %d are not inside 0 .. %d" % (first, first + count, N))
        return first, count

    def _per_slot(self, t, M, what):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != M:
            raise AmmsbError("cores: %s must be a contiguous [M] int32 (uint32 bits) device tensor" % what)

    def degrees(self, mask, N, K, base, M, offsets, targets, first=0, count=None, indeg=None, counts=None):
        """the inner degree of every slot of the nodes first .. first + count - 1 (default: through N - 1) into indeg [M]
        int32 (uint32 bits), and their slots and inner degrees added to counts [4] int64 (M, L, scans, rounds); either is made
        (indeg uninitialised, counts zeroed) where none is given; calls over disjoint ranges fill one indeg
        -> (indeg, counts)"""
        N, K, M = int(N), int(K), self.co.check_slots(M)
        first, count = self._range(N, first, count)
        self._check(mask, N, K, base, M, offsets, targets)
        indeg = self.ctx.empty((M,), torch.int32) if indeg is None else indeg
        counts = self.ctx.zeros((4,), torch.int64) if counts is None else counts
        self._per_slot(indeg, M, "indeg")
        if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.numel() != 4:
            raise AmmsbError("cores: counts must be a contiguous [4] int64 device tensor")
        if count and M:  # (an empty range is a valid no-op; an empty tensor has no address)
            tgt = targets if targets.numel() else self.ctx.zeros((1,), torch.int32)
            self.co.check(self.lib.ammsb_cores_degrees(_ptr(mask), N, K, _ptr(base), M, _ptr(offsets), _ptr(tgt), first, count,
                                                       _ptr(indeg), _ptr(counts), _stream()))
        return indeg, counts

    def offsets(self, indeg, max_bytes=None, threshold=None):
        """indeg -> (nbr_off [M + 1] int64, the exclusive prefix sum by a torch cumsum in int64, L = nbr_off[M]); waits for L
        and refuses L >= 2^32 or 4 L > max_bytes (default 4 GiB) before anything is allocated for nbr"""
        nbr_off = torch.zeros(indeg.numel() + 1, dtype=torch.int64, device=indeg.device)
        if indeg.numel():
            torch.cumsum(indeg.to(torch.int64) & 0xFFFFFFFF, 0, out=nbr_off[1:])
        return nbr_off, self.co.check_links(int(nbr_off[-1]), self.co.MAX_BYTES if max_bytes is None else max_bytes, threshold)

    def adjacency(self, mask, N, K, base, M, offsets, targets, indeg, nbr_off, L, first=0, count=None, nbr=None):
        """the rows of nbr [L] int32 (uint32 bits) of the nodes first .. first + count - 1 (default: through N - 1); nbr is
        made, uninitialised, where none is given -> nbr"""
        N, K, M, L = int(N), int(K), self.co.check_slots(M), int(L)
        first, count = self._range(N, first, count)
        self._check(mask, N, K, base, M, offsets, targets)
        self._per_slot(indeg, M, "indeg")
        if nbr_off.dtype != torch.int64 or not nbr_off.is_contiguous() or nbr_off.numel() != M + 1:
            raise AmmsbError("cores: nbr_off must be a contiguous [M + 1] int64 (uint64 bits) device tensor")
        if L < 0 or L >= self.co.MAX_NBR:
            raise AmmsbError("cores: %d entries of nbr; the library takes fewer than 2^32" % L)
        nbr = self.ctx.empty((L,), torch.int32) if nbr is None else nbr
        if nbr.dtype != torch.int32 or not nbr.is_contiguous() or nbr.numel() != L:
            raise AmmsbError("cores: nbr must be a contiguous [L] int32 (uint32 bits) device tensor")
        if count and M and L:
            self.co.check(self.lib.ammsb_cores_adjacency(_ptr(mask), N, K, _ptr(base), M, _ptr(offsets), _ptr(targets), first,
                                                         count, _ptr(indeg), _ptr(nbr_off), L, _ptr(nbr), _stream()))
        return nbr

    def state(self, N, K, M, indeg, counts=None):
        """-> the buffers of one peel and finish for an N x K pi with M slots: name -> device tensor (uint32 as int32, uint64
        as int64); deg [M], a copy of indeg that the peel lowers to the core numbers; queue [M]; ctl [2] int64 (tail, then
        next_level in the low half of the second word); members, inlinks2, degeneracy, nucleus, isolated [K], zeroed;
        best_core, best_comm, in_nucleus [N]; counts [4]"""
        self._per_slot(indeg, M, "indeg")
        out = {"deg": indeg.clone(), "queue": self.ctx.empty((M,), torch.int32), "ctl": self.ctx.zeros((2,), torch.int64)}
        out.update({name: self.ctx.zeros((K,), dtype) for name, dtype in self.PER_COMMUNITY})
        out.update({name: self.ctx.zeros((N,), dtype) for name, dtype in self.PER_NODE})
        out["counts"] = self.ctx.zeros((4,), torch.int64) if counts is None else counts
        return out

    def peel(self, M, indeg, nbr_off, nbr, state, num_nbr=None):
        """the host loop of the header over state["deg"]: scan a level, peel its queue launch by launch, read tail and
        next_level back (12 bytes) after every launch; ends when every slot is queued.  nbr holds num_nbr entries (default:
        all of it); rows need not be packed -> (scans, rounds) of this call"""
        M = self.co.check_slots(M)
        num_nbr = int(nbr.numel() if num_nbr is None else num_nbr)
        deg, queue, ctl, counts = state["deg"], state["queue"], state["ctl"], state["counts"]
        for t, what in ((indeg, "indeg"), (deg, "deg"), (queue, "queue")):
            self._per_slot(t, M, what)
        if nbr.dtype != torch.int32 or not nbr.is_contiguous() or num_nbr > nbr.numel() or num_nbr >= self.co.MAX_NBR:
            raise AmmsbError("cores: nbr must be a contiguous int32 (uint32 bits) device tensor of fewer than 2^32 entries")
        if nbr_off.dtype != torch.int64 or not nbr_off.is_contiguous() or nbr_off.numel() < M:
            raise AmmsbError("cores: nbr_off must be a contiguous int64 (uint64 bits) device tensor of at least M entries")
        if not M:
            return 0, 0
        tail_p, next_p = C.c_void_p(ctl.data_ptr()), C.c_void_p(ctl.data_ptr() + 8)
        none = 0xFFFFFFFF
        reset = torch.tensor([0, none], dtype=torch.int64, device=ctl.device)
        ctl.copy_(reset)
        scans = rounds = 0
        level = head = 0

        def read():
            got = ctl.cpu().numpy().view(np.uint32)   # (tail's two halves, next_level)
            return int(got[0]) | (int(got[1]) << 32), int(got[2])

        def scan(level, tail):
            reset[0] = tail
            ctl.copy_(reset)    # (next_level back to "none"; tail as it is)
            self.co.check(self.lib.ammsb_cores_scan(M, level, _ptr(deg), _ptr(queue), tail_p, next_p, _ptr(counts), _stream()))
            return read()

        tail = 0
        while True:
            tail, nxt = scan(level, tail)
            scans += 1
            if tail == head:                       # nothing at this level
                if tail >= M or nxt == none:
                    break
                level = nxt                        # (no peel ran since the scan: the smallest degree left)
                continue
            if level == 0:
                head = tail                        # (a slot of degree 0 has no row: nothing to lower)
            while head < tail:
                nb = _ptr(nbr) if nbr.numel() else None
                self.co.check(self.lib.ammsb_cores_peel(M, level, head, tail, _ptr(nbr_off), _ptr(indeg), nb, num_nbr, _ptr(deg),
                                                        _ptr(queue), tail_p, _ptr(counts), _stream()))
                rounds += 1
                head = tail
                tail, _ = read()
                if tail > M:
                    raise AmmsbError("cores: the queue holds %d slots of %d" % (tail, M))
            if tail >= M:
                break
            level += 1
        if tail != M:
            raise AmmsbError("cores: the peel ended with %d of %d slots queued" % (tail, M))
        return scans, rounds

    def finish(self, N, K, base, M, slot_comm, indeg, state):
        """after peel(): the K- and N-sized arrays of the state from indeg and core = state["deg"] -> state"""
        N, K, M = int(N), int(K), self.co.check_slots(M)
        if M and (slot_comm.dtype != torch.int16 or not slot_comm.is_contiguous() or slot_comm.numel() != M):
            raise AmmsbError("cores: slot_comm must be a contiguous [M] int16 (uint16 bits) device tensor")
        slot = lambda t: _ptr(t) if M else None   # noqa: E731  (an empty tensor has no address)
        node = lambda name: _ptr(state[name]) if N else None   # noqa: E731
        self.co.check(self.lib.ammsb_cores_finish(
            N, K, _ptr(base), M, slot(slot_comm), slot(indeg), slot(state["deg"]), _ptr(state["members"]),
            _ptr(state["inlinks2"]), _ptr(state["degeneracy"]), _ptr(state["nucleus"]), _ptr(state["isolated"]),
            node("best_core"), node("best_comm"), node("in_nucleus"), _stream()))
        return state

    def run(self, pi, thr, offsets, targets, max_bytes=None, mask=None):
        """-> (state, base, M, slot_comm, indeg, nbr_off, nbr) for the cover (pi, thr) and the simple CSR; the core numbers
        are state["deg"]"""
        N, K = int(pi.desc.num_rows), int(pi.cols)
        thr = self.co.check_threshold(thr)
        mask = self.links.mask(pi, thr) if mask is None else mask
        base, M = self.comp.base(self.comp.own(mask, N, K), thr)
        self.co.check_slots(M, thr)
        slots = self.comp.slots(mask, N, K, base, M, self.comp.state(N, K, M))
        slot_comm = slots["slot_comm"]
        del slots
        indeg, counts = self.degrees(mask, N, K, base, M, offsets, targets)
        nbr_off, L = self.offsets(indeg, max_bytes, thr)
        nbr = self.adjacency(mask, N, K, base, M, offsets, targets, indeg, nbr_off, L)
        state = self.state(N, K, M, indeg, counts)
        self.peel(M, indeg, nbr_off, nbr, state)
        return self.finish(N, K, base, M, slot_comm, indeg, state), base, M, slot_comm, indeg, nbr_off, nbr

    def kernel_name(self):
        return self.co.last_kernel_name()


class ChainAverage:
    """The running mean of (pi, beta) over the iterations since it was started (include/ammsb_average.h).  Owns a second
    matrix of pi's geometry (left uninitialised: a row's first flush does not read it), last [N], beta's binary64 mean
    and its binary32 rounding.  n counts the samples; the owner of the loop calls rows() with the mini-batch nodes and the
    n BEFORE an iteration, then bumps n and calls vector() after it.  flush() brings every row to n before a read."""

    FLUSH_SLAB_BYTES = 256 << 20  # most bytes of pi one flush launch walks

    def __init__(self, ctx, pi, beta):
        from . import _average
        self.ctx = ctx
        self.av = _average
        self.lib = _average.load()
        self.mean = RowPartitionedMatrix(ctx, pi.rows, pi.cols, pi.rows_in_block)
        self.last = ctx.zeros((pi.rows,), torch.int32)
        self.beta64 = ctx.empty((int(beta.numel()),), torch.float64)
        self.beta32 = ctx.empty((int(beta.numel()),), torch.float32)
        self.n = 0
        self.flushed = 0   # the n every row and beta32 were last brought to

    def reset(self):
        self.last.zero_()
        self.n = self.flushed = 0

    def rows(self, pi, n, nodes=None, count=None, first=0):
        """flush the rows nodes[:count] (a contiguous int32 device tensor of uint32 ids), or first .. first + count, to n"""
        if nodes is not None:
            if nodes.dtype != torch.int32 or not nodes.is_contiguous():
                raise AmmsbError("chain average: nodes must be a contiguous int32 (uint32 bits) device tensor")
            count = int(nodes.numel()) if count is None else int(count)
            if count > nodes.numel():
                raise AmmsbError("chain average: count %d past the %d listed nodes" % (count, nodes.numel()))
        else:
            count = pi.rows - int(first) if count is None else int(count)
        self.av.check(self.lib.ammsb_average_rows(C.byref(pi.desc), C.byref(self.mean.desc), _ptr(self.last), _ptr(nodes),
                                                  int(first), count, int(n), _stream()))

    def vector(self, x, n):
        """fold the float32 vector x (beta) into the binary64 mean as sample n"""
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != self.beta64.numel():
            raise AmmsbError("chain average: not the learner's beta")
        self.av.check(self.lib.ammsb_average_vector(_ptr(x), _ptr(self.beta64), int(x.numel()), int(n), _stream()))

    def round(self):
        """-> beta's mean rounded to float32 (the tensor the views hold)"""
        self.av.check(self.lib.ammsb_average_round(_ptr(self.beta64), _ptr(self.beta32), int(self.beta64.numel()), _stream()))
        return self.beta32

    def flush(self, pi):
        """every row of mean and beta32 up to date with n; nothing is launched when nothing ran since the last flush"""
        if self.n == 0:
            raise AmmsbError("chain average: no sample yet")
        if self.flushed == self.n:
            return
        slab = max(1, self.FLUSH_SLAB_BYTES // (4 * pi.cols))
        for lo in range(0, pi.rows, slab):
            self.rows(pi, self.n, first=lo, count=min(slab, pi.rows - lo))
        self.round()
        self.flushed = self.n

    def kernel_name(self):
        return self.av.last_kernel_name()


class ChainSpread(ChainAverage):
    """The running mean AND population variance of (pi, beta) over the iterations since it was started
    (include/ammsb_spread.h).  ChainAverage's interface and state, plus a third matrix of pi's geometry (var, uninitialised
    like mean) and beta's binary64 sum of squared deviations; rows() and vector() go to libammsb_spread.so, which leaves
    mean and beta's mean bit for bit what ChainAverage would.  bound() and rowsum() read the flushed state: call flush()
    first."""

    def __init__(self, ctx, pi, beta):
        super().__init__(ctx, pi, beta)
        from . import _spread
        self.sp = _spread
        self.splib = _spread.load()
        self.var = RowPartitionedMatrix(ctx, pi.rows, pi.cols, pi.rows_in_block)
        self.beta_m2 = ctx.empty((int(beta.numel()),), torch.float64)
        self.epoch = 0     # which chain n counts: reset() starts the next one, and (epoch, n) names a state of mean and var

    def reset(self):
        super().reset()
        self.epoch += 1

    def rows(self, pi, n, nodes=None, count=None, first=0):
        """flush the rows nodes[:count] (a contiguous int32 device tensor of uint32 ids), or first .. first + count, to n:
        mean and var in one pass"""
        if nodes is not None:
            if nodes.dtype != torch.int32 or not nodes.is_contiguous():
                raise AmmsbError("chain spread: nodes must be a contiguous int32 (uint32 bits) device tensor")
            count = int(nodes.numel()) if count is None else int(count)
            if count > nodes.numel():
                raise AmmsbError("chain spread: count %d past the %d listed nodes" % (count, nodes.numel()))
        else:
            count = pi.rows - int(first) if count is None else int(count)
        self.sp.check(self.splib.ammsb_spread_rows(C.byref(pi.desc), C.byref(self.mean.desc), C.byref(self.var.desc),
                                                   _ptr(self.last), _ptr(nodes), int(first), count, int(n), _stream()))

    def vector(self, x, n):
        """fold the float32 vector x (beta) into the binary64 mean and m2 as sample n"""
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != self.beta64.numel():
            raise AmmsbError("chain spread: not the learner's beta")
        self.sp.check(self.splib.ammsb_spread_vector(_ptr(x), _ptr(self.beta64), _ptr(self.beta_m2), int(x.numel()), int(n),
                                                     _stream()))

    def bound(self, z, out=None):
        """-> out (allocated unless given: a matrix of pi's geometry) = clamp(mean + z sd, 0, 1), in row slabs"""
        z = float(z)
        if not np.isfinite(z):
            raise AmmsbError("chain spread: z must be finite, not %r" % z)
        m = self.mean
        if out is None:
            out = RowPartitionedMatrix(self.ctx, m.rows, m.cols, m.rows_in_block)
        slab = max(1, self.FLUSH_SLAB_BYTES // (4 * m.cols))
        for lo in range(0, m.rows, slab):
            self.sp.check(self.splib.ammsb_spread_bound(C.byref(m.desc), C.byref(self.var.desc), C.byref(out.desc), z, lo,
                                                        min(slab, m.rows - lo), _stream()))
        return out

    def rowsum(self):
        """-> [N] float64 device tensor: every row's total variance, in the library's one order"""
        v = self.var
        out = self.ctx.empty((v.rows,), torch.float64)
        slab = max(1, self.FLUSH_SLAB_BYTES // (4 * v.cols))
        for lo in range(0, v.rows, slab):
            self.sp.check(self.splib.ammsb_spread_rowsum(C.byref(v.desc), C.c_void_p(out.data_ptr() + 8 * lo), lo,
                                                         min(slab, v.rows - lo), _stream()))
        return out

    def kernel_name(self):
        """the last kernel libammsb_spread.so launched (rows, vector, bound, rowsum).  round(), and so the end of flush(),
        launches in libammsb_average.so, which this does not see: ChainAverage.kernel_name(self) names that one"""
        return self.sp.last_kernel_name()


class ModelReducer:
    """The fitted model at fewer communities (include/ammsb_reduce.h): pi, phi_sum and theta under a _reduce.Plan.  The plan
    travels as its inverse CSR; a plan whose new communities have one source each goes as the bare source list, which is
    the select form.  Both pi matrices are alive at once: there is no in-place form."""

    def __init__(self, ctx):
        from . import _reduce
        self.ctx = ctx
        self.rd = _reduce
        self.lib = _reduce.load()

    def device_plan(self, plan, select=None):
        """-> (src_off or None, src, new_K, drops) on the device.  select: None = the select form where the plan allows it;
        False = always the CSR (the merge form); True = refuse a plan that merges"""
        if not isinstance(plan, self.rd.Plan):
            plan = self.rd.Plan(plan)
        off, src = plan.csr()
        if select is None:
            select = plan.selects
        if select and not plan.selects:
            raise AmmsbError("model reducer: the select form takes a plan that merges nothing")
        return (None if select else self.ctx.from_numpy(off)), self.ctx.from_numpy(src), plan.new_K, plan.drops

    def rows(self, pi, phi, dplan, out_pi, out_phi, emptied, first=0, count=None):
        """rows first .. first + count under device_plan()'s tuple; emptied: a zeroed int64 [1] device tensor (needed by a
        plan that drops).  pi and out_pi: RowPartitionedMatrix or anything with .desc"""
        off, src, new_K, drops = dplan
        for t, what in ((phi, "phi_sum"), (out_phi, "out_phi_sum")):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < int(pi.desc.num_rows):
                raise AmmsbError("model reducer: %s must be a contiguous float32 vector of N elements" % what)
        if emptied is not None and (emptied.dtype != torch.int64 or emptied.numel() < 1):
            raise AmmsbError("model reducer: emptied must be an int64 device tensor")
        count = int(pi.desc.num_rows) - int(first) if count is None else int(count)
        self.rd.check(self.lib.ammsb_reduce_rows(C.byref(pi.desc), _ptr(phi), _ptr(off), _ptr(src), new_K, int(drops),
                                                 C.byref(out_pi.desc), _ptr(out_phi), _ptr(emptied), int(first), count,
                                                 _stream()))

    def theta(self, theta, dplan, out_theta):
        """theta [K, 2] (2K contiguous floats) -> out_theta [K', 2]"""
        off, src, new_K, _ = dplan
        if theta.dtype != torch.float32 or not theta.is_contiguous() or theta.numel() % 2:
            raise AmmsbError("model reducer: theta must be a contiguous float32 [K, 2]")
        if out_theta.dtype != torch.float32 or not out_theta.is_contiguous() or out_theta.numel() != 2 * new_K:
            raise AmmsbError("model reducer: out_theta must be a contiguous float32 [new_K, 2]")
        self.rd.check(self.lib.ammsb_reduce_theta(_ptr(theta), _ptr(off), _ptr(src), int(theta.numel()) // 2, new_K,
                                                  _ptr(out_theta), _stream()))

    def run(self, pi, phi, theta, plan, slab_bytes=256 << 20, out_pi=None, out_phi=None, out_theta=None, select=None):
        """The whole model: pi in row slabs of at most slab_bytes of input, then theta.  Outputs are allocated unless
        given (out_pi with pi's rows and plan.new_K columns).  -> (out_pi, out_phi, out_theta, emptied rows); reading the
        count waits for the stream."""
        if not isinstance(plan, self.rd.Plan):
            plan = self.rd.Plan(plan)
        if plan.K != pi.cols:
            raise AmmsbError("model reducer: a plan over %d communities for a model of %d" % (plan.K, pi.cols))
        if int(theta.numel()) != 2 * plan.K:
            raise AmmsbError("model reducer: theta holds %d elements, not 2 x %d" % (theta.numel(), plan.K))
        c = self.ctx
        dplan = self.device_plan(plan, select)
        if out_pi is None:
            out_pi = RowPartitionedMatrix(c, pi.rows, plan.new_K)
        if out_pi.rows != pi.rows or out_pi.cols != plan.new_K:
            raise AmmsbError("model reducer: out_pi is %d x %d, not %d x %d" % (out_pi.rows, out_pi.cols, pi.rows, plan.new_K))
        out_phi = c.empty((pi.rows,), torch.float32) if out_phi is None else out_phi
        out_theta = c.empty((2 * plan.new_K,), torch.float32) if out_theta is None else out_theta
        emptied = c.zeros((1,), torch.int64)
        slab = max(1, int(slab_bytes) // (4 * pi.cols))
        for lo in range(0, pi.rows, slab):
            self.rows(pi, phi, dplan, out_pi, out_phi, emptied, first=lo, count=min(slab, pi.rows - lo))
        self.theta(theta, dplan, out_theta)
        return out_pi, out_phi, out_theta, int(emptied.item())

    def kernel_name(self):
        return self.rd.last_kernel_name()


class GraphLoop:
    """ammsb_loop (include/ammsb.h): whole iterations replayed as captured hipGraphs over a Learner's buffers."""

    def __init__(self, ctx, theta, beta, pi, phi_sum, training_set, heldout_set, phi, beta_upd, samples, sampler,
                 timestamps=False):
        self.ctx = ctx
        cfg = _capi.LoopConfig()
        cfg.theta, cfg.beta = theta.data_ptr(), beta.data_ptr()
        cfg.pi = C.pointer(pi.desc)
        cfg.phi_sum = phi_sum.data_ptr()
        cfg.training_set = C.pointer(training_set.desc)
        cfg.heldout_set = C.pointer(heldout_set.desc) if heldout_set is not None else None
        cfg.phi_seeds, cfg.phi_vec = phi.rand.seeds.data_ptr(), phi.phi_vec.data_ptr()
        cfg.phi_wg, cfg.phi_flags = phi.local, phi.flags
        cfg.beta_seeds, cfg.grads = beta_upd.rand.seeds.data_ptr(), beta_upd.grads.data_ptr()
        cfg.beta_wg, cfg.beta_flags = beta_upd.local, beta_upd.flags
        for i, s in enumerate(samples):
            ns = s.neighbor_sampler
            cfg.edges[i], cfg.nodes[i] = s.dev_edges.data_ptr(), s.dev_nodes.data_ptr()
            cfg.neighbors[i], cfg.nbr_table[i] = ns.data.data_ptr(), ns.hash.data_ptr()
            cfg.nbr_seeds[i] = ns.rand.seeds.data_ptr()
        cfg.nbr_wg = samples[0].neighbor_sampler.local
        cfg.csr_offsets, cfg.csr_targets = sampler.offsets.data_ptr(), sampler.targets.data_ptr()
        cfg.mb_seeds, cfg.mb_candidates = sampler.rand.seeds.data_ptr(), sampler.C
        cfg.mb_workspace, cfg.mb_count = sampler.workspace.data_ptr(), sampler.count.data_ptr()
        cfg.mini_batch, cfg.max_fan_out = sampler.m, sampler.max_fan_out
        cfg.max_nodes = min(int(s.dev_nodes.numel()) for s in samples)
        cfg.max_edges = min(int(s.dev_edges.numel()) for s in samples)
        cfg.flags = _capi.LOOP_TIMESTAMPS if timestamps else 0
        self.timestamps_on = bool(timestamps)
        self._keep = (theta, beta, pi, phi_sum, training_set, heldout_set, phi, beta_upd, samples, sampler)
        self._h = C.c_void_p()
        torch.cuda.synchronize()  # the captured kernels' buffers are initialised before anything replays
        ctx.check(ctx.lib.ammsb_loop_create(ctx.handle, C.byref(cfg), C.byref(self._h)))

    def run(self, pending, nxt, first_step, parity):
        """nxt: structured array of MB_CHOICE_DT (DeviceMiniBatchSampler.choose_many) or a list of 4-tuples."""
        if not isinstance(nxt, np.ndarray):
            nxt = np.array([tuple(int(x) for x in ch) for ch in nxt], dtype=MB_CHOICE_DT)
        nxt = np.ascontiguousarray(nxt)
        n = int(nxt.shape[0])
        pend = _capi.MbChoice(*[int(x) for x in pending])
        self.ctx.check(self.ctx.lib.ammsb_loop_run(self._h, C.byref(pend),
                                                   C.cast(nxt.ctypes.data, C.POINTER(_capi.MbChoice)), n,
                                                   int(first_step), int(parity), _stream()))

    def check(self):
        """Synchronises the loop's streams.  If a device-side wait between the two chains gave up, the library has
        skipped what came after it, switched to the stream-event hand-over and re-run the missing steps by the time
        this returns (ammsb_loop_check; status() counts the fallback); raises only if that recovery failed."""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.ammsb_loop_check(self._h, C.byref(n)))
        if n.value:
            raise AmmsbError("graph loop: %d device-side wait(s) timed out and the run could not be resumed on the "
                             "event hand-over" % n.value)

    def status(self):
        """(event_handover, fallbacks): whether the chains are ordered with stream events, and how many runs had to be
        finished that way after a device-side wait gave up."""
        ev, fb = C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.lib.ammsb_loop_status(self._h, C.byref(ev), C.byref(fb)))
        return bool(ev.value), int(fb.value)

    def timestamps(self, first_step, n):
        """(begin_ns, end_ns) arrays of update_phi for steps first_step .. first_step + n - 1.  Synchronises."""
        b, e = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self.ctx.check(self.ctx.lib.ammsb_loop_timestamps(self._h, int(first_step), int(n), b.ctypes.data_as(dp),
                                                          e.ctypes.data_as(dp)))
        return b, e

    STAMP_SLOTS = 8  # AMMSB_LOOP_STAMP_SLOTS
    STAMP_NAMES = ("update_phi", "update_pi", "beta_grads", "sum_theta", "released", "next_batch")

    def step_stamps(self, first_step, n):
        """[n, 8] device times in ns of steps first_step .. first_step + n - 1 (include/ammsb.h,
        ammsb_loop_step_stamps): columns 0..3 = start of update_phi / update_pi / the partial-row kernel / the
        partial-row sum + theta step, 4 = step released, 5 = next mini-batch available.  Synchronises."""
        out = np.zeros((int(n), self.STAMP_SLOTS), dtype=np.float64)
        self.ctx.check(self.ctx.lib.ammsb_loop_step_stamps(self._h, int(first_step), int(n),
                                                           out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def close(self):
        if self._h:
            self.ctx.lib.ammsb_loop_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- stream / event / collective plumbing used by learner.py (torch is the transport only)

def new_stream(ctx):
    """Stream of a Sample (sampling + neighbour kernels of the NEXT mini-batch).  Default priority on
    purpose: a same-box A/B of high priority showed no gain, and at default priority the chain already finishes
    inside the update_phi launch it overlaps."""
    return torch.cuda.Stream(device=ctx.device)


def stream(s):
    return _StreamScope(s)


def new_event():
    return torch.cuda.Event()


def record_event(ev):
    ev.record(_torch_stream())  # on the current stream


def sync_event(ev):
    ev.synchronize()  # the HOST waits (wait_event makes the current stream wait)


def wait_event(ev):
    ev.wait(_torch_stream())  # the current stream waits for the event


def synchronize():
    torch.cuda.synchronize()


def timing_mark():
    """A timing event recorded on torch's current stream (the multi-GPU step trace, Learner.shard_trace)."""
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(_torch_stream())
    return ev


def mark_elapsed_ms(a, b):
    """Device time between two timing_mark()s (both must have completed: call synchronize() first)."""
    return a.elapsed_time(b)


def elapsed_ms(fn):
    """Device time of fn() on the current stream (HIP events), for start-up calibration."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(torch.cuda.current_stream())
    fn()
    b.record(torch.cuda.current_stream())
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=True)


class ClockProbe:
    """ammsb_clock_probe: the shader clock every XCD holds while something else runs.  launch() enqueues the probe
    blocks on the probe's own stream (beside whatever the caller has in flight); read() waits for them and returns
    {"mhz_per_xcd": [...], "mhz": median, "blocks": n}."""

    def __init__(self, ctx, n_blocks=64):
        self.ctx, self.n = ctx, int(n_blocks)
        self.buf = ctx.zeros((self.n, 3), torch.int64)
        self.stream = torch.cuda.Stream(device=ctx.device)
        self.done = torch.cuda.Event()

    def launch(self, spin_us=200):
        c = self.ctx
        c.check(c.lib.ammsb_clock_probe(c.handle, _ptr(self.buf), self.n, int(spin_us), C.c_void_p(self.stream.cuda_stream)))
        self.done.record(self.stream)

    def read(self):
        self.done.synchronize()
        t = self.buf.cpu().numpy().astype(np.float64)
        ok = t[:, 1] > 0
        mhz = t[ok, 0] / t[ok, 1] * 100.0
        per = [round(float(np.median(mhz[t[ok, 2] == x])), 1) if (t[ok, 2] == x).any() else None for x in range(8)]
        return {"mhz_per_xcd": per, "mhz": round(float(np.median(mhz)), 1) if mhz.size else None, "blocks": int(ok.sum())}


def _via_host(dist, group):
    """gloo has no all_gather_into_tensor and no device transport: when the process group is gloo (several
    ranks sharing one GPU in tests, or a box without RCCL) the payload is staged through host memory.  Only
    the exchange changes; every kernel still runs on the device."""
    return dist.get_backend(group) == "gloo"


def all_gather_rows_async(dist, region, chunk, rank, world, group, mode="collective"):
    """In-place all-gather of the `world` equal row chunks of `region` (rank r owns chunk r), issued
    asynchronously: RCCL runs it on its own stream behind the work already queued on the current one,
    so the next phi launch overlaps it.  The in-place form (send buffer = own slot of the receive
    buffer) moves each chunk once.
    mode "collective": one all_gather_into_tensor.  mode "p2p": the direct form -- this rank's chunk sent to each
    of the world - 1 peers and their chunks received, as ONE batch of point-to-point operations (RCCL runs the
    2 (world - 1) transfers of a batch concurrently, one per xGMI link on a fully connected node, where a ring
    all-gather is bound by a single link's rate).  Same result; Learner._calibrate_split times both."""
    if _via_host(dist, group):
        mine = region[rank * chunk:(rank + 1) * chunk].cpu()
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        for r in range(world):
            if r != rank:
                region[r * chunk:(r + 1) * chunk].copy_(parts[r])
        return None
    if mode == "p2p" and world > 1:
        return p2p_all_gather_rows(dist, region, chunk, rank, world, group)
    return dist.all_gather_into_tensor(region, region[rank * chunk:(rank + 1) * chunk], group=group, async_op=True)


def p2p_all_gather_rows(dist, region, chunk, rank, world, group):
    """The direct form of the in-place all-gather: one batch of 2 (world - 1) point-to-point operations.  Returns
    the batch's work handles (wait_work takes the list)."""
    mine = region[rank * chunk:(rank + 1) * chunk]
    peer = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    batch = []
    for d in range(1, world):  # rank r sends to r + d and receives from r - d in round d: every link busy in every round
        to, frm = (rank + d) % world, (rank - d) % world
        batch.append(dist.P2POp(dist.isend, mine, peer(to), group))
        batch.append(dist.P2POp(dist.irecv, region[frm * chunk:(frm + 1) * chunk], peer(frm), group))
    return dist.batch_isend_irecv(batch)


def broadcast_async(dist, rows, src, group):
    if _via_host(dist, group):
        host = rows.cpu()
        dist.broadcast(host, src=src, group=group)
        if dist.get_rank(group) != src:
            rows.copy_(host)
        return None
    return dist.broadcast(rows, src=src, group=group, async_op=True)


def wait_work(work):
    if work is None:
        return
    for w in (work if isinstance(work, (list, tuple)) else [work]):
        w.wait()  # makes the current stream wait for the collective; does not block the host


def all_gather_flat(dist, out, local, rank, world, group):
    """out[r] = rank r's `local` (tiny payloads: [2K] gradient partials, 4 perplexity scalars)."""
    if _via_host(dist, group):
        mine = local.reshape(-1).cpu()
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        out.copy_(torch.stack(parts).reshape(out.shape))
        return
    dist.all_gather_into_tensor(out.view(-1), local.reshape(-1), group=group)
