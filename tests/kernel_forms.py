"""The kernel-form tables: every template instantiation the dispatchers of update_phi / update_pi, the beta gradient,
perplexity and the neighbour sampler can select, one row per form, with the environment (or in-process debug switch)
that selects it, the shape, the pi block count and the FULL name ctx.kernel_names() must report.

test_gpu_kernel_forms.py runs every row against the oracle; test_kernel_census.py checks, without a GPU, that these
tables and EXCLUDED together name every kernel instantiation in libammsb_hip.so and nothing that is not in it.
Plain Python: imports without torch and without a GPU.

Names are spelled as ammsb_kname(...) spells them, with integer suffixes dropped ("2u" -> "2": see normalize()).
"""
import re
from collections import namedtuple

# env:    ((variable, value), ...) set for the whole child process (the switches are read once per process)
# debug:  in-process switches of the row: {"phi_forms": (lds3, nb, ring)} (ammsb_debug_phi_forms, reset to -1 after),
#         {"beta_slots": "<P>"} (AMMSB_BETA_SLOTS, read at every call)
# op:     "phi" (update_phi + update_pi), "grads", "fused" (update_pi + gradient as one launch), "ppx", "nbr"
# shape:  (N, K, n, nodes, wg) -- nodes: mini-batch nodes (phi), edges (grads / fused), held-out edges (ppx)
# blocks: pi row blocks (2: rows of the mini-batch on both sides of the block boundary -> the `false` instantiations)
# flags:  "streaming" (one-wave-per-node forms only, AMMSB_PHI_STREAMING) or "small" (whatever a launch of this size takes)
# kernel: {kernel_names() slot: full name}; "" = the slot must stay empty (that form did not run)
Row = namedtuple("Row", "env debug op shape blocks flags kernel")

REG_ENV = (("AMMSB_PHI_FORM", "r"), ("AMMSB_BETA_FORM", "r"), ("AMMSB_PPX_FORM", "r"))
WGS = (16, 32, 64, 128, 256, 512, 1024)
KPTS = (1, 2, 4, 8, 16, 32)


def normalize(name):
    """'void (anonymous namespace)::ppx_lds_kernel<16, 2u, 64, true>(PpxArgs)' -> 'ppx_lds_kernel<16, 2, 64, true>'."""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    name = name.replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(name):  # cut the parameter list: the first '(' outside the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            name = name[:i]
            break
    return re.sub(r"\b(\d+)u\b", r"\1", name)


def _b(one):
    return "true" if one else "false"


def lds(kpt, w, d, nb, vl, blocks):
    return "update_phi_lds_kernel<%d, %d, %d, %d, %d, %s>" % (kpt, w, d, nb, vl, _b(blocks == 1))


def lds2(kpt, d, u, vl, blocks):
    return "update_phi_lds2_kernel<%d, %d, %d, %d, %s>" % (kpt, d, u, vl, _b(blocks == 1))


def lds3(vl, blocks):
    return "update_phi_lds3_kernel<16, %d, %s>" % (vl, _b(blocks == 1))


def pick_kpt(K, L):
    need = (K + L - 1) // L
    return next((c for c in KPTS if c >= need), 0)


def pi_name(K, wg):
    kpt = pick_kpt(K, wg)
    if kpt == 0:
        return "update_pi_gen_kernel<%d>" % (8 if K <= 4096 else 16)
    return "update_pi_kernel<%d, %d>" % (wg, kpt)


def phi(env, shape, blocks, name, flags="streaming", debug=None):
    K, wg = shape[1], shape[4]
    slot = "update_phi_small" if "wide_kernel" in name else "update_phi"
    kernel = {slot: name, "update_pi": pi_name(K, wg)}
    kernel["update_phi" if slot == "update_phi_small" else "update_phi_small"] = ""
    return Row(tuple(env), debug or {}, "phi", tuple(shape), blocks, flags, kernel)


def both(env, shape, make, flags="streaming", debug=None):
    """the single-block (`true`) and the two-block (`false`) instantiation of one form"""
    return [phi(env, shape, b, make(b), flags, debug) for b in (1, 2)]


def grads(env, shape, blocks, name, debug=None, op="grads"):
    # the partial-row sum that follows: the 8-wide form needs 2K % 8 == 0 (and a 16-byte aligned output, which a torch
    # allocation is)
    total = "sum_partials8_kernel" if shape[1] % 4 == 0 else "sum_partials_kernel"
    return Row(tuple(env), debug or {}, op, tuple(shape), blocks, "", {"beta_grads": name, "grads_sum": total})


def ppx(env, shape, blocks, name):
    return Row(tuple(env), {}, "ppx", tuple(shape), blocks, "", {"perplexity": name})


def nbr(env, shape, name):
    return Row(tuple(env), {}, "nbr", tuple(shape), 1, "", {"sample_neighbors": name})


def _default_rows():
    E = ()
    rows = []
    # ---- update_phi, one wave (or wg / 64 waves) per node, wg 64 and up
    rows += both(E, (2048, 256, 32, 200, 64), lambda b: lds2(4, 8, 4, 64, b))
    rows += both(E, (2048, 256, 6, 100, 64), lambda b: lds2(4, 8, 2, 64, b))
    rows += both(E, (2048, 256, 5, 100, 64), lambda b: lds(4, 1, 8, 1, 64, b))
    rows += both(E, (2048, 512, 32, 100, 64), lambda b: lds2(8, 4, 2, 64, b))
    rows += both(E, (2048, 512, 7, 100, 64), lambda b: lds(8, 1, 4, 1, 64, b))
    rows += both(E, (1024, 1024, 32, 64, 64), lambda b: lds(16, 1, 2, 1, 64, b))
    rows += both(E, (512, 2048, 8, 40, 64), lambda b: lds(32, 1, 2, 1, 64, b))
    rows += both(E, (1024, 1024, 8, 40, 128), lambda b: lds(8, 2, 2, 1, 64, b))
    rows += both(E, (512, 2048, 8, 40, 128), lambda b: lds(16, 2, 2, 1, 64, b))
    rows += both(E, (512, 4096, 4, 16, 256), lambda b: lds(16, 4, 2, 1, 64, b))
    rows += both(E, (300, 8192, 3, 6, 512), lambda b: lds(16, 8, 2, 1, 64, b))
    # ---- wg 32: 32 virtual lanes on the one-wave kernels
    rows += both(E, (2048, 256, 5, 100, 32), lambda b: lds(4, 1, 8, 1, 32, b))
    rows += both(E, (2048, 256, 6, 100, 32), lambda b: lds2(4, 8, 2, 32, b))
    rows += both(E, (2048, 256, 32, 200, 32), lambda b: lds2(4, 8, 4, 32, b))
    rows += both(E, (2048, 512, 7, 100, 32), lambda b: lds(8, 1, 4, 1, 32, b))
    rows += both(E, (2048, 512, 32, 100, 32), lambda b: lds2(8, 4, 2, 32, b))
    rows += both(E, (1024, 1024, 32, 64, 32), lambda b: lds(16, 1, 2, 1, 32, b))
    rows += both(E, (512, 2048, 8, 40, 32), lambda b: lds(32, 1, 2, 1, 32, b))
    # ---- ammsb_debug_phi_forms(lds3, nb, ring): the ring depths, two nodes per block, the three-slot kernel
    for ring, shape, make in [(2, (2048, 256, 32, 200, 64), lambda b: lds(4, 1, 2, 1, 64, b)),
                              (2, (2048, 512, 32, 100, 64), lambda b: lds(8, 1, 2, 1, 64, b)),
                              (4, (2048, 256, 32, 200, 64), lambda b: lds(4, 1, 4, 1, 64, b)),
                              (4, (2048, 512, 32, 100, 64), lambda b: lds(8, 1, 4, 1, 64, b)),
                              (4, (1024, 1024, 32, 64, 64), lambda b: lds(16, 1, 4, 1, 64, b)),
                              (8, (2048, 256, 32, 200, 64), lambda b: lds(4, 1, 8, 1, 64, b)),
                              (22, (2048, 256, 32, 200, 64), lambda b: lds2(4, 8, 2, 64, b)),
                              (42, (2048, 256, 32, 200, 64), lambda b: lds2(4, 4, 2, 64, b)),
                              (42, (2048, 256, 6, 100, 64), lambda b: lds2(4, 4, 2, 64, b))]:
        rows += both(E, shape, make, debug={"phi_forms": (-1, -1, ring)})
    rows += both(E, (1024, 1024, 32, 65, 64), lambda b: lds(16, 1, 2, 2, 64, b), debug={"phi_forms": (-1, 2, -1)})  # odd node count: an idle half-block
    rows += both(E, (1024, 1024, 32, 64, 64), lambda b: lds3(64, b), debug={"phi_forms": (1, -1, -1)})
    rows += both(E, (1024, 1024, 50, 64, 32), lambda b: lds3(32, b), debug={"phi_forms": (1, -1, -1)})
    rows += both(E, (1024, 1024, 17, 64, 64), lambda b: lds(16, 1, 2, 1, 64, b), debug={"phi_forms": (1, -1, -1)})  # n < KV + 2
    rows += both(E, (1024, 1024, 32, 64, 64), lambda b: lds(16, 1, 2, 1, 64, b), debug={"phi_forms": (0, -1, -1)})
    # ---- small launches: update_phi_wide_kernel, and the edges of its range
    for K, kpt, rw in ((256, 4, 15), (512, 8, 11), (1024, 16, 11)):
        for wg in (32, 64):
            rows.append(phi(E, (2048, K, 8, 100, wg), 1, "update_phi_wide_kernel<%d, %d, %d>" % (kpt, rw, wg), "small"))
    rows.append(phi(E, (2048, 256, 8, 100, 64), 2, "update_phi_wide_kernel<4, 15, 64>", "small"))
    rows.append(phi(E, (1024, 1024, 35, 512, 64), 1, "update_phi_wide_kernel<16, 11, 64>", "small"))  # wide_max groups, 4K(n+2)+4n = 151 692 B
    rows.append(phi(E, (1024, 1024, 35, 513, 64), 1, lds(16, 1, 2, 1, 64, 1), "small"))      # one group more
    rows.append(phi(E, (1024, 1024, 36, 100, 64), 1, lds(16, 1, 2, 1, 64, 1), "small"))      # 155 792 B > 150 KiB
    # ---- the generic kernel: more than 32 columns per work-item
    rows.append(phi(E, (512, 4096, 4, 16, 32), 1, "update_phi_gen_kernel<8, 4>"))
    rows.append(phi(E, (512, 4096, 6, 16, 32), 2, "update_phi_gen_kernel<8, 2>"))
    rows.append(phi(E, (512, 4096, 5, 16, 32), 1, "update_phi_gen_kernel<8, 1>"))
    rows.append(phi(E, (300, 8192, 3, 6, 32), 2, "update_phi_gen_kernel<16, 1>"))
    # ---- gradient
    for shape, name in [((2048, 256, 8, 3000, 64), "beta_grads_lds_kernel<4, 1, false, 64>"),
                        ((2048, 512, 8, 500, 64), "beta_grads_lds_kernel<8, 1, false, 64>"),
                        ((4096, 1024, 8, 1024, 64), "beta_grads_lds_kernel<16, 1, false, 64>"),
                        ((1024, 2048, 8, 300, 128), "beta_grads_lds_kernel<16, 2, false, 64>"),
                        ((1024, 4096, 8, 700, 256), "beta_grads_lds_kernel<16, 4, false, 64>"),
                        ((2048, 256, 8, 3000, 32), "beta_grads_lds_kernel<4, 1, false, 32>"),
                        ((2048, 512, 8, 500, 32), "beta_grads_lds_kernel<8, 1, false, 32>"),
                        ((4096, 1024, 8, 1024, 32), "beta_grads_lds_kernel<16, 1, false, 32>"),
                        ((1024, 4096, 8, 700, 32), "beta_grads_gen_kernel<8>"),
                        ((300, 8192, 8, 200, 32), "beta_grads_gen_kernel<16>"),
                        ((2048, 64, 8, 9000, 16), "beta_grads_kernel<16, 4, false, false>"),  # P clamped at max_partials
                        ((2048, 1021, 8, 500, 64), "beta_grads_kernel<64, 16, false, false>"),  # K % 4 != 0: sum_partials_kernel
                        ((2048, 50, 8, 500, 64), "beta_grads_kernel<64, 1, false, false>")]:
        rows += [grads(E, shape, b, name) for b in (1, 2)]
    # AMMSB_BETA_SLOTS: P below the edge count, equal to it, the floor of 64, the clamp at max_partials (the P used is
    # checked through the summation order it fixes: kernel_forms_child.py emulates it from the oracle's per-edge terms)
    for slots, n_edges in (("100", 500), ("500", 500), ("10", 500), ("100000000", 5000)):
        rows.append(grads(E, (2048, 256, 8, n_edges, 64), 1, "beta_grads_lds_kernel<4, 1, false, 64>",
                          debug={"beta_slots": slots}))
    rows.append(grads(E, (2048, 256, 8, 500, 64), 2, "beta_grads_lds_kernel<4, 1, false, 64>", debug={"beta_slots": "100"}))
    # ---- update_pi + gradient as one launch
    for K, kpt in ((256, 4), (512, 8), (1024, 16)):
        for wg in (32, 64):
            rows += [grads(E, (2048, K, 8, 300, wg), b, "beta_grads_lds_kernel<%d, 1, true, %d>" % (kpt, wg), op="fused")
                     for b in (1, 2)]
    for K, wg, kpt in ((64, 64, 1), (128, 64, 2), (32, 32, 1), (64, 32, 2)):
        rows += [grads(E, (2048, K, 8, 300, wg), b, "beta_grads_kernel<%d, %d, true, %s>" % (wg, kpt, _b(b == 1)), op="fused")
                 for b in (1, 2)]
    # ---- perplexity
    for K, kpt in ((256, 4), (512, 8), (1024, 16)):
        for wg in (32, 64):
            rows += [ppx(E, (1024, K, 8, 600, wg), b, "ppx_lds_kernel<%d, 2, %d, false>" % (kpt, wg)) for b in (1, 2)]
    rows.append(ppx(E, (512, 4096, 8, 600, 32), 1, "ppx_gen_kernel<8>"))
    rows.append(ppx(E, (300, 8192, 8, 600, 32), 2, "ppx_gen_kernel<16>"))
    # ---- neighbour sampler
    rows.append(nbr(E, (1000, 32, 32, 3000, 32), "sample_neighbors_wave_kernel"))
    rows.append(nbr(E, (100000, 32, 32, 20001, 32), "sample_neighbors_lds_kernel"))  # more nodes than the wave form takes
    rows.append(nbr(E, (5000, 32, 8, 300, 32), "sample_neighbors_lds_kernel"))
    rows.append(nbr(E, (5000, 32, 200, 300, 32), "sample_neighbors_kernel"))  # table too large for LDS
    return rows


def _switch_rows():
    rows = []
    E = (("AMMSB_PHI_NT", "1"),)  # non-temporal neighbour-row loads at small pi (on by default above 256 MB)
    rows += both(E, (2048, 256, 32, 200, 64), lambda b: lds2(4, 8, 4, 64, b))
    rows += both(E, (2048, 512, 32, 100, 32), lambda b: lds2(8, 4, 2, 32, b))
    rows += both(E, (2048, 256, 5, 100, 64), lambda b: lds(4, 1, 8, 1, 64, b))
    rows += both(E, (1024, 1024, 32, 64, 64), lambda b: lds(16, 1, 2, 1, 64, b))
    rows += both(E, (1024, 1024, 32, 64, 64), lambda b: lds3(64, b), debug={"phi_forms": (1, -1, -1)})
    rows += both(E, (1024, 1024, 32, 65, 64), lambda b: lds(16, 1, 2, 2, 64, b), debug={"phi_forms": (-1, 2, -1)})
    E = (("AMMSB_PHI_WIDE", "0"),)
    rows.append(phi(E, (2048, 256, 8, 100, 64), 1, lds2(4, 8, 4, 64, 1), "small"))
    rows.append(phi(E, (2048, 1024, 8, 100, 32), 1, lds(16, 1, 2, 1, 32, 1), "small"))
    E = (("AMMSB_PHI_WIDE", "100"),)
    rows.append(phi(E, (2048, 256, 8, 100, 64), 1, "update_phi_wide_kernel<4, 15, 64>", "small"))
    rows.append(phi(E, (2048, 256, 8, 101, 64), 1, lds2(4, 8, 4, 64, 1), "small"))
    E = (("AMMSB_PHI_WIDE_RW", "8"),)
    for K, kpt in ((256, 4), (512, 8), (1024, 16)):
        for wg in (32, 64):
            rows.append(phi(E, (2048, K, 8, 100, wg), 1, "update_phi_wide_kernel<%d, 8, %d>" % (kpt, wg), "small"))
    # persistent grid of update_phi_lds2_kernel: it is used once a launch has more groups than the chip holds resident
    # blocks (per_cu x CUs).  The node counts exceed 32 one-wave blocks x 256 CUs, the most any occupancy allows, so every
    # mode here runs the persistent grid (the child asserts it against the device's CU count).  Which of mode 1's two
    # grids (resident slots, or the even spread of mode 3) a count takes depends on the occupancy, which is not asserted.
    for mode in ("1", "3"):
        E = (("AMMSB_PHI_PERSIST", mode),)
        rows.append(phi(E, (20000, 256, 32, 9000, 64), 1, lds2(4, 8, 4, 64, 1)))
        rows.append(phi(E, (20000, 256, 16, 8292, 32), 2, lds2(4, 8, 4, 32, 2)))
    E = (("AMMSB_PHI_STREAM", "1"),)
    rows.append(phi(E, (20000, 256, 32, 5000, 64), 1, "update_phi_stream_kernel<4, 8, 4, 64>"))
    rows.append(phi(E, (20000, 256, 16, 3001, 32), 2, "update_phi_stream_kernel<4, 8, 4, 32>"))
    for mode, K, n, name in (("1", 256, 32, "update_phi_pair_kernel<8, 4, 2, %d>"),
                             ("1", 512, 8, "update_phi_pair_kernel<16, 4, 2, %d>"),
                             ("2", 256, 6, "update_phi_pair_kernel<8, 8, 2, %d>"),
                             ("3", 256, 32, "update_phi_pair_kernel<8, 8, 4, %d>")):
        E = (("AMMSB_PHI_PAIR", mode),)
        rows.append(phi(E, (2048, K, n, 201, 64), 1, name % 64))
        rows.append(phi(E, (2048, K, n, 100, 32), 2, name % 32))
    E = (("AMMSB_PPX_FOLD", "1"),)  # the launch reduces its own partials through a last-block ticket
    for K, kpt in ((256, 4), (512, 8), (1024, 16)):
        for wg in (32, 64):
            rows.append(ppx(E, (1024, K, 8, 600, wg), 1 if wg == 64 else 2, "ppx_lds_kernel<%d, 2, %d, true>" % (kpt, wg)))
    E = (("AMMSB_NBR_FORM", "t"),)
    rows.append(nbr(E, (1000, 32, 32, 3000, 32), "sample_neighbors_lds_kernel"))
    rows.append(nbr(E, (40, 32, 32, 300, 64), "sample_neighbors_lds_kernel"))
    return rows


def _reg_n(K):
    return 1024 if K <= 1024 else 512 if K <= 4096 else 256 if K <= 16384 else 128


def _register_rows():
    """the register-pipelined kernels (AMMSB_*_FORM=r): every work-group size x columns per work-item, full rows
    (K = wg * kpt) and rows with column guards (K < wg * kpt)"""
    rows = []
    for L in WGS:
        for kpt in KPTS:
            depth = 2 if kpt >= 32 else 4
            for full in (True, False):
                K = L * kpt if full else L * kpt - 3
                single = kpt <= 2 and L in (32, 64)  # (only these have a single-block `true` instantiation)
                for b in ((1, 2) if single else (2,)):
                    name = "update_phi_kernel<%d, %d, %d, %s, %s>" % (L, kpt, depth, _b(full), _b(single and b == 1))
                    rows.append(phi(REG_ENV, (_reg_n(K), K, 4 if full else 5, 24, L), b, name))
            K = L * kpt - 1
            rows.append(ppx(REG_ENV, (_reg_n(K), K, 4, 300, L), 1, "ppx_kernel<%d, %d>" % (L, kpt)))
            if kpt <= 16:
                for K in (L * kpt, L * kpt - 3):  # (the second: column guards, and K % 4 != 0)
                    rows.append(grads(REG_ENV, (_reg_n(K), K, 4, 300, L), 2, "beta_grads_kernel<%d, %d, false, false>" % (L, kpt)))
    return rows


ROWS = _default_rows() + _switch_rows() + _register_rows()


def groups():
    """[(env, [(index in ROWS, row), ...]), ...]: the rows by environment, the default environment first (one child
    process each)"""
    order, by = [], {}
    for i, r in enumerate(ROWS):
        if r.env not in by:
            order.append(r.env)
            by[r.env] = []
        by[r.env].append((i, r))
    return [(env, by[env]) for env in order]


def table_names():
    return {n for r in ROWS for n in r.kernel.values() if n}


# Instantiations no dispatcher chooses between: one form each, run by the tests named.
EXCLUDED = {
    "beta_from_theta_kernel": "single form; test_gpu_parity.py / smoke (theta -> beta)",
    "clock_probe_kernel": "timing probe of the device clock (measurement aid)",
    "loop_bump_kernel": "descriptor-loop bookkeeping; test_gpu_graph_loop.py",
    "loop_copy_kernel": "descriptor-loop bookkeeping; test_gpu_graph_loop.py",
    "loop_prime_kernel": "descriptor-loop bookkeeping; test_gpu_graph_loop.py",
    "loop_probe_set_kernel": "cross-queue timing probe (measurement aid)",
    "loop_probe_wait_kernel": "cross-queue timing probe (measurement aid)",
    "loop_wait_kernel": "descriptor-loop bookkeeping; test_gpu_graph_loop.py",
    "mb_count_kernel": "mini-batch sampler, single form; test_gpu_minibatch_oracle.py",
    "mb_draw_kernel": "mini-batch sampler, single form; test_gpu_minibatch_oracle.py",
    "mb_finish_kernel": "mini-batch sampler, single form; test_gpu_minibatch_oracle.py",
    "mb_link_kernel": "mini-batch sampler, single form; test_gpu_minibatch_oracle.py",
    "mb_write_kernel": "mini-batch sampler, single form; test_gpu_minibatch_oracle.py",
    "phi_noise_kernel": "noise pre-pass launched inside the generic update_phi form (update_phi_gen_kernel rows)",
    "pi_init_kernel": "single form; test_gpu_parity.py::test_pi_init_gamma",
    "ppx_reduce_kernel": "partial-sum reduction after every non-folding perplexity launch (ppx rows)",
    "randn_fill_kernel": "RNG test helper; test_gpu_parity.py::test_rng_seed_layout_and_normals",
    "rng_init_kernel": "stream seeding, single form; every GPU test",
    "rng_init_mixed_kernel": "stream seeding, single form; test_gpu_learner.py",
    "rpm_fetch_kernel": "pi-matrix test helper; test_gpu_parity.py::test_partitioned_matrix",
    "rpm_sum_kernel": "pi-matrix test helper; test_gpu_parity.py::test_partitioned_matrix",
    "set_build_kernel": "set-builder helper; test_gpu_setbuild.py",
    "set_clear_kernel": "set-builder helper; test_gpu_setbuild.py",
    "set_has_kernel": "set-membership helper; test_gpu_parity.py::test_cuckoo_membership",
    "sum_rows_kernel": "multi-GPU gradient reduction, single form; test_gpu_distributed.py",
    "sum_update_theta_kernel": "descriptor-loop theta step, single form; test_gpu_graph_loop.py",
    "theta_coef_kernel": "per-column gradient constants, launched before every gradient outside the descriptor loop (grads rows)",
    "update_theta_kernel": "theta step, single form; test_gpu_parity.py::test_beta_pipeline",
    "wg_normalize_kernel": "work-group primitive test helper; test_gpu_parity.py::test_wg_sum_and_normalize",
    "wg_sort_kernel<float>": "work-group primitive test helper; test_gpu_parity.py::test_wg_sort",
    "wg_sort_kernel<unsigned int>": "work-group primitive test helper; test_gpu_parity.py::test_wg_sort",
    "wg_sum_kernel<float>": "work-group primitive test helper; test_gpu_parity.py::test_wg_sum_and_normalize",
    "wg_sum_kernel<unsigned int>": "work-group primitive test helper; test_gpu_parity.py::test_wg_sum_and_normalize",
}
