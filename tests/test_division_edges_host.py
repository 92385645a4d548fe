"""CPU checks of the inputs of division_edges.py (no GPU): that they reach both sides of the exact-division branch at
every shape test_gpu_division_edges.py runs, and that they would expose a form that lost a guard.

Coverage: for every distinct (operation, state shape) among the phi, grads and fused rows of kernel_forms.ROWS and every
case, the conditions of division_edges.check_phi_coverage / check_grad_coverage hold (the GPU child asserts them again on
the state it uploads).  Counts of "at least 8" are scaled down where a launch is too small to hold them
(division_edges.need): a row of 6 nodes with 3 neighbours has 6 two-row steps in all; wherever a launch can hold 8 of
each kind twice over, the count is a plain 8.

Sensitivity (tests/cpp/div_guard_check.c): the operand pairs of both divisions, probs / probs_sum and then the quotient
/ den, as the float32 restatement of the oracle's arithmetic gives them, go through the two unguarded tails
(three-instruction Markstein, five-instruction Newton) and are compared with IEEE `x / d`.
  * decided-fast rows: no quotient differs -- the guards are sufficient on these inputs;
  * rows slow by the `lo` guard (a |probs| below 2^-100) and rows slow by the `den` guard: quotients DO differ, so a
    form that dropped either guard would fail the bit-for-bit comparison on these inputs.
  * `beta_safe` and the `probs_sum` range: no reachable operand was found on which dropping the guard alone changes a
    quotient (beta only bounds tt, whose consequences the `lo` guard sees as well; probs_sum in [2^-35, 64] with legal
    numerators keeps every remainder representable).  The test prints their counts and asserts nothing of them: these
    two guards are covered only by the both-sides run on the device.
"""
import os
import subprocess

import numpy as np
import pytest

import division_edges as de
import kernel_forms as kf
import kernel_forms_child as kc

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-7


def _shapes(op):
    seen = {}
    for i, r in enumerate(kf.ROWS):
        if r.op == op:
            key = kc.edge_state_shape(r) + ((r.shape[4],) if op == "fused" else ())
            seen.setdefault(key, i)
    return sorted(seen)


@pytest.fixture(scope="module")
def states(orc):
    cache = {}

    def get(N, K, n, nodes, deg=kc.EDGE_DEG):
        key = (N, K, n, nodes, deg)
        if key not in cache:
            cache.clear()  # (one state at a time: the large ones are 20 MB each)
            st = de.host_state(orc, N, K, n, nodes, deg=deg)
            cache[key] = (st, de.Saved(st))
        st, saved = cache[key]
        saved.restore(st)
        return st
    return get


@pytest.mark.parametrize("shape", _shapes("phi"), ids=lambda s: "x".join(map(str, s)))
def test_phi_cases_reach_both_sides(orc, states, shape):
    for case in de.CASES:
        st = states(*shape)
        assert abs(orc.make_params(*shape[:3]).epsilon - EPS) < 1e-12
        kc.phi_case(st, case, orc.make_params(*shape[:3]).epsilon)


@pytest.mark.parametrize("shape", _shapes("grads"), ids=lambda s: "x".join(map(str, s)))
def test_gradient_lists_reach_the_six_step_classes(orc, states, shape):
    p = orc.make_params(*shape[:3])
    for case in de.GRAD_CASES:
        kc.grad_case(orc, p, states(*shape, deg=kc.grad_deg(shape[0])), case, p.epsilon, False, 64)


@pytest.mark.parametrize("shape", _shapes("fused"), ids=lambda s: "x".join(map(str, s)))
def test_fused_lists_reach_the_six_step_classes(orc, states, shape):
    p = orc.make_params(*shape[:3])
    for case in de.GRAD_CASES:
        kc.grad_case(orc, p, states(*shape[:4], deg=kc.grad_deg(shape[0])), case, p.epsilon, True, shape[4])


# ------------------------------------------------------------------------------------------------- sensitivity

@pytest.fixture(scope="module")
def guard_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("div") / "div_guard_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "cpp", "div_guard_check.c"), "-lm"],
                   check=True)

    def run(pairs, path):
        np.ascontiguousarray(pairs, dtype=np.float32).tofile(path)
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split()
        assert out[0] == "pairs" and int(out[1]) == len(pairs), out
        return int(out[3]), int(out[5])
    return run


def _pairs(cls, pick):
    """(x, d) of both divisions for the (node, row, column) triples pick(i) selects: [rows, K] masks per node"""
    out = []
    for i, (probs, psum, den) in enumerate(cls.operands):
        mask = pick(i, probs)
        if not mask.any():
            continue
        with np.errstate(all="ignore"):
            q = (probs / psum[:, None]).astype(np.float32)
        d1 = np.broadcast_to(psum[:, None], probs.shape)
        d2 = np.broadcast_to(den[None, :], probs.shape)
        out.append(np.stack([probs[mask], d1[mask]], 1))
        out.append(np.stack([q[mask], d2[mask]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.float32)


@pytest.mark.parametrize("K,n", [(256, 32), (1024, 16)])
def test_slow_rows_would_expose_a_lost_guard(orc, states, guard_check, tmp_path, K, n):
    """see the module docstring; counts are printed per case (pytest -s)"""
    N, nodes = 1024, 96
    eps = orc.make_params(N, K, n).epsilon
    total = {"lo": [0, 0, 0], "den": [0, 0, 0], "psum": [0, 0, 0], "fast": [0, 0, 0]}
    for case in ("trained", "denormal", "den_lo_limits", "psum_limits"):
        st = states(N, K, n, nodes)
        de.apply_case(st, case, eps)
        c = de.classify_phi(st, eps, keep_operands=True)
        node_ok = ~(c.phi_sum_fail | c.den_fail_all)
        with np.errstate(all="ignore"):
            sel = {
                # rows slow by lo alone: the columns below 2^-100
                "lo": lambda i, probs: (node_ok[i] & c.lo_fail_all[i] & (c.psum[i] == 0))[:, None] & (np.abs(probs) < de.PROBS_LO),
                # nodes slow by den: the columns whose den is out of range (rows whose probs_sum passes)
                "den": lambda i, probs: np.broadcast_to(((not c.phi_sum_fail[i]) & (c.psum[i] == 0))[:, None], probs.shape)
                & ~de.in_range(c.operands[i][2], de.DEN_LO, de.DEN_HI)[None, :],
                "psum": lambda i, probs: np.broadcast_to((node_ok[i] & ~c.lo_fail_all[i] & (c.psum[i] == 1))[:, None], probs.shape),
                "fast": lambda i, probs: np.broadcast_to((node_ok[i] & ~c.lo_fail_all[i] & (c.psum[i] == 0))[:, None], probs.shape),
            }
            for what, pick in sel.items():
                pairs = _pairs(c, pick)
                t3, t5 = guard_check(pairs, str(tmp_path / "pairs.bin")) if len(pairs) else (0, 0)
                print("K=%d %s %s: %d pairs, %d / %d quotients differ (3- / 5-instruction tail)" % (K, case, what, len(pairs), t3, t5))
                for j, v in enumerate((len(pairs), t3, t5)):
                    total[what][j] += v
    assert total["fast"][0] > 10000 and total["fast"][1:] == [0, 0], total
    assert total["lo"][1] > 0 and total["lo"][2] > 0, total
    assert total["den"][1] > 0 and total["den"][2] > 0, total
