"""Every update_phi and beta-gradient form on BOTH sides of its exact-division branch, against the oracle bit for bit.

The rows are the phi, grads and fused rows of kernel_forms.ROWS, run by `kernel_forms_child.py GROUP edges FIRST LAST` on
the inputs of division_edges.py (trained / denormal pi, beta, phi_sum, den, lo and probs_sum on and beyond their limits,
all of them mixed; for the gradient a node-strategy edge list laid out for 64 slots).  The child asserts, per row: the
coverage conditions of the input (test_division_edges_host.py asserts them without a GPU), the exact instantiation, and
phi_vec, the stream states, the pi rows and phi_sum -- or the gradient, against the oracle's per-edge terms summed in the
order of 64 slots and against the default form's gradient -- bit for bit.

As in test_gpu_kernel_forms.py the AMMSB_* switches are read once per process, so every group runs in children of its
own environment, one at a time.  A group is cut into ranges of CHUNK rows so that a test stays at a few seconds.

Timeouts.  The existing mode (`kernel_forms_child.py 0 -`: two problems and four update_phi per phi row) was timed on the
parent commit on an MI355X: 4.6 s for the 147 rows of the default group after 2 s of start-up, 0.03 s per row.  That is
too little to scale: the edges mode spends its time on the host (per row seven cases, each with the oracle, the builders
and the classification), about 0.25 s per row and 5 s for a row of 9000 nodes, measured with this test (ranges of 12 rows
took 2.4 - 5.4 s, a 9000-node row 7.3 s, start-up included).  A range therefore gets 3 x ROW_S (3 x BIG_ROW_S) per row
-- the factor 3 on the edges mode's own time, which is more than 3 x the existing mode's -- plus CHILD_START for the
interpreter, torch and the libraries on a loaded machine.
"""
import os
import subprocess
import sys

import pytest

import kernel_forms as kf
import kernel_forms_child as kc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "kernel_forms_child.py")
GROUPS = kf.groups()
CHUNK = 12
CHILD_START = 60.0
ROW_S, BIG_ROW_S = 0.4, 6.0  # seconds per row of the edges mode (see above); BIG: thousands of mini-batch nodes


def _big(row):
    return row.op == "phi" and kc.edge_nodes(row) > 512


def _ranges():
    out = []
    for g, (env, rows) in enumerate(GROUPS):
        mine = [(i, r) for i, r in rows if r.op in ("phi", "grads", "fused")]
        cur = []
        for i, r in mine:
            if _big(r):  # (thousands of nodes: a range of its own)
                out.append((g, [(i, r)]))
                continue
            if len(cur) == CHUNK:
                out.append((g, cur))
                cur = []
            cur.append((i, r))
        if cur:
            out.append((g, cur))
    return out


RANGES = _ranges()


def _env(index):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("AMMSB_PHI_", "AMMSB_BETA_", "AMMSB_PPX_", "AMMSB_NBR_"))}
    env.update(dict(GROUPS[index][0]))
    return env


def _child(index, args, seconds):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no fallback path exists)")
    out = subprocess.run([sys.executable, CHILD, str(index)] + args, env=_env(index), capture_output=True, text=True,
                         timeout=seconds, cwd=os.path.dirname(HERE))
    if out.returncode != 0:
        pytest.fail("group %r %s (exit %d):\n%s\n%s" % (GROUPS[index][0], args, out.returncode, out.stdout[-2000:],
                                                        out.stderr[-5000:]), pytrace=False)
    assert "group ok" in out.stdout
    return out.stdout


@pytest.fixture(scope="module")
def default_edge_grads(tmp_path_factory):
    """the default forms' gradients of the inputs of every gradient row outside the default group"""
    path = str(tmp_path_factory.mktemp("edges") / "default_edge_grads.npz")
    rows = sum(1 for _, rs in GROUPS[1:] for _, r in rs if r.op == "grads")
    _child(0, ["edge-refs", path], CHILD_START + 3 * ROW_S * rows)
    return path


@pytest.mark.parametrize("which", range(len(RANGES)),
                         ids=["%d-%d-%d" % (g, rows[0][0], rows[-1][0]) for g, rows in RANGES])
def test_forms_on_both_division_paths(request, which):
    index, rows = RANGES[which]
    args = ["edges", str(rows[0][0]), str(rows[-1][0])]
    if index != 0 and any(r.op == "grads" for _, r in rows):
        args.append(request.getfixturevalue("default_edge_grads"))
    seconds = CHILD_START + 3 * sum(BIG_ROW_S if _big(r) else ROW_S for _, r in rows)
    out = _child(index, args, seconds)
    done = {int(line.split()[2]) for line in out.splitlines() if line.startswith("edge ok ")}
    assert done == {i for i, _ in rows}, "rows not run: %s" % sorted({i for i, _ in rows} - done)
