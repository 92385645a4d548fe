"""Every kernel form the dispatchers can select, against the oracle, with the exact instantiation asserted.

The rows are kernel_forms.ROWS (test_kernel_census.py checks, without a GPU, that they and kernel_forms.EXCLUDED name
every instantiation in the library).  The AMMSB_* switches are read once per process, so the rows run grouped by
environment, one child process per group, one after the other (kernel_forms_child.py); in-process switches
(ammsb_debug_phi_forms, AMMSB_BETA_SLOTS) are set and reset around their row inside the default group's child.  The
default group runs first and saves the default-form gradients that the gradient rows of the other groups must equal
bit for bit.

Bars, per operation: update_phi / update_pi -- noise on and off, two steps, phi_vec, the stream states, the pi rows and
phi_sum bit for bit; gradient -- 1e-5 relative of the oracle's f64 sum, and the default form's bits where the slot
count is kept; update_pi + gradient in one launch -- the separate launches' pi rows, phi_sum and gradient bit for bit;
perplexity -- three calls, then two calculators on one context in turn, per-edge state bit for bit, sums within 1e-12,
counts exact; neighbour sampler -- table, packed output and streams bit for bit.
"""
import os
import subprocess
import sys

import pytest

import kernel_forms as kf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "kernel_forms_child.py")
GROUPS = kf.groups()


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no fallback path exists)")


@pytest.fixture(scope="module")
def default_grads(tmp_path_factory):
    """runs the default group (first) and returns the file of default-form gradients it saved"""
    _need_gpu()
    path = str(tmp_path_factory.mktemp("forms") / "default_grads.npz")
    env, rows = GROUPS[0]
    assert env == ()
    _run(0, rows, ["-", path])
    return path


def _run(index, rows, extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("AMMSB_PHI_", "AMMSB_BETA_", "AMMSB_PPX_", "AMMSB_NBR_"))}
    env.update(dict(GROUPS[index][0]))
    out = subprocess.run([sys.executable, CHILD, str(index)] + extra, env=env, capture_output=True, text=True,
                         timeout=900, cwd=os.path.dirname(HERE))
    if out.returncode != 0:
        pytest.fail("group %r (exit %d):\n%s\n%s" % (GROUPS[index][0], out.returncode, out.stdout[-2000:], out.stderr[-5000:]),
                    pytrace=False)
    done = {int(line.split()[2]) for line in out.stdout.splitlines() if line.startswith("row ok ")}
    assert done == {i for i, _ in rows}, "rows not run: %s" % sorted({i for i, _ in rows} - done)
    assert "group ok" in out.stdout


def test_default_environment_forms(default_grads):
    assert os.path.exists(default_grads)


@pytest.mark.parametrize("index", range(1, len(GROUPS)), ids=["+".join("%s=%s" % kv for kv in GROUPS[i][0])
                                                                for i in range(1, len(GROUPS))])
def test_switched_forms(default_grads, index):
    _run(index, GROUPS[index][1], [default_grads])


def test_pi_larger_than_256mb():
    """N = 70 000, K = 1024: pi is 287 MB in one block, so update_phi requests neighbour rows non-temporally (rows_nt)
    and the fused update_pi + gradient launch may store pi rows non-temporally (ammsb_debug_beta_pi_nt).  300 mini-batch
    nodes: phi_vec and their pi rows bit for bit against the oracle; the fused launch with the stores on and off:
    pi rows and gradients bit-identical, the gradient within 1e-5 of the oracle's f64 sum."""
    _need_gpu()
    import kernel_forms_child as kc
    r = kc.Runner()
    assert 70000 * 1024 * 4 > 256 << 20
    row = kf.Row((), {}, "fused", (70000, 1024, 32, 299, 64), 1, "",
                 {"update_phi": kf.lds(16, 1, 2, 1, 64, 1), "beta_grads": "beta_grads_lds_kernel<16, 1, true, 64>"})
    r.fused(row, pi_nt=[1, 0])
