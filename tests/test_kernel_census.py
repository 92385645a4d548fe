"""Kernel census (no GPU): every kernel instantiation in libammsb_hip.so is either a row of the form tables that
test_gpu_kernel_forms.py runs against the oracle (kernel_forms.ROWS) or named, with a reason, in
kernel_forms.EXCLUDED -- and every name in those tables exists in the library.

The instantiations are read from the host-side kernel handles: one data symbol per __global__ instantiation, whose
demangled name is the kernel's signature ('void (anonymous namespace)::ppx_lds_kernel<16, 2u, 64, true>(PpxArgs)',
next to a '__device_stub__' function of the same name)."""
import os
import shutil
import subprocess

import pytest

import kernel_forms as kf


def _nm():
    for tool in ("nm", "llvm-nm"):
        path = shutil.which(tool)
        if path:
            return path
    for path in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm"):
        if os.path.exists(path):
            return path
    pytest.fail("no nm / llvm-nm to list the library's symbols")


@pytest.fixture(scope="module")
def instantiations():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _capi
    out = subprocess.run([_nm(), "-C", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True)
    names = set()
    for line in out.stdout.splitlines():
        parts = line.split(" ", 2)
        if len(parts) != 3 or parts[1] not in ("d", "D", "v", "V"):
            continue  # kernel handles are data objects (local in the anonymous namespace, weak for templates)
        sym = parts[2]
        if not sym.endswith(")") or sym.startswith(("guard variable", "typeinfo", "vtable")):
            continue
        names.add(kf.normalize(sym))
    stubs = {kf.normalize(line.split(" ", 2)[2]).replace("__device_stub__", "")
             for line in out.stdout.splitlines() if "__device_stub__" in line}
    assert stubs <= names, "device stubs without a kernel handle: %s" % sorted(stubs - names)
    return names


def test_normalize():
    assert kf.normalize("void (anonymous namespace)::ppx_lds_kernel<16, 2u, 64, true>((anonymous namespace)::PpxArgs)") \
        == "ppx_lds_kernel<16, 2, 64, true>"
    assert kf.normalize("void wg_sort_kernel<unsigned int>(unsigned int const*, unsigned int*)") \
        == "wg_sort_kernel<unsigned int>"
    assert kf.normalize("(anonymous namespace)::theta_coef_kernel(float const*, float*, unsigned int)") == "theta_coef_kernel"


def test_census_finds_the_dispatched_families(instantiations):
    families = {n.split("<")[0] for n in instantiations}
    for fam in ("update_phi_kernel", "update_phi_lds_kernel", "update_phi_lds2_kernel", "update_phi_lds3_kernel",
                "update_phi_wide_kernel", "update_phi_pair_kernel", "update_phi_stream_kernel", "update_phi_gen_kernel",
                "update_pi_kernel", "beta_grads_kernel", "beta_grads_lds_kernel", "ppx_kernel", "ppx_lds_kernel",
                "sample_neighbors_wave_kernel"):
        assert fam in families, "the census misses %s: symbol parsing broken?" % fam
    assert len(instantiations) > 300


def test_every_instantiation_is_tested_or_excluded(instantiations):
    covered = kf.table_names()
    missing = sorted(instantiations - covered - set(kf.EXCLUDED))
    assert not missing, "kernel instantiations in no form table and not excluded (%d): %s" % (len(missing), missing)
    both = sorted(covered & set(kf.EXCLUDED))
    assert not both, "both in a form table and excluded: %s" % both


def test_every_table_name_exists(instantiations):
    stale = sorted(kf.table_names() - instantiations)
    assert not stale, "form-table names that are not kernel instantiations of the library: %s" % stale
    stale = sorted(set(kf.EXCLUDED) - instantiations)
    assert not stale, "exclusions that are not kernel instantiations of the library: %s" % stale
    assert all(reason.strip() for reason in kf.EXCLUDED.values())


def test_rows_are_well_formed():
    ops = {"phi", "grads", "fused", "ppx", "nbr"}
    for row in kf.ROWS:
        assert row.op in ops and len(row.shape) == 5 and row.blocks in (1, 2), row
        assert any(row.kernel.values()), row
        assert set(row.debug) <= {"phi_forms", "beta_slots"}, row
        if row.op == "phi":
            assert row.flags in ("streaming", "small"), row
