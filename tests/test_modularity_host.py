"""Host half of the overlapping modularity (include/ammsb_modularity.h), no GPU: the derived measures from hand-made
integers against a fractions.Fraction statement (a partition gives Newman's modularity, one community that holds every
node gives 0 exactly, no valid key gives -1), the modularity file written and parsed back byte for byte, argument errors
returned before anything is launched, the drop-in boundary of the new library (header == exports == signature table,
built by build()), the command line's flag rules, and that no layer has a CPU path."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "mcmc-ammsb-gpu_amd")
EINVAL = -1  # AMMSB_EINVAL
F = 1 << 62


@pytest.fixture(scope="module")
def md():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _modularity
    _modularity.load()
    return _modularity


def _sums(members, keys, N):
    """the header's integers from a cover given as sets of nodes -> (IN, SV, m, skipped, deg)"""
    K = len(members)
    O = [sum(a in c for c in members) for a in range(N)]
    deg, IN, m, skipped = [0] * N, [0] * K, 0, 0
    for a, b in keys:
        if a >= N or b >= N:
            skipped += 1
            continue
        m += 1
        deg[a] += 1
        deg[b] += 1
        for k, c in enumerate(members):
            if a in c and b in c:
                IN[k] += F // (O[a] * O[b])
    SV = [sum(deg[a] * (F // O[a]) for a in c) for c in members]
    return IN, SV, m, skipped, deg


def _eq_fraction(members, keys, N):
    """the unquantised EQ per community as rationals"""
    O = [sum(a in c for c in members) for a in range(N)]
    good = [(a, b) for a, b in keys if a < N and b < N]
    m, deg = len(good), [0] * N
    for a, b in good:
        deg[a] += 1
        deg[b] += 1
    out = []
    for c in members:
        i = sum(Fraction(1, O[a] * O[b]) for a, b in good if a in c and b in c)
        s = sum(Fraction(deg[a], O[a]) for a in c)
        out.append((2 * i - s * s / (2 * m)) / (2 * m))
    return out


def test_derived_measures_agree_with_fractions_on_hand_made_integers(md):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    # two triangles joined by one link, as a partition: Newman's modularity 2 (3/7 - (7/14)^2) = 5/14
    keys = [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]
    part = [{0, 1, 2}, {3, 4, 5}]
    IN, SV, m, skipped, deg = _sums(part, keys, 6)
    assert IN == [3 * F, 3 * F] and SV == [7 * F, 7 * F] and (m, skipped) == (7, 0)
    r = md.Modularity(0.05, IN, SV, m, skipped, deg, N=6)
    assert r.q_each.dtype == r.in_each.dtype == r.s_each.dtype == np.float64 and r.internal.dtype == object
    assert r.in_each.tolist() == [3.0, 3.0] and r.s_each.tolist() == [7.0, 7.0]
    newman = [Fraction(3, 7) - Fraction(7, 14) ** 2] * 2
    assert _eq_fraction(part, keys, 6) == newman and sum(newman) == Fraction(5, 14)
    assert r.q_each.tolist() == [(2.0 * 3.0 - 7.0 * 7.0 / 14.0) / 14.0] * 2 and r.q == r.q_each[0] + r.q_each[1]
    assert abs(r.q - 5 / 14) <= 2 ** -52 and r.degree.tolist() == [2, 2, 3, 3, 2, 2] and r.degree.dtype == np.uint32
    # one community that holds every node: in = m, s = 2m, q = (2m - 4m^2 / 2m) / 2m = 0 exactly
    IN, SV, m, skipped, _ = _sums([set(range(6))], keys + [(1, 1), (0, 1), (9, 0)], 6)
    r = md.Modularity(0.05, IN, SV, m, skipped)
    assert (m, skipped) == (9, 1) and r.q == 0.0 and r.q_each.tolist() == [0.0] and r.degree is None
    # an overlapping cover: node 2 and node 3 in both; against the rationals within the float64 rounding of the four
    # operations (the fixed-point truncation is below 4 * 2^-62 of a term here)
    cover = [{0, 1, 2, 3}, {2, 3, 4, 5}, set()]
    IN, SV, m, skipped, _ = _sums(cover, keys, 6)
    r = md.Modularity(0.05, IN, SV, m, skipped)
    want = _eq_fraction(cover, keys, 6)
    for k in range(3):
        bound = 8 * 2.0 ** -53 * float((2 * Fraction(IN[k], F) + Fraction(SV[k], F) ** 2 / (2 * m)) / (2 * m)) + 2.0 ** -36 * abs(float(want[k]))
        assert abs(Fraction(r.q_each[k]) - want[k]) <= bound, k
    assert r.q_each[2] == 0.0 and r.q > 0
    # no valid key: -1 everywhere
    r = md.Modularity(0.05, [0, 0], [0, 0], 0, 3)
    assert r.q == -1.0 and r.q_each.tolist() == [-1.0, -1.0] and r.in_each.tolist() == [0.0, 0.0]
    # the conversion rounds once, to nearest even: 2^53 + 1 is a tie, 2^53 + 3 rounds up; a value past 2^64 keeps its high word
    r = md.Modularity(0.0, [2 ** 53 + 1, 2 ** 53 + 3, (5 << 64) | 7], [0, 0, 0], 1, 0)
    assert r.in_each.tolist() == [2.0 ** -9, (2.0 ** 53 + 4) * 2.0 ** -62, float((5 << 64) | 7) * 2.0 ** -62]
    assert md.wide(np.array([7, 5, 2 ** 64 - 1, 0], dtype=np.uint64)).tolist() == [(5 << 64) | 7, 2 ** 64 - 1]
    assert "Modularity" in repr(r)
    for bad in (lambda: md.Modularity(0.05, [0], [0, 0], 1, 0), lambda: md.Modularity(0.05, [-1], [0], 1, 0),
                lambda: md.Modularity(0.05, [0], [2 ** 128], 1, 0), lambda: md.Modularity(0.05, [0], [0], -1, 0)):
        with pytest.raises(AmmsbError):
            bad()


def test_the_modularity_file_round_trips_byte_for_byte(md, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    keys = [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3), (7, 1)]
    IN, SV, m, skipped, _ = _sums([{0, 1, 2, 3}, {2, 3, 4, 5}, set()], keys, 6)
    r = md.Modularity(0.05, IN, SV, m, skipped, N=6)
    path, again = str(tmp_path / "modularity.txt"), str(tmp_path / "again.txt")
    md.write_modularity(path, 6, r)
    lines = open(path).read().splitlines()
    assert lines[0] == "# 6 3 8 0.0500000007 1 %.17g" % r.q and len(lines) == 4
    assert lines[1].split()[4] == "%032x" % IN[0] and len(lines[1].split()[5]) == 32 and lines[3].split()[1:] == ["0", "0", "0", "0" * 32, "0" * 32]
    N, back = md.read_modularity(path)
    assert N == 6 and (back.links, back.skipped) == (7, 1) and back.threshold == float(np.float32(0.05)) and back.q == r.q
    assert back.internal.tolist() == r.internal.tolist() and back.volume.tolist() == r.volume.tolist()
    assert np.array_equal(back.q_each, r.q_each)
    md.write_modularity(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # m = 0, and sums past 2^64 keep their digits
    big = md.Modularity(0.0, [(3 << 64) | 5], [(1 << 127) | 1], 0, 2, N=5_000_000_000)
    md.write_modularity(path, 5_000_000_000, big)
    assert open(path).read() == "# 5000000000 1 2 0 2 -1\n0 -1 %.17g %.17g %032x %032x\n" % (big.in_each[0], big.s_each[0], (3 << 64) | 5, (1 << 127) | 1)
    N, back = md.read_modularity(path)
    assert N == 5_000_000_000 and back.internal.tolist() == [(3 << 64) | 5] and back.q == -1.0
    md.write_modularity(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    md.write_modularity(path, 6, r)
    good = open(path).read()
    first = good.splitlines()[1]
    for bad in ("", "# 1 2\n", good.replace("# 6 3", "# six 3"), good.replace("# 6 3 8", "# 6 4 8"), good.replace("\n1 ", "\n2 "),
                good.replace(first, first[:-1]), good.replace(first, first + " 1"), good.replace(first, first[:-1] + "g"),
                good + "3 0 0 0 %s %s\n" % ("0" * 32, "0" * 32), good.replace(" 1 %.17g" % r.q, " 9 %.17g" % r.q),
                good.replace(" %.17g\n" % r.q, " 0.25\n"), good.replace(first, first.replace(first.split()[4], "%032x" % (2 * IN[0])))):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            md.read_modularity(path)


def test_argument_errors_are_returned_before_anything_is_launched(md):
    lib = md.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    err = lib.ammsb_modularity_last_error

    def edges(m=p, rows=1000, K=64, e=p, n=10, d=p, i=p, c=p):
        return lib.ammsb_modularity_edges(m, rows, K, e, n, d, i, c, None)

    def nodes(m=p, rows=1000, K=64, d=p, v=p):
        return lib.ammsb_modularity_nodes(m, rows, K, d, v, None)

    for name in ("m", "e", "d", "i", "c"):
        assert edges(**{name: None}) == EINVAL and b"NULL" in err(), name
    for name in ("m", "d", "v"):
        assert nodes(**{name: None}) == EINVAL and b"NULL" in err(), name
    for K in (0, 8193, 2**32 - 1):
        assert edges(K=K) == EINVAL and b"num_cols" in err(), K
        assert edges(K=K, n=0) == EINVAL and b"num_cols" in err(), K
        assert nodes(K=K) == EINVAL and b"num_cols" in err(), K
    assert edges(rows=2**32) == EINVAL and b"2^32" in err() and nodes(rows=2**32) == EINVAL and b"2^32" in err()
    for n in (2**31, 2**31 + 1, 2**40):
        assert edges(n=n) == EINVAL and b"2^31" in err(), n
    for name, by in (("d", 2), ("i", 4), ("c", 4), ("d", 1)):
        assert edges(**{name: p + by}) == EINVAL and b"aligned" in err(), name
        assert edges(**{name: p + by}, n=0) == EINVAL, name
    assert nodes(d=p + 2) == EINVAL and b"aligned" in err() and nodes(v=p + 4) == EINVAL and b"aligned" in err()
    # n == 0 needs neither a mask nor a list nor a device; no node launches nothing
    assert edges(n=0) == 0 and edges(m=None, e=None, n=0) == 0
    assert edges(d=None, n=0) == EINVAL and edges(i=None, n=0) == EINVAL and edges(c=None, n=0) == EINVAL
    assert nodes(rows=0) == 0 and nodes(m=None, d=None, rows=0) == 0 and nodes(v=None, rows=0) == EINVAL
    assert lib.ammsb_modularity_last_kernel_name() == b""
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    assert md.check_keys(0) == 0 and md.check_keys(2**31 - 1) == 2**31 - 1
    for n in (2**31, 2**40, -1):
        with pytest.raises(AmmsbError):
            md.check_keys(n)
    assert md.check_threshold(0) == 0.0 and md.check_threshold(0.05) == float(np.float32(0.05))
    for thr in (-1e-9, float("nan"), float("inf"), 1e39):
        with pytest.raises(AmmsbError):
            md.check_threshold(thr)


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(md):
    from mcmc_ammsb_gpu_amd import _capi, _connect, _quality
    hdr = open(os.path.join(ROOT, "include", "ammsb_modularity.h")).read()
    declared = set(re.findall(r"\b(ammsb_modularity_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 4 and declared == set(md.SIGNATURES), declared ^ set(md.SIGNATURES)
    assert os.path.exists(md.LIB_PATH) and os.path.basename(md.LIB_PATH) == "libammsb_modularity.so"
    lib = C.CDLL(md.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(md.LIB_PATH)
    assert own == declared, own ^ declared
    for macro, value in (("MAX_COLS", md.MAX_COLS), ("W1_MAX_COLS", md.W1_MAX_COLS), ("FRAC_BITS", md.FRAC_BITS)):
        assert value == int(re.search(r"#define AMMSB_MODULARITY_%s (\d+)u" % macro, hdr).group(1)), macro
    assert md.MAX_EDGES == int(re.search(r"#define AMMSB_MODULARITY_MAX_EDGES (\d+)ull", hdr).group(1)) == 2**31
    src = open(os.path.join(PKG, "csrc", "ammsb_modularity.hip")).read()
    assert set(re.findall(r'"(modularity_[a-z0-9_]+)"', src)) == set(md.KERNEL_FORMS)
    for form in md.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef") and "Rounding." in hdr and "2^-36" in hdr
    # a library of its own: the existing ones do not know it, and its kernels are gfx950 code objects
    for other in (_capi, _quality, _connect):
        assert not [n for n in other.SIGNATURES if "modularity" in n]
        assert b"ammsb_modularity" not in open(other.LIB_PATH, "rb").read()
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name.endswith(".h") and name != "ammsb_modularity.h":
            assert "ammsb_modularity" not in open(os.path.join(ROOT, "include", name)).read(), name
    raw = open(md.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for form in md.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
    assert '#include "ammsb_postfit.h"' in src
    import make_dry_run as dry
    assert dry.header_rebuilds_object("modularity") and dry.csrc_all_builds("../libammsb_modularity.so", "ammsb_modularity.o")
    assert "ammsb_modularity" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert dry.host_all_builds("../modularity_test", "tests/cpp/modularity_test.cc", "-lammsb_modularity")
    for exe in ("modularity_test", "ammsb_main"):
        assert os.access(os.path.join(PKG, exe), os.X_OK), exe


def test_no_cpu_path_without_a_gpu(md, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner

    class Cfg:
        N, K = 50, 8
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    lrn.cfg = Cfg()
    for call in (lambda: lrn.Modularity(), lambda: lrn.Modularity(0.01, edges=[1, 2]), lambda: lrn.Modularity(degree=True)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    for bad in (lambda: lrn.Modularity(-1.0), lambda: lrn.Modularity(float("nan")), lambda: lrn.Modularity(threshold=float("inf"))):
        with pytest.raises(AmmsbError) as e:
            bad()
        assert "no CPU path" not in str(e.value)
    assert hasattr(ops, "Modularity")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(md, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    out = str(tmp_path / "out.txt")
    base = ["-f", missing, "-k", "8"]
    o = ["--modularity-out", out]
    for extra in (["--modularity-threshold", "0.1"],                    # the threshold without -out
                  o + ["--modularity-threshold", "-0.1"], o + ["--modularity-threshold", "inf"],
                  o + ["--modularity-threshold", "1e39"],                  # not finite as a binary32
                  o + ["--modularity-threshold", "nan"], o + ["--modularity-threshold", "half"],
                  o + ["--modularity-threshold", "0.1x"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, (extra, r.stderr[-500:])
        assert "need" in r.stderr or "must be" in r.stderr or "is invalid" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (o, o + ["--modularity-threshold", "0"], o + ["--modularity-threshold", "0.3", "--community-quality-out", out + "2"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
