"""Host half of the community relations (include/ammsb_relate.h), no GPU: the drop-in boundary of the new library (header
== exports == signature table, the existing libraries untouched), argument errors returned before anything is launched,
the derived shares and the duplicate / nested pairs on a hand-worked case, the related-communities file written and
parsed back byte for byte, the command line's flag rules, and that no layer has a CPU path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "mcmc-ammsb-gpu_amd")
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def rl():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _relate
    _relate.load()
    return _relate


def test_header_exports_and_signature_table_agree(rl):
    hdr = open(os.path.join(ROOT, "include", "ammsb_relate.h")).read()
    declared = set(re.findall(r"\b(ammsb_relate_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 6 and declared == set(rl.SIGNATURES), declared ^ set(rl.SIGNATURES)
    lib = C.CDLL(rl.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(rl.LIB_PATH)
    assert own == declared, own ^ declared
    for macro, value in (("MAX_COLS", rl.MAX_COLS), ("MAX_TOP", rl.MAX_TOP), ("TILE", rl.TILE), ("OVERLAP", rl.OVERLAP),
                         ("JACCARD", rl.JACCARD), ("CONTAINED", rl.CONTAINED)):
        assert value == int(re.search(r"#define AMMSB_RELATE_%s (\d+)u" % macro, hdr).group(1)), macro
    assert (rl.MAX_COLS, rl.MAX_TOP, rl.TILE) == (8192, 64, 128)
    assert rl.MEASURES == {"overlap": rl.OVERLAP, "jaccard": rl.JACCARD, "contained": rl.CONTAINED}
    src = open(os.path.join(PKG, "csrc", "ammsb_relate.hip")).read()
    assert set(re.findall(r'"(relate_[a-z0-9_]+)"', src)) == set(rl.KERNEL_FORMS)
    for form in rl.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef")


def test_the_kernels_are_a_library_of_their_own(rl):
    from mcmc_ammsb_gpu_amd import _capi, _omega, _quality
    for other in (_capi, _omega, _quality):
        assert not [n for n in other.SIGNATURES if "relate" in n]
        assert b"ammsb_relate" not in open(other.LIB_PATH, "rb").read()
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name.endswith(".h") and name != "ammsb_relate.h":
            assert "ammsb_relate" not in open(os.path.join(ROOT, "include", name)).read(), name
    raw = open(rl.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    hip = open(_capi.LIB_PATH, "rb").read()
    for form in rl.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
        assert form.encode() not in hip, form
    import make_dry_run as dry
    assert dry.header_rebuilds_object("relate") and dry.csrc_all_builds("../libammsb_relate.so", "ammsb_relate.o")
    assert "ammsb_relate" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert '#include "ammsb_postfit.h"' in open(os.path.join(PKG, "csrc", "ammsb_relate.hip")).read()
    assert dry.builds(dry.commands("host", "../relate_test"), "../relate_test", "tests/cpp/relate_test.cc", "-lammsb_relate")
    assert dry.host_all_builds("../relate_test", "tests/cpp/relate_test.cc", "-lammsb_relate")
    assert "relate" in dry.DEVICE_LIBS and dry.host_links()   # every link line carries every device library


def test_argument_errors_are_returned_before_anything_is_launched(rl):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    lib = rl.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    err = lib.ammsb_relate_last_error

    def desc(K=64, rows=1000, rib=None, blocks=1):
        d = Rpm()
        for b in range(blocks):
            d.blocks[b] = p
        d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows if rib is None else rib, rows, K, blocks
        return d

    def bits(pi=True, thr=0.05, row0=0, rows=100, out=p, **kw):
        return lib.ammsb_relate_bits(C.byref(desc(**kw)) if pi else None, thr, row0, rows, out, None)

    def pairs(b=p, K=64, rows=100, ov=p):
        return lib.ammsb_relate_pairs(b, K, rows, ov, None)

    def top(ov=p, K=64, measure=1, T=4, min_overlap=1, partner=p, shared=p):
        return lib.ammsb_relate_top(ov, K, measure, T, min_overlap, partner, shared, None)

    for kw in (dict(pi=False), dict(out=None)):
        assert bits(**kw) == EINVAL and b"NULL" in err(), kw
    for thr in (-1.0, -1e-9, float("nan"), float("inf")):
        assert bits(thr=thr) == EINVAL and b"thr" in err(), thr
    for K in (0, 8193):
        assert bits(K=K) == EINVAL and b"num_cols" in err(), K
        assert pairs(K=K) == EINVAL and b"num_cols" in err(), K
        assert top(K=K) == EINVAL and b"num_cols" in err(), K
    assert bits(rows=2**32, **{}) == EINVAL
    d = desc()
    d.num_rows = d.rows_in_block = 2**32
    assert lib.ammsb_relate_bits(C.byref(d), 0.05, 0, 10, p, None) == EINVAL and b"2^32" in err()
    for row0, rows in ((0, 1001), (960, 41), (1024, 0), (2**63, 2**63), (64, 2**64 - 1)):
        assert bits(row0=row0, rows=rows) == EINVAL and b"past num_rows" in err(), (row0, rows)
    for row0 in (1, 63, 65, 100):
        assert bits(row0=row0, rows=10) == EINVAL and b"multiple of 64" in err(), row0
    assert bits(rib=400, blocks=2) == EINVAL and b"cover" in err()     # 800 < 1000 rows
    assert bits(rib=0) == EINVAL and b"cover" in err()
    d = desc(blocks=2, rib=500)
    d.blocks[1] = None
    assert lib.ammsb_relate_bits(C.byref(d), 0.05, 0, 10, p, None) == EINVAL and b"NULL" in err()
    # bad arguments are refused before the empty range is accepted, which is a valid call without a device
    assert bits(rows=0, thr=-1.0) == EINVAL and bits(rows=0, row0=3) == EINVAL
    assert bits(rows=0) == 0 and bits(row0=960, rows=0) == 0 and bits(row0=0, rows=0, rib=500, blocks=2) == 0
    assert pairs(b=None) == EINVAL and b"NULL" in err() and pairs(ov=None) == EINVAL and b"NULL" in err()
    assert pairs(rows=2**32) == EINVAL and b"2^32" in err()
    assert pairs(rows=0, K=0) == EINVAL and pairs(rows=0) == 0
    for name in ("ov", "partner", "shared"):
        assert top(**{name: None}) == EINVAL and b"NULL" in err(), name
    for measure in (3, 7, 2**32 - 1):
        assert top(measure=measure) == EINVAL and b"measure" in err(), measure
    for T in (0, 65, 2**32 - 1):
        assert top(T=T) == EINVAL and b"top" in err(), T
    assert lib.ammsb_relate_last_kernel_name() == b""


def test_bits_bytes_on_hand_shapes(rl):
    lib = rl.load()
    f = lib.ammsb_relate_bits_bytes
    assert f(1, 1) == 8 and f(64, 1) == 8 and f(65, 1) == 16 and f(65, 3) == 48 and f(128, 8192) == 2 * 8192 * 8
    assert f(2**32 - 1, 8192) == 8192 * 2**26 * 8
    assert f(0, 5) == 0 and f(10, 0) == 0 and f(10, 8193) == 0 and f(2**32, 4) == 0
    assert rl.slab_rows(1024, 1 << 30) == (1 << 30) * 8 // 1024 and rl.slab_rows(1024, 1) == 64
    assert rl.slab_rows(33, 1000) == 192 and rl.slab_rows(8192, 1 << 20) == 1024


def _hand_case(rl):
    # four communities over 12 nodes: 0 = {0..7}, 1 = {0..7} (a duplicate of 0), 2 = {0, 1} (inside both), 3 = {7..10}
    # overlap: (0,1) 8, (0,2) 2, (0,3) 1, (1,2) 2, (1,3) 1, (2,3) 0; sizes 8, 8, 2, 4
    size = [8, 8, 2, 4]
    partner = [[1, 2, 3], [0, 2, 3], [0, 1, -1], [0, 1, -1]]
    overlap = [[8, 2, 1], [8, 2, 1], [2, 2, 0], [1, 1, 0]]
    return rl.Related(0.05, "jaccard", 1, size, partner, overlap, N=12)


def test_derived_shares_duplicates_and_nested_on_a_hand_worked_case(rl):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand_case(rl)
    assert r.top == 3 and r.size.dtype == np.int64 and r.partner.dtype == np.int32 and r.overlap.dtype == np.uint32
    assert r.jaccard.dtype == r.inside.dtype == r.contained.dtype == np.float64 and r.matrix is None
    assert r.jaccard.tolist() == [[1.0, 2 / 8, 1 / 11], [1.0, 2 / 8, 1 / 11], [2 / 8, 2 / 8, 0.0], [1 / 11, 1 / 11, 0.0]]
    assert r.inside.tolist() == [[1.0, 2 / 8, 1 / 8], [1.0, 2 / 8, 1 / 8], [1.0, 1.0, 0.0], [1 / 4, 1 / 4, 0.0]]
    assert r.contained.tolist() == [[1.0, 1.0, 1 / 4], [1.0, 1.0, 1 / 4], [2 / 8, 2 / 8, 0.0], [1 / 8, 1 / 8, 0.0]]
    assert r.duplicates() == [(0, 1)] and r.duplicates(0.25) == [(0, 1), (0, 2), (1, 2)]
    assert r.duplicates(0.09) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)] and r.duplicates(1.01) == []
    assert r.nested() == [(0, 1), (0, 2), (1, 0), (1, 2)]
    assert r.nested(0.25) == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1)]
    assert "Related" in repr(r)
    for bad in (lambda: rl.Related(0.05, "cosine", 1, [1], [[-1]], [[0]]),
                lambda: rl.Related(0.05, "jaccard", 1, [1, 2], [[-1]], [[0]]),
                lambda: rl.Related(0.05, "jaccard", 1, [1], [[-1, -1]], [[0]])):
        with pytest.raises(AmmsbError):
            bad()
    assert rl.check_args("contained", 64, 0) == (rl.CONTAINED, 64, 0)
    for by, T, mo in (("cosine", 4, 1), ("jaccard", 0, 1), ("jaccard", 65, 1), ("overlap", 4, -1), ("overlap", 4, 2**32)):
        with pytest.raises(AmmsbError):
            rl.check_args(by, T, mo)


def test_the_related_communities_file_round_trips_byte_for_byte(rl, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand_case(rl)
    path, again = str(tmp_path / "related.txt"), str(tmp_path / "again.txt")
    rl.write_related(path, 12, r)
    assert open(path).read() == ("# 12 4 0.0500000007 jaccard 3 1\n0 8 3 1 8 2 2 3 1\n1 8 3 0 8 2 2 3 1\n2 2 2 0 2 1 2\n"
                                 "3 4 2 0 1 1 1\n")
    N, back = rl.read_related(path)
    assert N == 12 and back.by == "jaccard" and back.top == 3 and back.min_overlap == 1
    assert back.threshold == float(np.float32(0.05))
    for name in ("size", "partner", "overlap", "jaccard", "inside", "contained"):
        assert np.array_equal(getattr(back, name), getattr(r, name)), name
    rl.write_related(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # counts past 2^31 and an N past 2^32 keep their digits
    big = rl.Related(0.0, "overlap", 3, [4_000_000_000, 3_000_000_000], [[1], [0]], [[2_999_999_999], [2_999_999_999]])
    rl.write_related(path, 5_000_000_000, big)
    assert open(path).read() == "# 5000000000 2 0 overlap 1 3\n0 4000000000 1 1 2999999999\n1 3000000000 1 0 2999999999\n"
    N, back = rl.read_related(path)
    assert N == 5_000_000_000 and back.overlap.tolist() == [[2_999_999_999]] * 2 and back.size.tolist() == big.size.tolist()
    good = "# 12 2 0.05 contained 2 1\n0 8 1 1 2\n1 2 1 0 2\n"
    open(path, "w").write(good)
    assert rl.read_related(path)[1].contained.tolist() == [[1.0, 0.0], [0.25, 0.0]]
    for bad in ("", "# 1 2\n", good.replace("contained", "cosine"), good.replace("\n1 2 1", "\n2 2 1"), good.replace("0 8 1 1 2", "0 8 1 1"),
                good.replace("0 8 1 1 2", "0 8 3 1 2 1 2 1 2"), good.replace("0 8 1 1 2", "0 8 1 x 2"), good.replace("1 2 1 0 2", "1 2 1 2 2"),
                good.replace("1 2 1 0 2", "1 2 1 -1 2"), good.splitlines()[0] + "\n0 8 0\n", good + "2 1 0\n", good.replace("# 12", "# twelve"),
                good.replace("contained 2", "contained 65")):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            rl.read_related(path)


def test_no_cpu_path_without_a_gpu(rl, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner

    class Cfg:
        N, K = 50, 8
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    lrn.cfg = Cfg()
    for call in (lambda: lrn.CommunityOverlap(), lambda: lrn.CommunityOverlap(0.01, max_bytes=64),
                 lambda: lrn.RelatedCommunities(), lambda: lrn.RelatedCommunities(0.1, 64, "contained", 0, 1, True),
                 lambda: lrn.RelatedCommunities(by="overlap", top=1)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    for bad in (lambda: lrn.CommunityOverlap(-1.0), lambda: lrn.CommunityOverlap(float("nan")), lambda: lrn.CommunityOverlap(max_bytes=0),
                lambda: lrn.RelatedCommunities(threshold=float("inf")), lambda: lrn.RelatedCommunities(top=0),
                lambda: lrn.RelatedCommunities(top=65), lambda: lrn.RelatedCommunities(by="cosine"),
                lambda: lrn.RelatedCommunities(min_overlap=-1)):
        with pytest.raises(AmmsbError) as e:
            bad()
        assert "no CPU path" not in str(e.value)
    assert hasattr(ops, "CommunityRelations")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(rl, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    out = str(tmp_path / "out.txt")
    base = ["-f", missing, "-k", "8"]
    o = ["--related-communities-out", out]
    for extra in (["--related-communities-threshold", "0.1"],                    # a modifier without -out
                  ["--related-communities-top", "4"],
                  ["--related-communities-by", "jaccard"],
                  o + ["--related-communities-by", "cosine"], o + ["--related-communities-by", "Jaccard"],
                  o + ["--related-communities-top", "0"], o + ["--related-communities-top", "65"],
                  o + ["--related-communities-top", "-3"], o + ["--related-communities-top", "four"],
                  o + ["--related-communities-top", "4.5"],
                  o + ["--related-communities-threshold", "-0.1"], o + ["--related-communities-threshold", "inf"],
                  o + ["--related-communities-threshold", "1e39"],                  # not finite as a binary32
                  o + ["--related-communities-threshold", "nan"], o + ["--related-communities-threshold", "half"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, (extra, r.stderr[-500:])
        assert "need" in r.stderr or "must be" in r.stderr or "is invalid" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (o, o + ["--related-communities-by", "overlap"], o + ["--related-communities-by", "contained", "--related-communities-top", "64"],
                  o + ["--related-communities-threshold", "0", "--related-communities-top", "1", "--related-communities-by", "jaccard"],
                  o + ["--community-quality-out", out + "2"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
