"""The helpers nine GPU suites rest on (postfit_support.py) can fail: the checkpoint record parser and the buffer comparison
on hand-built byte strings, the child's dispatcher, and the launcher on children that go wrong in each of the three ways it
must catch.  No device, no built library."""
import struct
import sys
import types

import pytest

import postfit_support as ps


def stream(recs):
    return b"".join(struct.pack("<Q", len(r)) + r for r in recs)


LONG = [bytes([i]) * 300 for i in range(1, 7)]           # six records that count as buffers (>= 200 bytes)
HEAD = b"\x0a\xd0\x0f"                                   # what precedes the buffer's bytes in a `partly` record
PARTLY = (8, 2000, 800)                                  # record 8: a buffer of 2000 bytes, 800 of them written


def checkpoint(short=(b"\x08\x01", b"\x08\x02"), tail=b"\xee" * 1200, written=b"\x11" * 800):
    return stream(list(short) + LONG + [HEAD + written + tail])


def test_records_round_trip_and_reject_a_truncated_stream():
    recs = [b"", b"abc", bytes(range(256)) * 3]
    data = stream(recs)
    assert ps.records(data) == recs and ps.records(b"") == []
    with pytest.raises(AssertionError):
        ps.records(data[:-1])
    with pytest.raises((AssertionError, struct.error)):
        ps.records(data + b"\x01\x00\x00")


def test_same_buffers_accepts_what_may_differ():
    ps.same_buffers(checkpoint(), checkpoint(), "equal", [PARTLY])
    ps.same_buffers(checkpoint(), checkpoint(tail=b"\x77" * 1200), "past valid", [PARTLY])
    ps.same_buffers(checkpoint(), checkpoint(short=(b"\x08\x81\x01", b"\x08")), "short records of other lengths", [PARTLY])


def flip(data, at):
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


def test_same_buffers_raises_on_what_must_not():
    good = checkpoint()
    start_of_long = 2 * (8 + 2) + 8                       # the first byte of LONG[0]
    with pytest.raises(AssertionError, match="record 2"):
        ps.same_buffers(good, flip(good, start_of_long + 150), "a long record", [PARTLY])
    start_of_partly = len(good) - 2000
    with pytest.raises(AssertionError, match="record 8"):
        ps.same_buffers(good, flip(good, start_of_partly + 799), "inside valid", [PARTLY])
    ps.same_buffers(good, flip(good, start_of_partly + 800), "the first byte past valid", [PARTLY])
    with pytest.raises(AssertionError, match="record 8"):
        ps.same_buffers(good, flip(good, start_of_partly + 800), "no partly: the whole record", [])
    with pytest.raises(AssertionError):
        ps.same_buffers(good, good + stream([b"\x08\x03"]), "a record more", [PARTLY])
    with pytest.raises(AssertionError):
        ps.same_buffers(good, stream([b"\x08\x01", b"\x08\x02"] + LONG[:5] + [b"\x09" * 199, good[-2003:]]),
                        "a buffer turned short", [PARTLY])


def test_child_main_prints_group_ok_only_after_a_group_that_returns(monkeypatch, capsys):
    built = []
    monkeypatch.setitem(sys.modules, "__graft_entry__", types.SimpleNamespace(build=lambda: built.append(1)))
    seen = []

    def boom(a):
        raise ValueError("the group failed")
    groups = {"fine": seen.append, "boom": boom}
    ps.child_main(groups, ["fine", "7", "x"])
    assert seen == [["7", "x"]] and built == [1] and capsys.readouterr().out.endswith("group ok\n")
    with pytest.raises(ValueError):
        ps.child_main(groups, ["boom"])
    assert "group ok" not in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        ps.child_main(groups, ["other"])
    assert e.value.code not in (0, None) and "unknown group 'other'" in str(e.value.code)
    assert "group ok" not in capsys.readouterr().out


@pytest.mark.parametrize("body,passes", [
    ("print('marker ok')\nprint('group ok')\n", True),
    ("print('marker ok')\n", False),                              # exit 0 without the dispatcher's last line
    ("print('another ok')\nprint('group ok')\n", False),          # exit 0 without the expected marker
    ("print('marker ok')\nprint('group ok')\nraise SystemExit(3)\n", False),
], ids=["all-well", "no-group-ok", "no-marker", "exit-3"])
def test_run_group_fails_on_a_child_that_went_wrong(monkeypatch, tmp_path, body, passes):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    child = tmp_path / "child.py"
    child.write_text(body)
    if passes:
        ps.run_group(str(child), [], "marker ok", 60)
    else:
        with pytest.raises((AssertionError, pytest.fail.Exception)):
            ps.run_group(str(child), [], "marker ok", 60)


def test_run_group_fails_without_a_device(monkeypatch, tmp_path):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    child = tmp_path / "child.py"
    child.write_text("print('marker ok')\nprint('group ok')\n")
    with pytest.raises(pytest.fail.Exception, match="HIP device"):
        ps.run_group(str(child), [], "marker ok", 60)


def test_big_fixture_windows_positions_aliases_and_keys():
    """the pure part of the big-pi fixture: where the windows lie, the compact numbering, the row a wrapped offset reads,
    and the edge list over them"""
    import numpy as np
    n, K = ps.BIG_ROWS, ps.BIG_K
    ids, wins = ps.big_ids(), ps.big_windows()
    assert n * K == 2 ** 32 + 2 ** 20 and ids.size == 640 == sum(hi - lo for lo, hi in wins) and (np.diff(ids) > 0).all()
    assert ids[0] == 0 and ids[-1] == n - 1 and all(lo % 64 == 0 and hi % 64 == 0 for lo, hi in wins)
    # what each window straddles: byte offset 2^32, element 2^31, element 2^32
    assert [(lo * K < at <= (hi - 1) * K) for (lo, hi), at in zip(wins[1:], (2 ** 30, 2 ** 31, 2 ** 32))] == [True] * 3
    assert (wins[1][0] + 64) * K * 4 == 2 ** 32 and (wins[2][0] + 64) * K == 2 ** 31 and (wins[3][0] + 128) * K == 2 ** 32
    # the alias of a row: itself below 2^19, a row of the first window from there on, all 128 of them
    assert np.array_equal(ps.big_alias(ids[ids < 2 ** 19]), ids[ids < 2 ** 19])
    assert np.array_equal(ps.big_alias(ids[ids >= 2 ** 19]), np.arange(128)) and (ids >= 2 ** 19).sum() == 128
    assert ps.big_alias(2 ** 19 + 5, K=4096) == 2 ** 19 + 5 and ps.big_alias(2 ** 20 + 5, K=4096) == 5
    # positions: the planted rows in order, the zero rows after them, rows past the end stay past the end
    assert np.array_equal(ps.big_positions(ids), np.arange(640))
    assert np.array_equal(ps.big_positions(ids[::-7]), np.arange(640)[::-7])
    zr = ps.BIG_ZERO_ROWS
    assert not set(zr) & set(ids.tolist()) and all(z < n for z in zr)
    assert ps.big_positions(list(zr)).tolist() == [640 + j for j in range(len(zr))]
    past = ps.big_positions([n, n + 5, 2 ** 32 - 1])
    assert (past >= 640 + len(zr)).all() and (past < 2 ** 32).all() and len(set(past.tolist())) == 3
    with pytest.raises(ValueError):
        ps.big_positions([129])
    # the wrapped view of the compact rows: only the rows >= 2^19 change, each to its alias's row
    compact = np.arange(640 * 3, dtype=np.float32).reshape(640, 3) + 1
    wrapped = ps.big_wrapped(compact)
    assert np.array_equal(wrapped[:512], compact[:512]) and np.array_equal(wrapped[512:], compact[:128])
    ext = ps.big_extended(compact)
    assert ext.shape == (640 + len(zr), 3) and not ext[640:].any() and np.array_equal(ext[:640], compact)
    assert ps.big_threshold(np.linspace(0.001, 1, 640 * 100, dtype=np.float32).reshape(640, 100)) > 0
    # the keys: every two windows and every window with itself, both orders, the irregular ones, the zero rows
    keys = ps.big_keys(3)
    assert np.array_equal(keys, ps.big_keys(3)) and 2000 < keys.size < 10000
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    win_of = lambda r: np.select([(r >= lo) & (r < hi) for lo, hi in wins], range(4), -1)   # noqa: E731
    valid = (a < n) & (b < n)
    seen = {(int(x), int(y)) for x, y in zip(win_of(a)[valid], win_of(b)[valid])}
    assert {(i, j) for i in range(4) for j in range(4)} <= seen
    assert ((a >= 2 ** 19) & (b >= 2 ** 19) & valid).sum() > 20 and ((a >= 2 ** 19) & (b < 128)).sum() > 20
    assert (a == b).sum() > 20 and (~valid).sum() > 20 and np.unique(keys).size < keys.size - 20
    assert (a == n).any() or (b == n).any()
    assert all(((a == z) | (b == z)).sum() >= 4 for z in zr) and (np.isin(a, zr) & np.isin(b, zr)).any()
    local = ps.big_remap(keys)
    la, lb = (local >> np.uint64(32)).astype(np.int64), (local & np.uint64(0xFFFFFFFF)).astype(np.int64)
    Nc = 640 + len(zr)
    assert np.array_equal((la < Nc) & (lb < Nc), valid) and np.array_equal(la < Nc, a < n) and np.array_equal(lb < Nc, b < n)
    assert np.array_equal(la[a < n], ps.big_positions(a[a < n])) and np.array_equal(la == lb, a == b)
    # the adjacency of the keys, globally and in compact numbering: the same rows
    off, tgt = ps.big_csr(keys, n)
    loff, ltgt = ps.big_csr(local, Nc)
    assert off.size == n + 1 and int(off[-1]) == tgt.size == int((a < n).sum() + (b < n).sum()) == int(loff[-1])
    rows = np.concatenate([ids, zr])
    assert np.array_equal(np.diff(off.astype(np.int64))[rows], np.diff(loff.astype(np.int64)))
    assert int(np.diff(off.astype(np.int64))[rows].sum()) == tgt.size        # no other row has a target
    for g, c in ((0, 0), (int(ids[-1]), 639), (zr[1], 641)):
        mine = tgt[int(off[g]):int(off[g + 1])].astype(np.int64)
        theirs = ltgt[int(loff[c]):int(loff[c + 1])].astype(np.int64)
        assert mine.size and np.array_equal(ps.big_positions(mine), theirs)
    assert (tgt.astype(np.int64) >= n).any()
