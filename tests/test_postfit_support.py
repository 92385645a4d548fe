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
