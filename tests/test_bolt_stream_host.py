"""CPU: the layout code of the windowed trimmed-store writer (drand_amd/csrc/bolt_write.hpp) as a
stand-alone program under AddressSanitizer + UBSan (tests/bolt_stream_san): a record list and a window size in; head,
runs and tail out, built through the shared functions alone (plan_window, leaf_dword over the two row segments,
finish_tail) into exact-size heap buffers, the carried rows in two exact-size sets.

For every case of tests/bolt_write_cases.py and the windows 1, 2, 3, 7, 64 and all rows: no sanitizer report, bytes
equal to boltwrite2.write_bolt2's (the one-shot image), and check_image holds. Nobody has opened these images with Go
bbolt: that walk is the extent to which their acceptance by it is argued."""
import os
import shutil
import struct
import subprocess

import pytest

import bolt_cases as bc
import bolt_write_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "bolt_stream_san")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
WINDOWS = (1, 2, 3, 7, 64, None)  # None: all rows


@pytest.fixture(scope="module")
def stream_check():
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    r = subprocess.run(["make", "-s", "_build/bolt_stream_check"], cwd=SAN, env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(tmp, name, P, kv, window):
        src, dst = str(tmp / (name + ".rec")), str(tmp / ("%s_w%d.db" % (name, window)))
        if not os.path.exists(src):
            with open(src, "wb") as f:
                f.write(struct.pack("<II", P, len(kv)))
                for r in sorted(kv):
                    f.write(struct.pack("<QI", r, len(kv[r])) + kv[r])
        r = subprocess.run([os.path.join(SAN, "_build", "bolt_stream_check"), src, dst, str(window)], env=ENV, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, (name, window, r.stdout[-2000:], r.stderr[-4000:])  # a sanitizer report aborts
        line = r.stdout.split()
        assert line[0] == "OK", (name, window, r.stdout)
        return open(dst, "rb").read(), [int(x) for x in line[1:]]

    return run


@pytest.mark.parametrize("case", wc.cases(), ids=lambda c: c[0])
def test_every_window_gives_the_one_shot_image(stream_check, tmp_path, case):
    name, P, kv = case
    want, lay = wc.expected(tmp_path, name, P, kv)
    info = wc.check_image(want)
    for window in WINDOWS:
        w = window or len(kv)
        got, (rows, leaves, pages, _idle) = stream_check(tmp_path, name.replace("+", "p"), P, kv, w)
        assert len(got) == pages * P == len(want), (name, w)
        assert got == want, (name, w)
        assert (rows, leaves, pages) == (len(kv), len(lay["leaves"]), lay["pages"]), (name, w)
    assert info["records"] == [(bc.key(r), kv[r]) for r in sorted(kv)]
    assert wc.check_image(got) == info


def test_small_windows_close_no_leaf(stream_check, tmp_path):
    """The carry is exercised: with one row a window and 5 records a leaf, most appends emit nothing."""
    name, P, kv = next(c for c in wc.cases() if c[0] == "depth3_p512")
    got, (rows, leaves, _pages, idle) = stream_check(tmp_path, name, P, kv, 1)
    assert rows == len(kv) and idle >= rows - leaves - 1 > 0
    assert got == wc.expected(tmp_path, name, P, kv)[0]
