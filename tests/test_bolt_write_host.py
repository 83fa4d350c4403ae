"""CPU: the layout code of the trimmed-store writer (drand_amd/csrc/bolt_write.hpp), which the pack
kernel shares with the host, as a stand-alone program under AddressSanitizer + UBSan (tests/bolt_write_san): a record
list in, the whole image out, built through the shared functions alone into exact-size heap buffers.

* no sanitizer report, and bytes equal to boltwrite2.write_bolt2(path, items, page_size=P) over the case list of
  tests/bolt_write_cases.py (page sizes 256 / 512 / 4096 / 16384; one record; a full leaf and one more; 48- and 96-byte
  values; depths 3 and 4; a 32-byte genesis value, a 95-byte and a zero-length value, an overflow leaf between fitting
  records, gaps, round 2^64 - 1);
* check_image, a structural restatement of bbolt's consistency walk, holds for the two Go-written fixtures under
  tests/golden/boltdb and for every image produced. Nobody has opened these images with Go bbolt: this walk is the
  extent to which their acceptance by it is argued."""
import os
import shutil
import struct
import subprocess

import pytest

import bolt_cases as bc
import bolt_json_cases as jc
import bolt_write_cases as wc
from drand_amd.store import BoltTrimmedStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "bolt_write_san")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def write_check():
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    r = subprocess.run(["make", "-s", "_build/bolt_write_check"], cwd=SAN, env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(tmp, name, P, kv):
        src, dst = str(tmp / (name + ".rec")), str(tmp / (name + ".db"))
        with open(src, "wb") as f:
            f.write(struct.pack("<II", P, len(kv)))
            for r in sorted(kv):
                f.write(struct.pack("<QI", r, len(kv[r])) + kv[r])
        r = subprocess.run([os.path.join(SAN, "_build", "bolt_write_check"), src, dst], env=ENV, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])  # a sanitizer report aborts
        line = r.stdout.split()
        assert line[0] == "OK", (name, r.stdout)
        return open(dst, "rb").read(), [int(x) for x in line[1:]]

    return run


@pytest.mark.parametrize("case", wc.cases(), ids=lambda c: c[0])
def test_image_equals_write_bolt2(write_check, tmp_path, case):
    name, P, kv = case
    got, (rows, leaves, pages) = write_check(tmp_path, name.replace("+", "p"), P, kv)
    want, lay = wc.expected(tmp_path, name, P, kv)
    assert len(got) == pages * P == len(want)
    assert got == want
    assert (rows, leaves, pages) == (len(kv), len(lay["leaves"]), lay["pages"])
    info = wc.check_image(got)
    assert info["records"] == [(bc.key(r), kv[r]) for r in sorted(kv)]
    assert info["depth"] == lay["depth"] == wc.DEPTHS.get(name, lay["depth"])
    # and the project's own reader agrees
    path = tmp_path / "img.db"
    path.write_bytes(got)
    st = BoltTrimmedStore(str(path), False)
    assert st.rounds() == sorted(kv) and all(st.get(r).signature == kv[r] for r in list(kv)[:50])


def test_consistency_walk_accepts_the_go_written_fixtures():
    for path in (bc.REF_TRIMMED, jc.REF_UNTRIMMED):
        info = wc.check_image(open(path, "rb").read())
        assert info["records"], path


def test_consistency_walk_rejects_broken_images(tmp_path):
    """The walk is not vacuous: each defect it names is found."""
    P = 512
    want, lay = wc.expected(tmp_path, "base", P, wc.recs(range(0, 130), 96, "w"))
    leaf, branch = lay["leaves"][3] * P, lay["branches"][0] * P

    def broken(patches, cut=None):
        b = bytearray(want)
        for off, val in patches:
            b[off:off + len(val)] = val
        with pytest.raises(AssertionError):
            wc.check_image(bytes(b if cut is None else b[:cut]))

    wc.check_image(want)
    broken([(72, b"\x01\x02\x03\x04")])  # a meta checksum
    broken([(branch + 16 + 16 + 8, struct.pack("<Q", lay["leaves"][0]))])  # a leaf reached twice, another never
    e1 = leaf + 16 + 16
    kpos = e1 + struct.unpack_from("<I", want, e1 + 4)[0]
    broken([(kpos, bc.key(0))])  # keys descend inside a leaf
    e0 = leaf + 16
    broken([(e0 + struct.unpack_from("<I", want, e0 + 4)[0] + 7, b"\xff")])  # a leaf's first key is not its branch key
    broken([(leaf + 12, struct.pack("<I", 1 << 20))])  # an extent beyond the file
    broken([], cut=len(want) - P)  # the file ends below the high-water mark
