"""CPU: the bbolt page parser shared by the host and the store kernels (drand_amd/csrc/bolt.hpp).

* dh_bolt_index (host only) against BoltFile's walk: leaf order and count, and the records of its leaves against
  BoltFile.bucket, on the reference's own trimmed store and on files of every page size, depth and bucket form;
* bolt.hpp as a stand-alone program under AddressSanitizer + UBSan (tests/bolt_san): the index walk and
  bolt_leaf_check / bolt_leaf_elem (the calls the kernels make) over files in exact-size heap buffers — digests equal
  Python's, corrupt files yield an error code with no sanitizer report and never disagree with a BoltFile rejection,
  plus a byte-mutation sweep over one leaf and one branch header;
* the expected faulty sets of the GPU replay cases (tests/test_gpu_bolt.py), computed here with check_past_beacons
  over BoltTrimmedStore and the oracle, equal the record in tests/golden/bolt_cases.json."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bolt_cases as bc
from drand_amd.store import BoltError, BoltFile, BoltTrimmedStore
from drand_amd.sync import check_past_beacons
from test_readers import OracleScheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "drand_amd", "libdrandhip.so")
SAN = os.path.join(ROOT, "tests", "bolt_san")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libdrandhip.so not built")


# ---------------------------------------------------------------- Python's view of a file

def py_walk(data):
    """(leaf byte offsets in key order, [(key, value)] of the beacons bucket without nested buckets) by BoltFile."""
    bf = BoltFile(data)
    leaves = []

    def leaves_under(buf_off):
        _, flags, count, _ = struct.unpack_from("<QHHI", data, buf_off)
        if flags & 0x02:
            leaves.append(buf_off)
        elif flags & 0x01:
            for i in range(count):
                _p, _k, child = struct.unpack_from("<IIQ", data, buf_off + 16 + 16 * i)
                leaves_under(bf._page(child)[1])
        else:
            raise BoltError("flags")

    def elements(off):  # (key offset, key, value, flags) of one leaf
        _, _f, count, _ = struct.unpack_from("<QHHI", data, off)
        for i in range(count):
            e = off + 16 + 16 * i
            fl, pos, ks, vs = struct.unpack_from("<IIII", data, e)
            yield e + pos, bytes(data[e + pos:e + pos + ks]), bytes(data[e + pos + ks:e + pos + ks + vs]), fl

    top = []
    leaves_under(bf._page(bf.meta["root"])[1])
    top, leaves = leaves, []
    for off in top:
        for koff, k, v, fl in elements(off):
            if k == b"beacons" and fl & 1 and not leaves:
                root = struct.unpack_from("<Q", v)[0]
                if root:
                    leaves_under(bf._page(root)[1])
                else:
                    leaves.append(koff + len(k) + 16)
    recs = [(k, v) for off in leaves for _o, k, v, fl in elements(off) if not fl & 1]
    return leaves, recs


def py_digest(recs):
    h = 0xcbf29ce484222325
    for k, v in recs:
        for x in struct.pack("<II", len(k), len(v)) + k + v:
            h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return "%016x" % h


def py_accepts(data):
    """BoltFile's decision on a file (any exception is a rejection), and the digest when it accepts."""
    try:
        kv = BoltFile(data).bucket(b"beacons")
        return True, kv
    except Exception:  # noqa: BLE001 - BoltError, struct.error, RecursionError: all "the reader refuses the file"
        return False, None


# ---------------------------------------------------------------- dh_bolt_index

@needs_lib
def test_bolt_index_matches_boltfile(tmp_path):
    from drand_amd import _lib
    lib = _lib.load()
    for name, path, _lay in bc.parity_files(tmp_path):
        data = open(path, "rb").read()
        want_leaves, want_recs = py_walk(data)
        buf = np.frombuffer(data, np.uint8)
        offs = np.zeros(max(1, len(want_leaves)) + 4, np.uint64)
        psz, n = ctypes.c_uint32(0), ctypes.c_size_t(0)
        rc = lib.dh_bolt_index(buf.ctypes.data, len(data), ctypes.byref(psz), offs.ctypes.data, len(offs), ctypes.byref(n))
        assert rc == 0, (name, _lib.last_error())
        assert psz.value == BoltFile(data).page_size, name
        assert offs[:n.value].tolist() == want_leaves, name
        kv = BoltFile(data).bucket(b"beacons")
        assert dict(want_recs) == kv and len(want_recs) == len(kv), name
        # too little room: DH_EINVAL with the count needed
        if n.value > 1:
            n2 = ctypes.c_size_t(0)
            assert lib.dh_bolt_index(buf.ctypes.data, len(data), None, offs.ctypes.data, 1, ctypes.byref(n2)) == _lib.DH_EINVAL
            assert n2.value == n.value
    # no bucket of that name, and a file that is no bbolt file
    other = str(tmp_path / "other.db")
    bc.write_bolt2(other, [], bucket=b"other")
    for data in (open(other, "rb").read(), b"\0" * 100, b""):
        n = ctypes.c_size_t(0)
        buf = np.frombuffer(data + b"\0", np.uint8)
        assert lib.dh_bolt_index(buf.ctypes.data, len(data), None, None, 0, ctypes.byref(n)) == _lib.DH_ECORRUPT
        assert "bbolt store" in _lib.last_error()


# ---------------------------------------------------------------- the sanitizer program

@pytest.fixture(scope="module")
def bolt_check():
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    r = subprocess.run(["make", "-s", "_build/bolt_check"], cwd=SAN, env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([os.path.join(SAN, "_build", "bolt_check")] + [str(a) for a in args], env=ENV,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])  # a sanitizer report aborts
        return r.stdout.splitlines()

    return run


def test_parser_under_sanitizers_matches_python(bolt_check, tmp_path):
    files = bc.parity_files(tmp_path)
    lines = bolt_check(*[p for _n, p, _l in files])
    assert len(lines) == len(files)
    for (name, path, _lay), line in zip(files, lines):
        data = open(path, "rb").read()
        leaves, recs = py_walk(data)
        rounds = [k for k, _v in recs if len(k) == 8]
        assert line.split() == ["OK", str(BoltFile(data).page_size), str(len(leaves)), str(len(recs)), str(len(rounds)),
                                py_digest(recs)], (name, line)


def _classify(line, data, what):
    """The program's line against BoltFile on the same bytes: a BoltFile rejection is a rejection here, and a file both
    accept has the same records. Returns "OK" / "ERR"."""
    ok, kv = py_accepts(data)
    verdict = line.split()[0]
    assert verdict in ("OK", "ERR"), (what, line)
    if not ok:
        assert verdict == "ERR", (what, line)
    elif verdict == "OK":
        _leaves, recs = py_walk(data)
        assert line.split()[5] == py_digest(recs) and int(line.split()[3]) == len(kv), (what, line)
    return verdict


def test_corrupt_files_under_sanitizers(bolt_check, tmp_path):
    files, base, at = bc.corrupt_files(tmp_path)
    lines = bolt_check(*[p for _n, p in files])
    got = {}
    for (name, path), line in zip(files, lines):
        got[name] = _classify(line, open(path, "rb").read(), name)
    assert got == bc.load_golden()["corrupt"]
    assert got["meta0_bad"] == "OK" and got["descending"] == "ERR" and got["metas_bad"] == "ERR"
    # mutation sweep: every byte of the first 64 of one leaf and one branch set to 0x00 / 0xFF / +1
    data = open(base, "rb").read()
    for what in ("leaf", "branch"):
        lines = bolt_check("--sweep", base, at[what], 64)
        assert len(lines) == 64 * 3
        k = 0
        rejected = 0
        for i in range(at[what], at[what] + 64):
            for mu in (0x00, 0xFF, (data[i] + 1) & 0xFF):
                b = bytearray(data)
                b[i] = mu
                rejected += _classify(lines[k], bytes(b), (what, i, mu)) == "ERR"
                k += 1
        assert 0 < rejected < 64 * 3  # some mutations break the structure, some only change a record


# ---------------------------------------------------------------- expected faulty sets of the GPU cases

def compute_golden(oracle, tmp):
    replay = {}
    for name in bc.SCHEMES:
        pk, _sk, _kv = bc.chain(name)
        files = bc.replay_files(tmp, name, oracle)
        s = OracleScheme(oracle, name)
        for kind, up_to, window in bc.REPLAY_CALLS:
            st = BoltTrimmedStore(files[kind], s.chained)
            replay[bc.call_id(name, kind, up_to, window)] = check_past_beacons(st, s, pk, up_to, window=window)
    return replay


def test_recorded_faulty_sets(oracle, tmp_path):
    gold = bc.load_golden()["replay"]
    got = compute_golden(oracle, tmp_path)
    assert got == gold
    # the shapes the cases exist for
    c, u = "pedersen-bls-chained", "bls-unchained-g1-rfc9380"
    assert gold[bc.call_id(c, "clean", 1000, 8)] == [] and gold[bc.call_id(u, "clean", 1000, 8)] == []
    assert gold[bc.call_id(c, "rm7", 1000, 8)] == [7, 8] and gold[bc.call_id(u, "rm7", 1000, 8)] == [7]
    assert gold[bc.call_id(c, "odd", 1000, 8)] == [10] and gold[bc.call_id(u, "odd", 1000, 8)] == [10]
    assert gold[bc.call_id(c, "swap", 1000, 8)] == [12, 13, 14] and gold[bc.call_id(u, "swap", 1000, 8)] == [12, 13]
