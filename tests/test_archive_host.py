"""CPU: RandomData JSON-lines archives on the host side.

* drand_amd/csrc/rdjson.hpp, the record parser the archive kernels share with the host, compiled into a stand-alone
  program under ASan + UBSan (tests/rdjson_san) and run over exact-size heap buffers: every canonical line decodes to
  exactly what store.random_data_from_line gives, every line that function rejects (or returns None for) is deferred,
  and every random_data_line output is canonical.
* the framing rule against store.archive_lines, the JSON-array form refused.
* store.check_random_data_host, with the oracle verifying, on the faulty 300-record archives of tests/archive_cases.py
  equals the record in tests/golden/archive_cases.json."""
import os
import struct
import subprocess

import pytest

import archive_cases as ac
from drand_amd import scheme_from_name
from drand_amd import store

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = os.path.join(HERE, "rdjson_san")
R32, R48, R96 = ac.rand_bytes("r32", 32), ac.rand_bytes("r48", 48), ac.rand_bytes("r96", 96)
G1 = store.random_data_line({"round": 367, "randomness": R32, "signature": R48})
G2C = store.random_data_line({"round": 2634945, "randomness": R32, "signature": R96, "previous_signature": ac.rand_bytes("p96", 96)})
MUTANTS = b'",:{}0aAg \\\x00'  # the 12 bytes of the mutation sweep


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "_build/rdjson_check"], cwd=SAN)
    return os.path.join(SAN, "_build", "rdjson_check")


def canonical_lines():
    """Lines random_data_line writes: the parser must call every one of them canonical."""
    full = {"round": 5, "randomness": R32, "signature": R96, "previous_signature": R48}
    out = [store.random_data_line({}), G1, G2C]
    out += [store.random_data_line({k: full[k]}) for k in full]                          # each single field
    out += [store.random_data_line({k: v for k, v in full.items() if k != d}) for d in full]  # each field absent in turn
    out += [store.random_data_line({"round": r, "signature": v}) for r in (1, 9, 10, (1 << 64) - 1) for v in (R32, R48, R96, b"\x00")]
    return out


def deferred_lines():
    """One line per deferred class of the issue; the host decoder accepts some of them, the device none."""
    sig = R48.hex().encode()
    return [
        G1.replace(sig, sig.upper()),                                   # uppercase hex
        G1.replace(sig, sig[:-1]),                                      # an odd digit count
        b'{"round":5,"signature":""}', b'{"round":0,"signature":"00"}', b'{"round":0}',  # "" and "round":0
        G1 + b"\r", b" " + G1, G1.replace(b":", b": ", 1), G1.replace(b",", b", ", 1), G1[:-1] + b" }", b"   ", b"\t",
        b'{"signature":"00","round":5}', b'{"round":5,"round":6}', b'{"randomness":"00","randomness":"01"}',
        G1[:-1] + b',"metadata":{"beaconID":"default"}}', b'{"previous_signature":"00","signature":"00"}',
        b'{"round":123456789012345678901}', b'{"round":18446744073709551616}', b'{"round":99999999999999999999}',
        b'{"round":05}', b'{"round":-5}', b'{"round":5.0}', b'{"round":"5"}', b'{"round":}',
        G1[:-1], G1 + b"}", G1 + b"x", b"{", b"}", b"{}{}", b'{,}', b'{"round":5,}', b'{"round":5,,"signature":"00"}',
        G1.replace(sig, b"zz" + sig[2:]), b'{"signature":"0g"}', b'{"signature":"00', b'{"signature":00}',
        b'{"signature":null}', b"[]", b"null", b"5", b'[{"round":5}]', b"\xff\xfe", b'{"round":5,"signature":"\xc3\xa9"}',
        ac.line_of_length(4097),                                        # above RDJSON_MAX_LINE
    ]


def sweep_lines():
    out = []
    for rec in (G1, G2C):
        out += [rec[:k] for k in range(len(rec))]                       # cut at each length
        out += [rec[:k] + bytes([m]) + rec[k + 1:] for k in range(len(rec)) for m in MUTANTS]
    return out


def run_parser(prog, tmp_path, lines):
    corpus = os.path.join(str(tmp_path), "corpus.bin")
    with open(corpus, "wb") as f:
        for l in lines:
            f.write(struct.pack("<I", len(l)) + l)
    res = subprocess.run([prog, corpus], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]  # no sanitizer report
    got = res.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def host(line):
    """random_data_from_line as the parser's output line, or None when it rejects the line / returns None."""
    try:
        r = store.random_data_from_line(line)
    except store.DECODE_ERRORS:
        return None
    if r is None:
        return None
    return "C %d %s %s %s" % (r["round"], r["randomness"].hex() or "-", r["signature"].hex() or "-", r["previous_signature"].hex() or "-")


def test_parser_agrees_with_the_host_decoder(prog, tmp_path):
    canon, deferred, sweep = canonical_lines(), deferred_lines(), sweep_lines()
    edge = [ac.line_of_length(4096)]  # a line of exactly RDJSON_MAX_LINE bytes is still parsed
    assert len(edge[0]) == 4096 and len(ac.line_of_length(4097)) == 4097 == len(deferred[-1])
    lines = canon + edge + deferred + sweep
    got = run_parser(prog, tmp_path, lines)
    n_canon = 0
    for l, g in zip(lines, got):
        want = host(l)
        if g != "D":
            n_canon += 1
            assert g == want, (l, g, want)  # canonical: exactly what the host decoder gives
        assert want is not None or g == "D", (l, g)  # rejected or None on the host: deferred
    for l, g in zip(canon + edge, got):
        assert g != "D" and g == host(l), l  # so the parser cannot pass by deferring everything
    for l, g in zip(deferred, got[len(canon) + 1:]):
        assert g == "D", l
    assert n_canon > len(canon) + 1000  # hex-for-hex and digit-for-digit mutants stay canonical


def test_line_writer_round_trips():
    for l in canonical_lines():
        assert store.random_data_line(store.random_data_from_line(l)) == l
    assert store.random_data_line({"round": 0, "signature": b""}) == b"{}"
    assert store.random_data_from_line("  \r") is None and store.random_data_from_line(b"") is None
    for bad in (b"{", b'{"round":-1}', b'{"round":18446744073709551616}', b'{"signature":"0"}', b"[]", b"\xff"):
        with pytest.raises(store.DECODE_ERRORS):
            store.random_data_from_line(bad)
    # the array / line reader of the parent commit reads the same records from the same lines
    text = b"\n".join(canonical_lines()).decode()
    assert store.read_random_data(text) == [store.random_data_from_line(l) for l in canonical_lines()]


@pytest.mark.parametrize("data", [b"", b"\n", b"\n\n\n", b"a", b"a\n", b"\na", b"a\n\nb", b"\n\na\n\n\nbc\n\n", b"ab\ncd",
                                  b"x" * 4096 + b"\n" + b"y" * 4097 + b"\nz", b" [\n", b"{}\n[\n"])
def test_host_framing(prog, tmp_path, data):
    path = os.path.join(str(tmp_path), "buf")
    open(path, "wb").write(data)
    got = subprocess.run([prog, "-f", path], capture_output=True, text=True, check=True).stdout.split()
    want, at = [], 0
    for run in data.split(b"\n"):
        if run:
            want += [str(at), str(min(len(run), 4097))]
        at += len(run) + 1
    assert got == want
    assert [data[int(o):int(o) + int(n)] for o, n in zip(got[::2], got[1::2])] == [l[:4097] for l in store.archive_lines(data)]


@pytest.mark.parametrize("data", [b"[", b"\n\n[{}]\n", b'[{"round":1}]'])
def test_array_form_is_not_framed(prog, tmp_path, data):
    path = os.path.join(str(tmp_path), "buf")
    open(path, "wb").write(data)
    assert subprocess.run([prog, "-f", path], capture_output=True, text=True, check=True).stdout == "A\n"


def test_argument_refusals():
    s = scheme_from_name("bls-unchained-g1-rfc9380")
    with pytest.raises(store.DECODE_ERRORS):
        store.random_data_from_line(b'{"round":"x"}')
    with pytest.raises(store.DECODE_ERRORS):
        store.random_data_line(None)
    # no record, no status; an anchor alone decides nothing
    assert len(store.check_random_data_host(b"", s, b"", verify=lambda *a: [])) == 0
    assert len(store.check_random_data_host(b"\n \n", s, b"", anchor=(1, b"x"), verify=lambda *a: [])) == 0
    # a signature of another length never reaches the verifier
    seen = []
    st = store.check_random_data_host(b'{"round":1,"signature":"00"}\n{"round":2}\nnope\n', s, b"", verify=lambda sc, pk, r: seen.extend(r) or [])
    assert list(st) == [store.AR_INVALID, store.AR_NO_SIGNATURE | store.AR_INVALID, store.AR_INVALID] and not seen


@pytest.fixture(scope="module")
def gold():
    return ac.load_golden()


@pytest.mark.parametrize("name", ac.SCHEMES)
def test_recorded_statuses(oracle, gold, name):
    """check_random_data_host with the oracle verifying, on the clean and the faulty archive, with the anchor, without
    one and with one the chain does not follow."""
    assert [s.hex() for s in ac.sign_chain(name, oracle)[:3]] == gold["chains"][name]["sigs"][:3]
    got = ac.host_status(name, gold, oracle)
    assert got == gold["status"][name]
    assert not any(got["clean"]) and len(got["clean"]) == ac.N
    faulty = {i: x for i, x in enumerate(got["anchor"]) if x}
    chained = name == "pedersen-bls-chained"
    inv, rnd, seq, link = store.AR_INVALID, store.AR_RANDOMNESS, store.AR_SEQUENCE, store.AR_LINK if chained else 0
    want = {10: inv | rnd, 20: inv | rnd, 30: inv | rnd | store.AR_NO_SIGNATURE, 40: rnd, 50: seq | link, 60: seq | link, 90: inv,
            91: seq | link}
    if chained:  # the records after a damaged signature carry the true one; a wrong previous_signature does not verify
        want.update({11: link, 21: link, 31: link, 70: inv | link})
    assert faulty == want
    assert got["no_anchor"] == got["anchor"] and got["bad_anchor"][0] == seq | link and got["bad_anchor"][1:] == got["anchor"][1:]
