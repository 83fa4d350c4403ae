"""CPU: the host side of the served-record encoders: store.metadata_bytes against the metadata
packet_bytes embeds (itself pinned against google.protobuf by tests/test_packet_host.py), the argument refusals of
dh_rand_encode_device, which are decided before the device is touched, and the yardstick builders of
tests/serve_cases.py that tests/test_gpu_serve.py compares the device's bytes with."""
import ctypes
import hashlib

import pytest

import packet_cases as pc
import serve_cases as sc
from drand_amd import _lib, store

META_CASES = {
    "empty": {},
    "id_only": {"beacon_id": pc.BEACON_ID},
    "full": pc.FULL_META,
    "full_no_prerelease": dict(pc.FULL_META, node_version=dict(pc.NODE_VERSION, prerelease=None)),
}
SIGNATURE = _lib.SIGNATURES["dh_rand_encode_device"]  # without the entry point nothing below means anything


def test_metadata_bytes_absent():
    assert store.metadata_bytes(None) is None
    assert store.packet_bytes(pc.PR, {"round": 5}) == b"\x08\x05"  # and no field without it


@pytest.mark.parametrize("case", sorted(META_CASES))
def test_metadata_bytes_equals_the_embedded_metadata(case):
    md = META_CASES[case]
    body = store.metadata_bytes(md)
    lead = store.packet_bytes(pc.PR, {"round": 5})
    rec = store.packet_bytes(pc.PR, {"round": 5, "metadata": md})
    prefix = bytearray([0x2A])
    store._pb_put_varint(prefix, len(body))
    assert rec == lead + bytes(prefix) + body
    got = store.packet_from_bytes(pc.PR, rec)
    assert got["metadata"] is not None and got["beacon_id"] == md.get("beacon_id", "")
    if case == "empty":
        assert body == b""
    if case.startswith("full"):
        assert (b"rc1" in body) == (case == "full")


def call(form=1, rounds=0x1000, sigs=0x2000, sig_stride=48, sig_lens=0x3000, prevs=None, prev_stride=0, prev_lens=None, rands=None, keep=None,
         n=4, metadata=None, metadata_len=0, flags=0, out=None, cap=0, rec_lens=None, total=True):
    """dh_rand_encode_device with made-up device addresses: a call that is refused never reads them."""
    size = ctypes.c_size_t(77)
    rc = _lib.load().dh_rand_encode_device(form, rounds, sigs, sig_stride, sig_lens, prevs, prev_stride, prev_lens, rands, keep, n, metadata,
                                           metadata_len, flags, out, cap, rec_lens, ctypes.byref(size) if total else None, None)
    return rc, size.value, _lib.last_error()


REFUSALS = {
    "null_len_out": dict(total=False),
    "form_0": dict(form=0),
    "form_3": dict(form=3),
    "metadata_with_json": dict(form=1, metadata=b"\x12\x01x", metadata_len=3),
    "delimited_with_json": dict(form=1, flags=2),
    "newline_with_protobuf": dict(form=2, flags=1),
    "both_flags_json": dict(form=1, flags=3),
    "both_flags_protobuf": dict(form=2, flags=3),
    "unknown_flag": dict(form=2, flags=4),
    "prevs_without_lens": dict(prevs=0x4000, prev_stride=96),
    "lens_without_prevs": dict(prev_lens=0x5000),
    "stride_130": dict(sig_stride=130),
    "stride_0": dict(sig_stride=0),
    "prev_stride_130": dict(prevs=0x4000, prev_stride=130, prev_lens=0x5000),
    "stride_above_1_mib": dict(sig_stride=(1 << 20) + 4),
    "misaligned_sigs": dict(sigs=0x2002),
    "misaligned_prevs": dict(prevs=0x4001, prev_stride=96, prev_lens=0x5000),
    "misaligned_rands": dict(rands=0x6003),
    "n_16m": dict(n=1 << 24),
    "metadata_4097": dict(form=2, metadata=b"\x00" * 4097, metadata_len=4097),
    "null_column": dict(sigs=None),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_argument_refusals_without_a_device(case):
    rc, size, msg = call(**REFUSALS[case])
    assert rc == _lib.DH_EINVAL and msg, (case, rc, msg)
    if case != "null_len_out":
        assert size == 0  # *len_out is cleared before anything is decided
    if case == "n_16m":
        assert "split the call" in msg


def test_refusals_come_before_the_device():
    """The same calls with valid arguments get past the checks: on a machine without a device they end in the device
    error, never in DH_EINVAL (with one, n == 0 is DH_OK with length 0)."""
    for form, flags, md in ((1, 0, None), (1, 1, None), (2, 0, None), (2, 2, b""), (2, 2, b"\x00" * 4096)):
        rc, size, msg = call(form=form, flags=flags, metadata=md, metadata_len=len(md or b""), n=0)
        assert rc in (_lib.DH_OK, _lib.DH_EDEVICE), (form, flags, rc, msg)
        assert size == 0


def test_constants_and_binding():
    assert (_lib.DH_ENC_RANDOM_DATA_JSON, _lib.DH_ENC_PUBLIC_RAND_PB, _lib.DH_ENC_NEWLINE, _lib.DH_ENC_DELIMITED) == (1, 2, 1, 2)
    assert len(SIGNATURE[1]) == 19
    for f in ("encode_random_data", "encode_public_rand", "random_data_frames", "public_rand_frames", "export_random_data", "metadata_bytes"):
        assert callable(getattr(store, f))
    from drand_amd import client
    assert callable(client.relay_s3_sync_store)


def test_yardstick_builders():
    """serve_cases' expected bytes: random_data_line / packet_bytes of each kept row with the randomness named, framed."""
    rows = sc.shaped_rows(70, 0)
    assert {len(r["signature"]) for r in rows} >= {0, 1, 3, 47, 48, 96} and {len(r["previous_signature"]) for r in rows} >= {0, 32, 96}
    want, lens = sc.want_json(rows, newline=True)
    lines = want.split(b"\n")
    assert lines[-1] == b"" and len(lines) == len(rows) + 1 and lens == [len(l) for l in lines[:-1]]
    for r, l in zip(rows, lines):
        got = store.random_data_from_line(l)
        assert got["randomness"] == hashlib.sha256(r["signature"]).digest() and got["signature"] == r["signature"]
        assert got["round"] == r["round"] and got["previous_signature"] == r["previous_signature"]
    empty = store.random_data_from_line(sc.want_json([{"round": 0, "signature": b"", "previous_signature": b""}], newline=False)[0])
    assert empty["randomness"].hex().startswith("e3b0c442")
    keep = [i % 2 for i in range(len(rows))]
    want, lens = sc.want_pb(rows, keep=keep, delimited=True, metadata=pc.FULL_META)
    recs, rest = store.frame_delimited(want)
    assert rest == b""
    assert [len(r) for r in recs] == [l for l in lens if l] and [bool(l) for l in lens] == [bool(k) for k in keep]
    given = [bytes([i]) * 32 for i in range(len(rows))]
    want, _ = sc.want_pb(rows[:3], rands=given[:3])
    assert given[2] in want and hashlib.sha256(rows[2]["signature"]).digest() not in want
    assert sorted(set(len(str(r)) for r in sc.BOUNDARY_ROUNDS if r)) == list(range(1, 21))
    assert sorted(set((r.bit_length() + 6) // 7 for r in sc.BOUNDARY_ROUNDS if r)) == list(range(1, 11))
