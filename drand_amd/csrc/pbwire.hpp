// The protobuf wire form of drand's beacon records (protobuf/drand/protocol.proto:113-118 BeaconPacket and
// protobuf/drand/api.proto:44-52 PublicRandResponse of the reference): the parser of ONE record, shared by the host
// (plain g++, no HIP) and the device (k_packet.hip). No heap, no state; every byte is read through
// bolt.hpp's bounds-checked view. Framing is the caller's: it hands in each record's extent.
//
// Only the canonical form is decoded, what proto.Marshal writes: the fields in field-number order, each at most once,
// the record ending exactly at its end.
//   BeaconPacket       := [0A L bytes] [10 V] [1A L bytes] [22 M Metadata]               prev, round, sig, metadata
//   PublicRandResponse := [08 V] [12 L bytes] [1A L bytes] [22 L bytes] [2A M Metadata]  round, sig, prev, randomness, metadata
//   Metadata           := [0A M NodeVersion] [12 L ascii] [1A L bytes]                   node_version, beaconID, chain_hash
//   NodeVersion        := [08 V32] [10 V32] [18 V32] [22 M ascii]                        major, minor, patch, prerelease
// Every varint is minimal (at most 10 bytes, a last byte of zero only in the one-byte zero, the tenth byte at most 1);
// 1 <= V < 2^64, 1 <= V32 < 2^32, L >= 1 (proto3 never writes a zero or an empty bytes field), M >= 0 (a present, empty
// sub-message is written; prerelease has explicit presence); ascii = bytes below 0x80 only (the host decoder validates
// UTF-8, this parser does not, so it is never the more lenient side). A record of 0 bytes is canonical: every field
// absent, round 0. Every other record, and every record above PBWIRE_MAX_RECORD bytes, is DEFERRED: nothing is decided
// about it here, the caller's host decoder (store.packet_from_bytes) does.
#pragma once
#include "bolt.hpp"

namespace dh {
namespace bolt {

constexpr uint32_t PBWIRE_MAX_RECORD = 4096;  // a longer record is deferred unread (a chained G2 packet is about 220 bytes)
constexpr int PB_BEACON_PACKET = 1, PB_PUBLIC_RAND = 2;

// offsets are inside the record; a length of 0 = the field is absent
struct pbrec {
  uint64_t round;
  uint32_t sig_off, sig_len, prev_off, prev_len, rand_off, rand_len, id_off, id_len, has_meta;
};

// a minimal varint at [*i, end): *i moves past it
BOLT_HD bool pb_varint(const view& r, uint64_t* i, uint64_t end, uint64_t* out) {
  uint64_t v = 0;
  for (uint32_t k = 0; k < 10; k++) {
    if (*i + k >= end) return false;
    const uint32_t b = r.p[*i + k];
    if (k == 9 && b > 1) return false;
    v |= (uint64_t)(b & 0x7f) << (7 * k);
    if (!(b & 0x80)) {
      if (k > 0 && b == 0) return false;  // not minimal
      *i += k + 1;
      *out = v;
      return true;
    }
  }
  return false;
}

// is the byte at *i (inside end) the tag `t`; then *i moves past it
BOLT_HD bool pb_tag(const view& r, uint64_t* i, uint64_t end, uint32_t t) {
  if (*i >= end || r.p[*i] != t) return false;
  ++*i;
  return true;
}

// a length-delimited extent of at least `least` bytes inside end; *i moves past it
BOLT_HD bool pb_extent(const view& r, uint64_t* i, uint64_t end, uint64_t least, uint32_t* off, uint32_t* len) {
  uint64_t n;
  if (!pb_varint(r, i, end, &n) || n < least || n > end - *i) return false;
  *off = (uint32_t)*i;
  *len = (uint32_t)n;
  *i += n;
  return true;
}

BOLT_HD bool pb_ascii(const view& r, uint32_t off, uint32_t len) {
  for (uint32_t k = 0; k < len; k++)
    if (r.p[off + k] & 0x80) return false;
  return true;
}

// [tag V]: 1 <= V <= most, when the tag is there
BOLT_HD bool pb_opt_uint(const view& r, uint64_t* i, uint64_t end, uint32_t t, uint64_t most, uint64_t* out) {
  if (!pb_tag(r, i, end, t)) return true;
  return pb_varint(r, i, end, out) && *out >= 1 && *out <= most;
}

// [tag L bytes], L >= 1, when the tag is there
BOLT_HD bool pb_opt_bytes(const view& r, uint64_t* i, uint64_t end, uint32_t t, uint32_t* off, uint32_t* len) {
  if (!pb_tag(r, i, end, t)) return true;
  return pb_extent(r, i, end, 1, off, len);
}

BOLT_HD bool pb_node_version(const view& r, uint64_t i, uint64_t end) {
  uint64_t v;
  uint32_t off, len;
  for (uint32_t t = 0x08; t <= 0x18; t += 8)
    if (!pb_opt_uint(r, &i, end, t, 0xffffffffull, &v)) return false;
  if (pb_tag(r, &i, end, 0x22) && !(pb_extent(r, &i, end, 0, &off, &len) && pb_ascii(r, off, len))) return false;
  return i == end;
}

BOLT_HD bool pb_metadata(const view& r, uint64_t i, uint64_t end, pbrec* out) {
  uint32_t off, len;
  if (pb_tag(r, &i, end, 0x0A) && !(pb_extent(r, &i, end, 0, &off, &len) && pb_node_version(r, off, (uint64_t)off + len))) return false;
  if (!pb_opt_bytes(r, &i, end, 0x12, &out->id_off, &out->id_len) || !pb_ascii(r, out->id_off, out->id_len)) return false;
  if (!pb_opt_bytes(r, &i, end, 0x1A, &off, &len)) return false;
  return i == end;
}

BOLT_HD bool pbwire_match(int kind, const view& r, pbrec* out) {
  if (r.len > PBWIRE_MAX_RECORD) return false;
  const uint64_t end = r.len;
  uint64_t i = 0;
  uint32_t meta_tag;
  if (kind == PB_BEACON_PACKET) {
    if (!pb_opt_bytes(r, &i, end, 0x0A, &out->prev_off, &out->prev_len)) return false;
    if (!pb_opt_uint(r, &i, end, 0x10, ~0ull, &out->round)) return false;
    if (!pb_opt_bytes(r, &i, end, 0x1A, &out->sig_off, &out->sig_len)) return false;
    meta_tag = 0x22;
  } else if (kind == PB_PUBLIC_RAND) {
    if (!pb_opt_uint(r, &i, end, 0x08, ~0ull, &out->round)) return false;
    if (!pb_opt_bytes(r, &i, end, 0x12, &out->sig_off, &out->sig_len)) return false;
    if (!pb_opt_bytes(r, &i, end, 0x1A, &out->prev_off, &out->prev_len)) return false;
    if (!pb_opt_bytes(r, &i, end, 0x22, &out->rand_off, &out->rand_len)) return false;
    meta_tag = 0x2A;
  } else {
    return false;
  }
  if (pb_tag(r, &i, end, meta_tag)) {
    uint32_t off, len;
    if (!pb_extent(r, &i, end, 0, &off, &len) || !pb_metadata(r, off, (uint64_t)off + len, out)) return false;
    out->has_meta = 1;
  }
  return i == end;
}

// true = canonical (and *out is set), false = deferred (*out all zero); reads only inside `rec`
BOLT_HD bool pbwire_parse(int kind, const view& rec, pbrec* out) {
  *out = pbrec{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (pbwire_match(kind, rec, out)) return true;
  *out = pbrec{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return false;
}

// The walk over varint-delimited records (the host convenience of dh_pb_frame_delimited; never on the hot path, where
// the caller holds the lengths): minimal prefixes below 2^32. Stops at the first prefix that is malformed or whose
// payload runs past the buffer; *consumed = where it stopped. Fills at most `cap` entries and returns the count.
BOLT_HD uint64_t pb_frame_delimited(const view& f, uint64_t* off_out, uint32_t* len_out, uint64_t cap, uint64_t* consumed) {
  uint64_t i = 0, n = 0;
  for (;;) {
    uint64_t j = i, l;
    if (!pb_varint(f, &j, f.len, &l) || l >> 32 || l > f.len - j) break;
    if (n < cap) {
      off_out[n] = j;
      len_out[n] = (uint32_t)l;
    }
    n++;
    i = j + l;
  }
  *consumed = i;
  return n;
}

}  // namespace bolt
}  // namespace dh
