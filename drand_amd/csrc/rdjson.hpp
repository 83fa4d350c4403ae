// client.RandomData JSON-lines archives (client/random.go:5-10 of the reference, marshalled through nikkolasg/hexjson
// by the HTTP relays): the framing rule and the parser of ONE record, shared by the host (plain g++, no HIP) and the
// device (k_archive.hip). No heap, no state; every byte is read through bolt.hpp's bounds-checked view.
//
// Framing: records are the maximal runs of bytes between '\n' (0x0A) bytes; a last run without a closing '\n' is a
// record when it is not empty; zero-length runs are skipped. A JSON string cannot hold a raw 0x0A, so this framing is
// exact for any valid JSON. The JSON-array form is not framed here (rdjson_is_array: the caller keeps the host reader).
//
// Only the canonical form is decoded: exactly '{' fields '}' with nothing before, between or after, the fields a
// subsequence of "round":D "randomness":"H" "signature":"H" "previous_signature":"H" in that order, joined by single
// commas ({} is canonical: round 0, every length 0). D is a decimal of 1-20 digits without a leading zero, not 0,
// that fits 64 bits; H is a non-zero even number of characters 0-9a-f (omitempty never writes 0 or ""). Every other
// record is DEFERRED: nothing is decided about it here, the caller's host decoder does. That decoder
// (store.random_data_from_line) is this project's restatement of the record's JSON rules, not a decoder pinned to
// nikkolasg/hexjson: a verdict on a deferred record is the restatement's. Relays write canonical records only.
#pragma once
#include "bolt.hpp"

namespace dh {
namespace bolt {

constexpr uint32_t RDJSON_MAX_LINE = 4096;  // a longer line is deferred unread (a chained G2 record is about 560 bytes)

// offsets are inside the line; the hex lengths count characters, 0 = the field is absent
struct rdjson {
  uint64_t round;
  uint32_t rand_off, rand_hex, sig_off, sig_hex, prev_off, prev_hex;
};

// is `i` the start of a record: a non-'\n' byte at offset 0 or after a '\n'
BOLT_HD bool rdjson_starts(const view& f, uint64_t i) { return f.p[i] != '\n' && (i == 0 || f.p[i - 1] == '\n'); }

// the first byte of the first record is '[': the JSON-array form
BOLT_HD bool rdjson_is_array(const view& f) {
  for (uint64_t i = 0; i < f.len; i++)
    if (f.p[i] != '\n') return f.p[i] == '[';
  return false;
}

// H" with its first character at *i (the opening quote belongs to the key's literal)
BOLT_HD bool rdjson_hex(const view& l, uint64_t* i, uint32_t* off, uint32_t* hex) {
  uint64_t j = *i;
  while (j < l.len && hj_hex(l.p[j])) j++;
  const uint64_t n = j - *i;
  if (j >= l.len || l.p[j] != '"' || n == 0 || (n & 1)) return false;
  *off = (uint32_t)*i;
  *hex = (uint32_t)n;
  *i = j + 1;
  return true;
}

BOLT_HD bool rdjson_match(const view& l, rdjson* out) {
  if (l.len < 2 || l.len > RDJSON_MAX_LINE || l.p[0] != '{') return false;
  uint64_t i = 1;
  if (l.p[1] == '}') return l.len == 2;
  for (int next = 0;; next++) {  // `next`: the first field that may still come
    int k = next;
    if (k <= 0 && hj_lit(l, &i, "\"round\":", 8)) {
      const uint64_t d0 = i;
      uint64_t r = 0;
      while (i < l.len && l.p[i] >= '0' && l.p[i] <= '9') {
        const uint32_t d = l.p[i] - '0';
        if (i - d0 >= 20 || r > (~0ull - d) / 10) return false;
        r = r * 10 + d;
        i++;
      }
      if (i == d0 || l.p[d0] == '0') return false;
      out->round = r;
      k = 0;
    } else if (k <= 1 && hj_lit(l, &i, "\"randomness\":\"", 14)) {
      if (!rdjson_hex(l, &i, &out->rand_off, &out->rand_hex)) return false;
      k = 1;
    } else if (k <= 2 && hj_lit(l, &i, "\"signature\":\"", 13)) {
      if (!rdjson_hex(l, &i, &out->sig_off, &out->sig_hex)) return false;
      k = 2;
    } else if (k <= 3 && hj_lit(l, &i, "\"previous_signature\":\"", 22)) {
      if (!rdjson_hex(l, &i, &out->prev_off, &out->prev_hex)) return false;
      k = 3;
    } else {
      return false;
    }
    next = k;
    if (i >= l.len) return false;
    if (l.p[i] == '}') return i + 1 == l.len;
    if (l.p[i] != ',' || k == 3) return false;
    i++;
  }
}

// true = canonical (and *out is set), false = deferred (*out all zero); reads only inside `line`
BOLT_HD bool rdjson_parse(const view& line, rdjson* out) {
  *out = rdjson{0, 0, 0, 0, 0, 0, 0};
  if (rdjson_match(line, out)) return true;
  *out = rdjson{0, 0, 0, 0, 0, 0, 0};
  return false;
}

}  // namespace bolt
}  // namespace dh
