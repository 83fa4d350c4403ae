// Read-only bbolt (go.etcd.io/bbolt, file format v2) page parser shared by the host (plain g++, no HIP) and the
// device: the trimmed beacon store of chain/boltdb/trimmed.go (bucket "beacons", key = round as 8 bytes big-endian,
// value = the raw signature), restated from drand_amd/store.py, which it must agree with; and the value parser of the
// legacy store of chain/boltdb/store.go (value = hexjson Beacon.Marshal(); hexjson_parse below).
//
// Everything is read through bounds-checked little-endian byte accessors over a view {pointer, length}; offsets are
// 64-bit. A structural defect is an error code (bolt::err), never a read outside the view. The leaf functions take a
// view of ONE leaf's extent (the page and its overflow pages, or the inline page inside a bucket value), so the
// kernels can hand them a leaf staged in LDS; a leaf is named by its byte offset in the file, which makes an inline
// bucket just one more leaf.
//
// Page header 16 B {id u64, flags u16, count u16, overflow u32}; meta at page + 16 {magic, version, pageSize, flags,
// root pgid, sequence, freelist, high-water pgid, txid, checksum = FNV-64a of the 56 bytes before it}; leaf element
// 16 B {flags u32, pos u32, ksize u32, vsize u32}, key at element address + pos, value after it, flag 0x01 = nested
// bucket; branch element 16 B {pos u32, ksize u32, pgid u64}; bucket value {root pgid u64, sequence u64}, root 0 =
// inline: a page image follows the 16-byte bucket header inside the value.
#pragma once
#include <stdint.h>

#ifndef BOLT_HD
#if defined(__HIPCC__)
#define BOLT_HD __host__ __device__ inline
#else
#define BOLT_HD inline
#endif
#endif

#include <vector>

namespace dh {
namespace bolt {

enum err : uint32_t {
  OK = 0,
  E_META = 1,      // no valid meta page
  E_PAGE_ID = 2,   // page id at or above the high-water mark, or beyond the file
  E_TRUNC = 3,     // a page's extent (overflow pages included) ends beyond the file / the inline value
  E_COUNT = 4,     // 16 + 16 * count beyond the page's extent
  E_ELEM = 5,      // pos + ksize + vsize beyond the page's extent
  E_FLAGS = 6,     // a page that is neither branch nor leaf where one is required
  E_DEPTH = 7,     // branch depth above MAX_DEPTH
  E_CYCLE = 8,     // a page reached twice
  E_ORDER = 9,     // round keys not strictly ascending
  E_NO_BUCKET = 10,  // the bucket is not in the root bucket
  E_BUCKET = 11,   // a bucket value shorter than its header
};

constexpr uint32_t MAGIC = 0xED0CDAEDu;
constexpr uint16_t F_BRANCH = 0x01, F_LEAF = 0x02, F_META = 0x04;
constexpr uint32_t F_BUCKET = 0x01;  // leaf element flag: nested bucket
constexpr int MAX_DEPTH = 16;

struct view {
  const uint8_t* p;
  uint64_t len;
};

BOLT_HD bool in(const view& f, uint64_t off, uint64_t n) { return off <= f.len && n <= f.len - off; }
// the callers check the range first
BOLT_HD uint32_t rd16(const view& f, uint64_t o) { return (uint32_t)f.p[o] | ((uint32_t)f.p[o + 1] << 8); }
BOLT_HD uint32_t rd32(const view& f, uint64_t o) { return rd16(f, o) | (rd16(f, o + 2) << 16); }
BOLT_HD uint64_t rd64(const view& f, uint64_t o) { return (uint64_t)rd32(f, o) | ((uint64_t)rd32(f, o + 4) << 32); }
BOLT_HD uint64_t rd64be(const view& f, uint64_t o) {
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v = (v << 8) | f.p[o + i];
  return v;
}

struct meta {
  uint32_t page_size;
  uint64_t root, hw, txid;
};

BOLT_HD bool meta_at(const view& f, uint64_t off, meta* m) {
  if (!in(f, off, 80)) return false;
  if (!(rd16(f, off + 8) & F_META) || rd32(f, off + 16) != MAGIC || rd32(f, off + 20) != 2) return false;
  uint64_t h = 0xcbf29ce484222325ull;
  for (int i = 16; i < 72; i++) h = (h ^ f.p[off + i]) * 0x100000001b3ull;
  if (h != rd64(f, off + 72)) return false;
  m->page_size = rd32(f, off + 24);
  m->root = rd64(f, off + 32);
  m->hw = rd64(f, off + 56);
  m->txid = rd64(f, off + 64);
  // a page holds at least its header and one element, and page arithmetic must not degenerate
  return m->page_size >= 64 && m->page_size <= (1u << 24);
}

// The valid meta of pages 0 / 1 with the larger txid (page 1 lies at the page size that page 0's meta names, as
// store.py's reader places it).
BOLT_HD uint32_t bolt_meta(const view& f, meta* out) {
  const uint64_t guess = in(f, 24, 4) ? rd32(f, 24) : 4096;
  meta m[2];
  bool ok0 = meta_at(f, 0, &m[0]), ok1 = meta_at(f, guess, &m[1]);
  if (!ok0 && !ok1) return E_META;
  *out = (ok0 && (!ok1 || m[0].txid >= m[1].txid)) ? m[0] : m[1];
  return OK;
}

struct page {
  uint64_t off, ext;  // byte offset in the file, bytes the page spans (overflow pages included)
  uint32_t flags, count;
};

BOLT_HD uint32_t bolt_page(const view& f, const meta& m, uint64_t pgid, page* pg) {
  if (pgid >= m.hw || pgid > f.len / m.page_size) return E_PAGE_ID;
  const uint64_t off = pgid * (uint64_t)m.page_size;
  if (!in(f, off, 16)) return E_PAGE_ID;
  const uint64_t span = (uint64_t)rd32(f, off + 12) + 1;
  if (span > m.hw - pgid) return E_PAGE_ID;
  if (!in(f, off, span * m.page_size)) return E_TRUNC;
  pg->off = off;
  pg->ext = span * m.page_size;
  pg->flags = rd16(f, off + 8);
  pg->count = rd16(f, off + 10);
  if (16 + 16 * (uint64_t)pg->count > pg->ext) return E_COUNT;
  return OK;
}

// ---- leaves: `leaf` is a view of the leaf's own extent

BOLT_HD uint32_t bolt_leaf_head(const view& leaf, uint32_t* count) {
  if (!in(leaf, 0, 16)) return E_TRUNC;
  if (!(rd16(leaf, 8) & F_LEAF)) return E_FLAGS;
  *count = rd16(leaf, 10);
  if (16 + 16 * (uint64_t)*count > leaf.len) return E_COUNT;
  return OK;
}

struct elem {
  uint32_t flags, ksize, vsize;
  uint64_t koff;  // key offset inside the leaf; the value follows at koff + ksize
};
BOLT_HD bool is_round(const elem& e) { return e.ksize == 8 && !(e.flags & F_BUCKET); }

// element i < count of a leaf whose head passed bolt_leaf_head
BOLT_HD uint32_t bolt_leaf_elem(const view& leaf, uint32_t i, elem* e) {
  const uint64_t eo = 16 + 16 * (uint64_t)i;
  e->flags = rd32(leaf, eo);
  e->ksize = rd32(leaf, eo + 8);
  e->vsize = rd32(leaf, eo + 12);
  e->koff = eo + rd32(leaf, eo + 4);
  if (!in(leaf, e->koff, (uint64_t)e->ksize + e->vsize)) return E_ELEM;
  return OK;
}

// What the scan keeps per leaf (40 bytes). n_all counts what BoltFile.bucket keeps: every element but nested buckets.
struct leaf_info {
  uint64_t off;
  uint64_t first, last;  // smallest / largest round (n_round > 0)
  uint32_t n_round, n_all, max_vsize, err;
};
static_assert(sizeof(leaf_info) == 40, "leaf table record");

BOLT_HD void info_init(leaf_info* a) {
  a->first = ~0ull;
  a->last = 0;
  a->n_round = a->n_all = a->max_vsize = a->err = 0;
}
BOLT_HD void info_merge(leaf_info* a, uint64_t first, uint64_t last, uint32_t n_round, uint32_t n_all, uint32_t max_vsize,
                        uint32_t err) {
  if (first < a->first) a->first = first;
  if (last > a->last) a->last = last;
  a->n_round += n_round;
  a->n_all += n_all;
  if (max_vsize > a->max_vsize) a->max_vsize = max_vsize;
  if (!a->err) a->err = err;
}

// Validate elements i0, i0 + step, ... of a leaf and accumulate their statistics into *acc (info_init first). The
// host calls it with (0, 1); the scan kernel with (lane, 64) and merges the lanes. A round key must exceed the nearest
// round key before it.
BOLT_HD void bolt_leaf_check(const view& leaf, uint32_t count, uint32_t i0, uint32_t step, leaf_info* acc) {
  for (uint32_t i = i0; i < count; i += step) {
    elem e;
    uint32_t rc = bolt_leaf_elem(leaf, i, &e);
    if (rc) {
      if (!acc->err) acc->err = rc;
      continue;
    }
    if (!(e.flags & F_BUCKET)) acc->n_all++;
    if (!is_round(e)) continue;
    const uint64_t r = rd64be(leaf, e.koff);
    for (uint32_t j = i; j-- > 0;) {
      elem p;
      if (bolt_leaf_elem(leaf, j, &p) || !is_round(p)) continue;
      if (rd64be(leaf, p.koff) >= r && !acc->err) acc->err = E_ORDER;
      break;
    }
    info_merge(acc, r, r, 1, 0, e.vsize, 0);
  }
}

// ---- hexjson values: the legacy store of chain/boltdb/store.go, value = Beacon.Marshal()
//
// Only the canonical form is decoded: exactly {"PreviousSig":P,"Round":D,"Signature":S} with nothing before, between
// or after; P and S are null or a quoted even number (0 allowed) of characters 0-9a-f; D is a decimal of 1-20 digits
// without a leading zero (0 itself excepted) that fits 64 bits and equals the record's key. Every other value is
// DEFERRED: nothing is decided about it here, the caller's host decoder does. Offsets are inside the value; the hex
// lengths count characters (null and "": 0).
struct hexjson {
  uint32_t prev_off, prev_hex, sig_off, sig_hex;
};

BOLT_HD bool hj_lit(const view& v, uint64_t* i, const char* s, uint32_t n) {
  if (!in(v, *i, n)) return false;
  for (uint32_t k = 0; k < n; k++)
    if (v.p[*i + k] != (uint8_t)s[k]) return false;
  *i += n;
  return true;
}
BOLT_HD bool hj_hex(uint32_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f'); }
BOLT_HD bool hj_field(const view& v, uint64_t* i, uint32_t* off, uint32_t* hex) {
  *off = *hex = 0;
  if (*i >= v.len) return false;
  if (v.p[*i] == 'n') return hj_lit(v, i, "null", 4);
  if (v.p[*i] != '"') return false;
  uint64_t j = *i + 1;
  while (j < v.len && hj_hex(v.p[j])) j++;
  if (j >= v.len || v.p[j] != '"' || ((j - *i - 1) & 1)) return false;
  *off = (uint32_t)(*i + 1);
  *hex = (uint32_t)(j - *i - 1);
  *i = j + 1;
  return true;
}

BOLT_HD bool hexjson_match(const view& val, uint64_t key, hexjson* out) {
  if (val.len > 0xffffffffull) return false;
  uint64_t i = 0;
  if (!hj_lit(val, &i, "{\"PreviousSig\":", 15) || !hj_field(val, &i, &out->prev_off, &out->prev_hex)) return false;
  if (!hj_lit(val, &i, ",\"Round\":", 9)) return false;
  const uint64_t d0 = i;
  uint64_t r = 0;
  while (i < val.len && val.p[i] >= '0' && val.p[i] <= '9') {
    const uint32_t d = val.p[i] - '0';
    if (i - d0 >= 20 || r > (~0ull - d) / 10) return false;
    r = r * 10 + d;
    i++;
  }
  if (i == d0 || (i - d0 > 1 && val.p[d0] == '0') || r != key) return false;
  if (!hj_lit(val, &i, ",\"Signature\":", 13) || !hj_field(val, &i, &out->sig_off, &out->sig_hex)) return false;
  return hj_lit(val, &i, "}", 1) && i == val.len;
}
// true = canonical (and *out is set), false = deferred (*out all zero); reads only inside `val`
BOLT_HD bool hexjson_parse(const view& val, uint64_t key, hexjson* out) {
  if (hexjson_match(val, key, out)) return true;
  out->prev_off = out->prev_hex = out->sig_off = out->sig_hex = 0;
  return false;
}

// the byte two validated hex characters at `o` spell
BOLT_HD uint32_t hj_nib(uint32_t c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
BOLT_HD uint32_t hj_byte(const view& v, uint64_t o) { return (hj_nib(v.p[o]) << 4) | hj_nib(v.p[o + 1]); }

// What the hexjson scan adds per leaf (16 bytes): deferred round records, the longest decoded Signature / PreviousSig
struct leaf_json {
  uint32_t n_deferred, max_sig, max_prev, pad;
};

// the value of a round element of `leaf`
BOLT_HD view elem_value(const view& leaf, const elem& e) { return view{leaf.p + e.koff + e.ksize, e.vsize}; }

// a leaf by its byte offset in the file and the bytes it spans
struct leaf_ref {
  uint64_t off, ext;
};

// ---- host only: the branch walk

// Leaves under the page `root`, depth-first in key order (iterative; MAX_DEPTH branch levels; every page once).
inline uint32_t bolt_leaf_list(const view& f, const meta& m, uint64_t root, std::vector<leaf_ref>* out) {
  struct frame {
    page pg;
    uint32_t next;
  };
  std::vector<bool> seen(f.len / m.page_size + 1, false);
  frame st[MAX_DEPTH + 1];
  int depth = 0;
  auto enter = [&](uint64_t pgid, frame* fr) -> uint32_t {
    uint32_t rc = bolt_page(f, m, pgid, &fr->pg);
    if (rc) return rc;
    if (seen[pgid]) return E_CYCLE;
    seen[pgid] = true;
    fr->next = 0;
    return OK;
  };
  uint32_t rc = enter(root, &st[0]);
  if (rc) return rc;
  for (;;) {
    frame& fr = st[depth];
    if (fr.pg.flags & F_LEAF) {
      out->push_back({fr.pg.off, fr.pg.ext});
    } else if (fr.pg.flags & F_BRANCH) {
      if (fr.next < fr.pg.count) {
        const uint64_t eo = fr.pg.off + 16 + 16 * (uint64_t)fr.next++;
        if (eo - fr.pg.off + rd32(f, eo) + rd32(f, eo + 4) > fr.pg.ext) return E_ELEM;  // the separator key
        if (depth == MAX_DEPTH) return E_DEPTH;
        if ((rc = enter(rd64(f, eo + 8), &st[depth + 1]))) return rc;
        depth++;
        continue;
      }
    } else {
      return E_FLAGS;
    }
    if (depth-- == 0) return OK;
  }
}

// The bucket `name` of the root bucket: the first element of that key carrying the bucket flag, as BoltFile.bucket
// takes it; its leaves in key order (an inline bucket: the one page inside the value).
inline uint32_t bolt_find_bucket(const view& f, const meta& m, const uint8_t* name, uint32_t nlen,
                                 std::vector<leaf_ref>* leaves) {
  std::vector<leaf_ref> top;
  uint32_t rc = bolt_leaf_list(f, m, m.root, &top);
  if (rc) return rc;
  for (const leaf_ref& lr : top) {
    const view leaf{f.p + lr.off, lr.ext};
    uint32_t count;
    if ((rc = bolt_leaf_head(leaf, &count))) return rc;
    for (uint32_t i = 0; i < count; i++) {
      elem e;
      if ((rc = bolt_leaf_elem(leaf, i, &e))) return rc;
      if (!(e.flags & F_BUCKET) || e.ksize != nlen) continue;
      bool same = true;
      for (uint32_t k = 0; k < nlen && same; k++) same = leaf.p[e.koff + k] == name[k];
      if (!same) continue;
      if (e.vsize < 16) return E_BUCKET;
      const uint64_t voff = e.koff + e.ksize, broot = rd64(leaf, voff);
      if (broot) return bolt_leaf_list(f, m, broot, leaves);
      if (e.vsize < 32) return E_TRUNC;
      leaves->push_back({lr.off + voff + 16, (uint64_t)e.vsize - 16});
      return OK;
    }
  }
  return E_NO_BUCKET;
}

inline const char* err_name(uint32_t e) {
  static const char* n[] = {"ok", "no valid meta page", "page id beyond the high-water mark or the file",
                            "page extent beyond the file", "element count beyond the page", "element beyond the page",
                            "page is neither branch nor leaf", "branch depth above 16", "page reached twice",
                            "round keys not ascending", "bucket not found", "bucket value too short"};
  return e < sizeof n / sizeof n[0] ? n[e] : "unknown";
}

}  // namespace bolt
}  // namespace dh
