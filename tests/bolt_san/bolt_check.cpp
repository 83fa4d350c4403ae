// Stand-alone host driver of drand_amd/csrc/bolt.hpp for the sanitizer build (tests/bolt_san/Makefile, run by
// tests/test_bolt_host.py): the same meta / bucket / branch walk dh_bolt_index runs and the same bolt_leaf_check /
// bolt_leaf_elem calls the store kernels make, over files loaded into exact-size heap buffers, so that any read
// outside [file, file + len) is an AddressSanitizer report.
//   bolt_check FILE...                  one line per file
//   bolt_check --sweep FILE OFF N      FILE with each of the N bytes from OFF set to 0x00, 0xFF and +1, one line each
// A line is "OK <page size> <leaves> <len> <rounds> <digest>" or "ERR <code> <name>". The digest is FNV-64a over
// (ksize u32 LE, vsize u32 LE, key, value) of every element that is not a nested bucket, in walk order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../drand_amd/csrc/bolt.hpp"

using namespace dh::bolt;

static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

static bool same(const leaf_info& a, const leaf_info& b) {
  return a.n_round == b.n_round && a.n_all == b.n_all && a.max_vsize == b.max_vsize && !a.err == !b.err &&
         (!a.n_round || (a.first == b.first && a.last == b.last));
}

static uint32_t check(const uint8_t* buf, size_t len, char* line, size_t cap) {
  const view f{buf, (uint64_t)len};
  meta m;
  uint32_t rc = bolt_meta(f, &m);
  if (rc) return rc;
  std::vector<leaf_ref> leaves;
  if ((rc = bolt_find_bucket(f, m, (const uint8_t*)"beacons", 7, &leaves))) return rc;
  uint64_t n_all = 0, n_round = 0, h = 0xcbf29ce484222325ull, prev_last = 0;
  bool have_prev = false;
  for (const leaf_ref& lr : leaves) {
    if (!in(f, lr.off, lr.ext)) return E_TRUNC;  // what the host hands the kernels must lie inside the file
    const view leaf{buf + lr.off, lr.ext};
    uint32_t count = 0;
    if ((rc = bolt_leaf_head(leaf, &count))) return rc;
    leaf_info one;
    info_init(&one);
    bolt_leaf_check(leaf, count, 0, 1, &one);
    // the scan kernel's form: 64 lanes, merged
    leaf_info wave;
    info_init(&wave);
    for (uint32_t lane = 0; lane < 64; lane++) {
      leaf_info a;
      info_init(&a);
      bolt_leaf_check(leaf, count, lane, 64, &a);
      info_merge(&wave, a.first, a.last, a.n_round, a.n_all, a.max_vsize, a.err);
    }
    if (!same(one, wave)) {
      fprintf(stderr, "lane-split check disagrees with the serial one at leaf offset %llu\n", (unsigned long long)lr.off);
      exit(3);
    }
    if (one.err) return one.err;
    if (one.n_round) {
      if (have_prev && prev_last >= one.first) return E_ORDER;
      prev_last = one.last;
      have_prev = true;
    }
    n_all += one.n_all;
    n_round += one.n_round;
    for (uint32_t i = 0; i < count; i++) {
      elem e;
      if ((rc = bolt_leaf_elem(leaf, i, &e))) return rc;
      if (e.flags & F_BUCKET) continue;
      const uint8_t hdr[8] = {(uint8_t)e.ksize, (uint8_t)(e.ksize >> 8), (uint8_t)(e.ksize >> 16), (uint8_t)(e.ksize >> 24),
                              (uint8_t)e.vsize, (uint8_t)(e.vsize >> 8), (uint8_t)(e.vsize >> 16), (uint8_t)(e.vsize >> 24)};
      h = fnv(h, hdr, 8);
      h = fnv(h, leaf.p + e.koff, (size_t)e.ksize + e.vsize);
    }
  }
  snprintf(line, cap, "OK %u %zu %llu %llu %016llx", m.page_size, leaves.size(), (unsigned long long)n_all,
           (unsigned long long)n_round, (unsigned long long)h);
  return OK;
}

static void report(const uint8_t* src, size_t len) {
  // an exact-size heap copy: one byte past the end is a sanitizer report
  uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
  memcpy(buf, src, len);
  char line[256];
  const uint32_t rc = check(buf, len, line, sizeof line);
  if (rc)
    printf("ERR %u %s\n", rc, err_name(rc));
  else
    printf("%s\n", line);
  free(buf);
}

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* fp = fopen(path, "rb");
  if (!fp) {
    perror(path);
    exit(2);
  }
  uint8_t tmp[65536];
  size_t k;
  while ((k = fread(tmp, 1, sizeof tmp, fp)) > 0) v.insert(v.end(), tmp, tmp + k);
  fclose(fp);
  return v;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "--sweep")) {
    std::vector<uint8_t> v = slurp(argv[2]);
    const size_t off = strtoull(argv[3], nullptr, 10), n = strtoull(argv[4], nullptr, 10);
    for (size_t i = off; i < off + n && i < v.size(); i++) {
      const uint8_t orig = v[i];
      const uint8_t muts[3] = {0x00, 0xFF, (uint8_t)(orig + 1)};
      for (uint8_t mu : muts) {
        v[i] = mu;
        report(v.data(), v.size());
      }
      v[i] = orig;
    }
    return 0;
  }
  for (int a = 1; a < argc; a++) {
    std::vector<uint8_t> v = slurp(argv[a]);
    report(v.data(), v.size());
  }
  return 0;
}
