// Stand-alone host driver of the RandomData record parser in drand_amd/csrc/rdjson.hpp for the sanitizer build
// (tests/rdjson_san/Makefile, run by tests/test_archive_host.py): rdjson_parse and hj_byte, the calls the archive
// kernels make, over lines in exact-size heap buffers, so that any read outside the line is an AddressSanitizer report.
//   rdjson_check CORPUS      CORPUS = records {length u32 LE, line bytes}; one output line per record:
//                            "C <round> <randomness hex or -> <signature hex or -> <previous_signature hex or ->"
//                            (canonical, decoded and printed again as hex) or "D" (deferred)
//   rdjson_check -f FILE     the framing of a whole buffer, as the index kernels define it: "<offset> <length>" per record
//                            (a line above 4096 bytes: length 4097), or "A" for the JSON-array form
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../drand_amd/csrc/rdjson.hpp"

using namespace dh::bolt;

// decoded the way k_ndjson_gather writes a row: dword w of a stride-wide row from 8 hex characters, zero-padded
static std::string decode(const view& v, uint32_t off, uint32_t hex) {
  const uint32_t nb = hex / 2, stride = (nb + 3) & ~3u;
  std::vector<uint8_t> row(stride, 0xAA);
  for (uint32_t w = 0; w < stride / 4; w++) {
    uint32_t word = 0;
    for (uint32_t j = 0; j < 4; j++)
      if (4 * w + j < nb) word |= hj_byte(v, off + 8 * (uint64_t)w + 2 * j) << (8 * j);
    memcpy(&row[4 * w], &word, 4);
  }
  for (uint32_t k = nb; k < stride; k++)
    if (row[k]) {
      fprintf(stderr, "padding byte %u is not zero\n", k);
      exit(3);
    }
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint32_t k = 0; k < nb; k++) {
    s += d[row[k] >> 4];
    s += d[row[k] & 15];
  }
  return s.empty() ? "-" : s;
}

static int framing(const char* path) {
  FILE* fp = fopen(path, "rb");
  if (!fp) {
    perror(path);
    return 2;
  }
  fseek(fp, 0, SEEK_END);
  const long len = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
  if (len && fread(buf, 1, len, fp) != (size_t)len) return 2;
  fclose(fp);
  const view f{buf, (uint64_t)len};
  if (rdjson_is_array(f)) {
    printf("A\n");
  } else {
    for (uint64_t i = 0; i < f.len; i++) {
      if (!rdjson_starts(f, i)) continue;
      uint64_t n = 0;
      while (i + n < f.len && f.p[i + n] != '\n' && n <= RDJSON_MAX_LINE) n++;
      printf("%llu %llu\n", (unsigned long long)i, (unsigned long long)n);
    }
  }
  free(buf);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "-f")) return framing(argv[2]);
  if (argc != 2) return 2;
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) {
    perror(argv[1]);
    return 2;
  }
  for (;;) {
    uint8_t hdr[4];
    if (fread(hdr, 1, 4, fp) != 4) break;
    uint32_t len = 0;
    for (int i = 3; i >= 0; i--) len = (len << 8) | hdr[i];
    // an exact-size heap buffer: one byte past the end is a sanitizer report
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, fp) != len) return 2;
    const view v{buf, len};
    rdjson r;
    if (rdjson_parse(v, &r)) {
      printf("C %llu %s %s %s\n", (unsigned long long)r.round, decode(v, r.rand_off, r.rand_hex).c_str(),
             decode(v, r.sig_off, r.sig_hex).c_str(), decode(v, r.prev_off, r.prev_hex).c_str());
    } else {
      if (r.round | r.rand_off | r.rand_hex | r.sig_off | r.sig_hex | r.prev_off | r.prev_hex) {
        fprintf(stderr, "a deferred line left fields behind\n");
        return 3;
      }
      printf("D\n");
    }
    free(buf);
  }
  fclose(fp);
  return 0;
}
