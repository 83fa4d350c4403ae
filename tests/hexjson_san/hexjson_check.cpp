// Stand-alone host driver of the hexjson value parser in drand_amd/csrc/bolt.hpp for the sanitizer build
// (tests/hexjson_san/Makefile, run by tests/test_bolt_json_host.py): hexjson_parse and hj_byte, the calls the store
// kernels make, over values in exact-size heap buffers, so that any read outside the value is an AddressSanitizer
// report.
//   hexjson_check CORPUS     CORPUS = records {key u64 LE, length u32 LE, value bytes}; one line per record:
//                            "C <sig bytes> <prev bytes> <sig hex or -> <prev hex or ->" (canonical, decoded and
//                            printed again as hex) or "D" (deferred)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../drand_amd/csrc/bolt.hpp"

using namespace dh::bolt;

// decoded the way k_bolt_gather_json writes a row: dword w of a stride-wide row from 8 hex characters, zero-padded
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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) {
    perror(argv[1]);
    return 2;
  }
  for (;;) {
    uint8_t hdr[12];
    if (fread(hdr, 1, 12, fp) != 12) break;
    uint64_t key = 0;
    uint32_t len = 0;
    for (int i = 7; i >= 0; i--) key = (key << 8) | hdr[i];
    for (int i = 3; i >= 0; i--) len = (len << 8) | hdr[8 + i];
    // an exact-size heap buffer: one byte past the end is a sanitizer report
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, fp) != len) return 2;
    const view v{buf, len};
    hexjson h;
    if (hexjson_parse(v, key, &h)) {
      printf("C %u %u %s %s\n", h.sig_hex / 2, h.prev_hex / 2, decode(v, h.sig_off, h.sig_hex).c_str(),
             decode(v, h.prev_off, h.prev_hex).c_str());
    } else {
      if (h.sig_off | h.sig_hex | h.prev_off | h.prev_hex) {
        fprintf(stderr, "a deferred value left offsets behind\n");
        return 3;
      }
      printf("D\n");
    }
    free(buf);
  }
  fclose(fp);
  return 0;
}
