// attach_check.cpp -- a stand-alone driver of sct_bam_attach_* (bamtag.cpp) for host sanitizer runs:
//
//   g++ -g -O1 -std=c++17 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -o tools/debug/attach_check tools/debug/attach_check.cpp \
//       sctools_amd/csrc/bamdec.cpp sctools_amd/csrc/bamsplit.cpp sctools_amd/csrc/bamtag.cpp -lz
//   tools/debug/attach_check tests/golden/fastq/test_r2.bam /tmp/attach_check.bam
//
// It attaches four tags in windows of 7 records (one tag listed twice, one with per-record
// lengths that include -1 and 0), asks for more records than the file has, exercises the error
// returns, and reads the output back through sct_bam_tag_collect.  Exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/sct_bam.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, sct_bam_last_error()); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN.bam OUT.bam\n", argv[0]);
    return 2;
  }
  sct_bam_attach_t* h = nullptr;
  CHECK(sct_bam_attach_open("/nonexistent/in.bam", argv[2], 6, 2, &h) != 0 && !h);
  CHECK(sct_bam_attach_open(argv[1], argv[2], 11, 2, &h) != 0 && !h);
  CHECK(sct_bam_attach_open(argv[1], argv[2], 6, 3, &h) == 0 && h);
  const int64_t n = sct_bam_attach_n(h);
  CHECK(n > 20);
  const int64_t window = 7;
  int64_t total = 0;
  for (int64_t at = 0; at < n + window; at += window) {
    std::vector<uint8_t> cr(window * 16), ur(window * 10), cb(window * 16), cr2(window * 16);
    std::vector<int32_t> cb_len(window);
    for (int64_t i = 0; i < window; i++) {
      memset(cr.data() + i * 16, 'A' + (int)((at + i) % 4), 16);
      memset(cr2.data() + i * 16, 'T', 16);
      memset(ur.data() + i * 10, 'G', 10);
      memset(cb.data() + i * 16, 'C', 16);
      cb_len[i] = (at + i) % 3 == 0 ? -1 : (at + i) % 3 == 1 ? 0 : 16;
    }
    const uint8_t* values[4] = {cr.data(), ur.data(), cb.data(), cr2.data()};
    const int64_t strides[4] = {16, 10, 16, 16};
    const int32_t* lengths[4] = {nullptr, nullptr, cb_len.data(), nullptr};
    int64_t wrote = -1;
    CHECK(sct_bam_attach_write(h, window, 4, "CRURCBCR", values, strides, lengths, &wrote) == 0);
    CHECK(wrote == (at + window <= n ? window : at < n ? n - at : 0));
    total += wrote;
  }
  CHECK(total == n);
  {  // errors leave the stream as it is
    std::vector<uint8_t> v(16, 0);
    const uint8_t* values[1] = {v.data()};
    const int64_t strides[1] = {16};
    int64_t wrote = -1;
    CHECK(sct_bam_attach_write(h, 1, 1, "CRX", values, strides, nullptr, &wrote) != 0);
    CHECK(sct_bam_attach_write(h, -1, 1, "CR", values, strides, nullptr, &wrote) != 0);
    CHECK(sct_bam_attach_write(h, 0, 0, nullptr, nullptr, nullptr, nullptr, &wrote) == 0 && wrote == 0);
  }
  CHECK(sct_bam_attach_close(h) == 0);
  CHECK(sct_bam_attach_close(nullptr) == 0);

  // a second pass over the output: existing tags are cut out and set again; NUL bytes and long lengths are refused
  std::string second = std::string(argv[2]) + ".2";
  CHECK(sct_bam_attach_open(argv[2], second.c_str(), 1, 1, &h) == 0);
  {
    std::vector<uint8_t> v((size_t)n * 4, 'N'), z((size_t)n * 4, 0);
    std::vector<int32_t> too_long((size_t)n, 5);
    const uint8_t* values[1] = {z.data()};
    const int64_t strides[1] = {4};
    const int32_t* lengths[1] = {too_long.data()};
    int64_t wrote = -1;
    CHECK(sct_bam_attach_write(h, n, 1, "UR", values, strides, nullptr, &wrote) != 0 && wrote == 0);
    values[0] = v.data();
    CHECK(sct_bam_attach_write(h, n, 1, "UR", values, strides, lengths, &wrote) != 0 && wrote == 0);
    CHECK(sct_bam_attach_write(h, n - 3, 1, "UR", values, strides, nullptr, &wrote) == 0 && wrote == n - 3);
  }
  CHECK(sct_bam_attach_close(h) == 0);

  sct_bam_tags_t* t = nullptr;
  int64_t bad = -1;
  CHECK(sct_bam_tag_collect(argv[2], "CR", "CB", 16, 2, &t, &bad) == 0);
  CHECK(sct_bam_tag_n(t) == n);
  const uint8_t* cr = sct_bam_tag_values(t);
  for (int64_t i = 0; i < n; i++)
    for (int k = 0; k < 16; k++) CHECK(cr[i * 16 + k] == 'T');  // the later CR won
  sct_bam_tag_close(t);
  CHECK(sct_bam_tag_collect(second.c_str(), "UR", "CB", 4, 2, &t, &bad) == 0);
  CHECK(sct_bam_tag_n(t) == n - 3);
  for (int64_t i = 0; i < (n - 3) * 4; i++) CHECK(sct_bam_tag_values(t)[i] == 'N');
  sct_bam_tag_close(t);
  remove(second.c_str());
  printf("attach_check: %lld records, all checks held\n", (long long)n);
  return 0;
}
