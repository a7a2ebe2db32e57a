// shards_check.cpp -- a stand-alone driver of sct_bam_shards_* (bamshards.cpp) for host sanitizer runs:
//
//   g++ -g -O1 -std=c++17 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -o tools/debug/shards_check tools/debug/shards_check.cpp \
//       sctools_amd/csrc/bamdec.cpp sctools_amd/csrc/bamsplit.cpp sctools_amd/csrc/bamtag.cpp \
//       sctools_amd/csrc/bamshards.cpp -lz
//   tools/debug/shards_check /tmp/shards_check
//
// It writes three BAM shards and one header-less shard in appends cut at odd places (an empty
// shard, a shard of several 0xff00-byte members, an empty append), reads the BAMs back through
// sct_bam_tag_collect, exercises the error returns and the removal of every file on abort and on
// a failed open.  Exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

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

static bool exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0;
}

// an unaligned record with one CR:Z tag of 16 bytes
static void add_record(std::vector<uint8_t>& out, int i) {
  char name[32];
  const int l_name = snprintf(name, sizeof(name), "read%d", i) + 1;
  const uint32_t l_seq = 20;
  std::vector<uint8_t> body(32 + l_name + (l_seq + 1) / 2 + l_seq + 3 + 16 + 1, 0);
  const int32_t minus = -1;
  memcpy(&body[0], &minus, 4), memcpy(&body[4], &minus, 4);
  body[8] = (uint8_t)l_name;
  body[10] = 4680 & 255, body[11] = 4680 >> 8;
  body[14] = 4;
  memcpy(&body[16], &l_seq, 4);
  memcpy(&body[20], &minus, 4), memcpy(&body[24], &minus, 4);
  memcpy(&body[32], name, l_name);
  size_t at = 32 + l_name;
  memset(&body[at], 0x12, (l_seq + 1) / 2), at += (l_seq + 1) / 2;
  memset(&body[at], 30, l_seq), at += l_seq;
  body[at] = 'C', body[at + 1] = 'R', body[at + 2] = 'Z';
  memset(&body[at + 3], "ACGT"[i & 3], 16);
  const uint32_t size = (uint32_t)body.size();
  out.insert(out.end(), (const uint8_t*)&size, (const uint8_t*)&size + 4);
  out.insert(out.end(), body.begin(), body.end());
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s OUT_PREFIX\n", argv[0]);
    return 2;
  }
  const std::string prefix = argv[1];
  const std::string names[4] = {prefix + "_0.bam", prefix + "_1.bam", prefix + "_2.bam", prefix + ".fastq.gz"};
  const char* paths[4] = {names[0].c_str(), names[1].c_str(), names[2].c_str(), names[3].c_str()};
  const char* text = "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tSM:check\n";
  const char* headers[4] = {text, text, text, nullptr};
  sct_bam_shards_t* h = nullptr;
  CHECK(sct_bam_shards_open(nullptr, headers, 4, 6, 2, &h) != 0 && !h);
  CHECK(sct_bam_shards_open(paths, headers, 0, 6, 2, &h) != 0 && !h);
  CHECK(sct_bam_shards_open(paths, headers, 4, 12, 2, &h) != 0 && !h);
  {  // the last file cannot be created: the three before it are removed again
    const std::string nowhere = prefix + "_missing_dir/x.bam";
    const char* bad[4] = {paths[0], paths[1], paths[2], nowhere.c_str()};
    CHECK(sct_bam_shards_open(bad, headers, 4, 6, 2, &h) != 0 && !h);
    CHECK(!exists(names[0]) && !exists(names[1]) && !exists(names[2]));
  }
  CHECK(sct_bam_shards_open(paths, headers, 4, 6, 3, &h) == 0 && h);
  // shard 0 stays empty, shard 1 gets 10 records, shard 2 gets 4000 (several members), the text 300 KB
  std::vector<uint8_t> shard[4];
  const int counts[3] = {0, 10, 4000};
  for (int s = 0; s < 3; s++)
    for (int i = 0; i < counts[s]; i++) add_record(shard[s], i);
  for (int i = 0; i < 20000; i++) {
    char line[64];
    const int k = snprintf(line, sizeof(line), "@r%d\nACGT\n+\nIIII\n", i);
    shard[3].insert(shard[3].end(), line, line + k);
  }
  const int steps = 7;
  for (int step = 0; step < steps; step++) {
    std::vector<uint8_t> data;
    int64_t bounds[5] = {0, 0, 0, 0, 0};
    for (int s = 0; s < 4; s++) {
      const size_t lo = shard[s].size() * step / steps, hi = shard[s].size() * (step + 1) / steps;
      data.insert(data.end(), shard[s].begin() + lo, shard[s].begin() + hi);
      bounds[s + 1] = (int64_t)data.size();
    }
    CHECK(sct_bam_shards_append(h, data.data(), bounds) == 0);
  }
  {
    const int64_t empty[5] = {0, 0, 0, 0, 0}, backwards[5] = {0, 4, 2, 4, 4};
    CHECK(sct_bam_shards_append(h, nullptr, empty) == 0);
    CHECK(sct_bam_shards_append(h, (const uint8_t*)"abcd", backwards) != 0);
    CHECK(sct_bam_shards_append(h, nullptr, backwards) != 0);
    CHECK(sct_bam_shards_append(h, nullptr, nullptr) != 0);
    CHECK(sct_bam_shards_append(nullptr, nullptr, empty) != 0);
  }
  CHECK(sct_bam_shards_close(h) == 0);
  CHECK(sct_bam_shards_close(nullptr) == 0);
  for (int s = 0; s < 3; s++) {
    sct_bam_tags_t* t = nullptr;
    int64_t bad = -1;
    if (counts[s] == 0) {
      CHECK(exists(names[s]));
      continue;
    }
    CHECK(sct_bam_tag_collect(paths[s], "CR", "CB", 16, 2, &t, &bad) == 0);
    CHECK(sct_bam_tag_n(t) == counts[s]);
    const uint8_t* cr = sct_bam_tag_values(t);
    for (int i = 0; i < counts[s]; i++) CHECK(cr[(size_t)i * 16 + 15] == (uint8_t)"ACGT"[i & 3]);
    sct_bam_tag_close(t);
  }
  CHECK(exists(names[3]));
  // abort removes every file
  CHECK(sct_bam_shards_open(paths, nullptr, 4, 1, 1, &h) == 0 && h);
  {
    const int64_t bounds[5] = {0, 1, 2, 3, 4};
    CHECK(sct_bam_shards_append(h, (const uint8_t*)"abcd", bounds) == 0);
  }
  sct_bam_shards_abort(h);
  sct_bam_shards_abort(nullptr);
  for (int s = 0; s < 4; s++) CHECK(!exists(names[s]));
  printf("shards_check: %d + %d + %d records and %zu text bytes, all checks held\n", counts[0], counts[1], counts[2],
         shard[3].size());
  return 0;
}
