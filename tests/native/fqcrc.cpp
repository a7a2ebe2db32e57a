// Host build of the CRC routine of sctools_amd/csrc/fqinflate.h for tests/test_fastq_bgzf_cpu.py: the
// same slices, tables and fold the k_fq_crc32 kernel runs on the device, beside zlib.crc32 in the test.
#include <stdint.h>

#include "../../sctools_amd/csrc/fqinflate.h"

// the gzip CRC-32 of data[0, n) as the wave computes it
extern "C" uint32_t fq_crc32_wave(const uint8_t* data, uint32_t n) { return fqi::crc32_as_the_wave(data, n); }

// got[i] = the CRC of data[off[i], off[i] + len[i])
extern "C" int fq_crc32_many(const uint8_t* data, const int64_t* off, const uint32_t* len, int64_t n, uint32_t* got) {
  for (int64_t i = 0; i < n; i++) got[i] = fqi::crc32_as_the_wave(data + off[i], len[i]);
  return 0;
}

// the pieces, for a test that wants to see them: a * b mod P and x^bits mod P
extern "C" uint32_t fq_gf_mul(uint32_t a, uint32_t b) { return fqi::gf_mul(a, b); }
extern "C" uint32_t fq_gf_xpow(uint64_t bits) { return fqi::gf_xpow(bits); }
