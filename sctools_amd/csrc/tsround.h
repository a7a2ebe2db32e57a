// tsround.h -- the value the native TagSort gatherer sees for a per-read quality ratio.
//
// The reference's per-read stage (fastqpreprocessing/src/htslib_tagsort.cpp:126-187) divides
// two float32 integers, writes the quotient to a temporary text file with operator<<(float)
// ("%g": six significant digits) and the gatherer reads it back with std::stof
// (metricgatherer.cpp:44-49).  So the value that enters the sums is
//     strtof(sprintf("%g", (float)a / (float)b)).
// ts_roundtrip computes exactly that from the integer pair (a, b), a, b < 2^16, in integer
// arithmetic: the correctly rounded float32 quotient q = m * 2^e, its exact round-half-even
// to six significant decimal digits D * 10^(k-5) (what glibc's printf produces from the exact
// binary value), and the correctly rounded float32 of that decimal (what strtof produces).
//
// Used by the HIP kernels (device) and compiled on the host by the tests.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SCT_TS_HD __host__ __device__ __forceinline__
#else
#define SCT_TS_HD static inline
#endif

namespace sct {

constexpr uint32_t kTsNan = 0xFFC00000u;  // 0/0 on x86: the default NaN has its sign set ("-nan")
constexpr uint32_t kTsInf = 0x7F800000u;

SCT_TS_HD int ts_bitlen(uint64_t x) {  // x > 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 64 - __clzll((long long)x);
#else
  return 64 - __builtin_clzll(x);
#endif
}

// RN_float32(a / b) as mantissa m in [2^23, 2^24) and exponent e (value m * 2^e); 0 < a < 2^36, 0 < b < 2^36.
SCT_TS_HD void ts_rn_div(uint64_t a, uint64_t b, uint32_t* m, int* e) {
  const int sh = 25 + ts_bitlen(b) - ts_bitlen(a);  // (a << sh) / b in [2^24, 2^26); sh <= 60 - bitlen(a)
  uint64_t num, den;
  if (sh >= 0) {
    num = a << sh, den = b;
  } else {
    num = a, den = b << -sh;
  }
  const uint64_t q = num / den;
  const bool sticky = q * den != num;
  const int drop = ts_bitlen(q) - 24;  // 1 or 2
  const uint64_t low = q & ((1ull << drop) - 1), half = 1ull << (drop - 1);
  uint64_t mant = q >> drop;
  if (low > half || (low == half && (sticky || (mant & 1)))) mant++;
  int ex = drop - sh;
  if (mant == (1ull << 24)) {
    mant >>= 1;
    ex++;
  }
  *m = (uint32_t)mant;
  *e = ex;
}

// float32 bit pattern of strtof(sprintf("%g", (float)a / (float)b)); a, b < 2^16.
SCT_TS_HD uint32_t ts_roundtrip(uint32_t a, uint32_t b) {
  if (b == 0) return a == 0 ? kTsNan : kTsInf;
  if (a == 0) return 0u;
  uint32_t m;
  int e;
  ts_rn_div(a, b, &m, &e);  // q = m * 2^e in [2^-16, 2^16): e in [-39, -8]
  const int s = -e;
  // k = floor(log10 q), the largest k with m * 10^(5-k) >= 10^5 * 2^s (all exact in 64 bits:
  // m * 10^10 < 2^58, 10^6 * 2^39 < 2^59)
  uint64_t p10 = 10;  // 10^(5-k), k = 4
  int k = 4;
  uint64_t nn = (uint64_t)m * p10;
  const uint64_t lo = 100000ull << s;
  while (nn < lo) {
    p10 *= 10;
    k--;
    nn = (uint64_t)m * p10;
  }
  uint64_t d = nn >> s;
  const uint64_t rem = nn & ((1ull << s) - 1), half = 1ull << (s - 1);
  if (rem > half || (rem == half && (d & 1))) d++;
  if (d == 1000000ull) {
    d = 100000ull;
    k++;
  }
  // y = RN_float32(d / 10^(5-k)); 5 - k in [0, 10]
  uint64_t den = 1;
  for (int i = 0; i < 5 - k; i++) den *= 10;
  ts_rn_div(d, den, &m, &e);
  return ((uint32_t)(e + 23 + 127) << 23) | (m & 0x7FFFFFu);
}

}  // namespace sct
