// Host build of sctools_amd/csrc/tsround.h for tests/test_tagsort_native_cpu.py (the same header
// the HIP kernels use on the device), beside glibc's own text round trip of the float32 quotient.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../sctools_amd/csrc/tsround.h"

// got[i] = ts_roundtrip(a[i], b[i]); want[i] = bits of strtof(snprintf("%g", (float)a / (float)b))
extern "C" int ts_roundtrip_pairs(const uint32_t* a, const uint32_t* b, int64_t n, uint32_t* got, uint32_t* want) {
  for (int64_t i = 0; i < n; i++) {
    got[i] = sct::ts_roundtrip(a[i], b[i]);
    volatile float fa = (float)a[i], fb = (float)b[i];
    const float q = fa / fb;
    char buf[64];
    snprintf(buf, sizeof(buf), "%g", q);
    const float y = strtof(buf, nullptr);
    memcpy(&want[i], &y, 4);
  }
  return 0;
}
