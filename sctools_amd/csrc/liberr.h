// liberr.h -- the error state of a stand-alone library (barcode.hip, fastq.hip with fqmetrics.h,
// gbam.hip): one thread-local message that the library's *_last_error() returns, fail() to set
// it and hand back the call's return code, and SCT_LIB_HIP for a HIP runtime call.  Host code
// only.  The engine (util.h) and the host BAM decoder (bgzf.h) keep their own: the engine's
// fail() is tied to its profiler scopes.
//
// Each of these libraries is one translation unit, so the state lives in an unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <string>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace

// returns `code` from the calling function, with the failed call's text and HIP's message
#define SCT_LIB_HIP(code, call)                                                          \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) return fail((code), "%s: %s", #call, hipGetErrorString(e_));   \
  } while (0)
