// Error reporting and version entry points of the C ABI, and the one kernel of block_ops.h that is not a template.
#include <stdarg.h>
#include "common.h"

static thread_local char g_err[512] = "";

void se3_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* se3_last_error(void) { return g_err; }
extern "C" const char* se3_version(void) { return "se3et_hip 0.1 (gfx950)"; }

namespace {
__global__ __launch_bounds__(1024) void exclusive_scan_i64_kernel(int64_t* __restrict__ a, int64_t n) {
  __shared__ int64_t sh[1024];
  const int64_t total = se3_block_scan<kSe3ScanExclusive>(a, n, sh);
  if (threadIdx.x == 0) a[n] = total;
}
}  // namespace

void se3_exclusive_scan_i64(int64_t* a, int64_t n, hipStream_t stream) { exclusive_scan_i64_kernel<<<1, 1024, 0, stream>>>(a, n); }
