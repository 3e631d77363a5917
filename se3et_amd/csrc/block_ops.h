// The building blocks the geometry kernels share (common.h includes this file): the wave sum, the single-workgroup prefix scan, the
// block-wide bounding box and the host-side workspace carver.  Everything is a template or an inline function, so every file
// that includes common.h sees the same text and the link sees no duplicate.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// sum over the 64 lanes of a wave, in every lane (float, double, int, long long); a fixed butterfly: the same bits on every run
template <class T>
__device__ __forceinline__ T se3_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- prefix scan over one workgroup of THREADS threads ---------------------------------------------------------------------------------
// Every thread hands in one value and gets back the sum of the values of the threads before it; *total is the sum of all of them.
// sh: THREADS entries of LDS.  A Hillis-Steele pass over the values; the barrier in front lets a caller reuse `sh` from call to call.
template <class T, int THREADS = 1024>
__device__ __forceinline__ T se3_block_exclusive(T value, T* sh, T* total) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = value;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    const T v = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  *total = sh[THREADS - 1];
  return sh[t] - value;
}

enum Se3Scan { kSe3ScanExclusive, kSe3ScanInclusive, kSe3ScanSuffix };

// Prefix sum of a[0, n) in place by one workgroup and the total as the return value: each thread sums a consecutive chunk, the chunk sums
// are scanned by se3_block_exclusive, each thread writes its chunk back.  Exclusive: a[i] = sum of a[j < i]; Inclusive: j <= i; Suffix:
// j > i (the exclusive scan from the far end).  a[] is visible to the whole workgroup on return.
template <Se3Scan MODE, class T, class Index, int THREADS = 1024>
__device__ __forceinline__ T se3_block_scan(T* a, Index n, T* sh) {
  const Index t = threadIdx.x, chunk = (n + THREADS - 1) / THREADS;
  const Index lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  T sum = 0, total;
  for (Index i = lo; i < hi; i++) sum += a[MODE == kSe3ScanSuffix ? n - 1 - i : i];
  T run = se3_block_exclusive<T, THREADS>(sum, sh, &total);
  for (Index i = lo; i < hi; i++) {
    const Index at = MODE == kSe3ScanSuffix ? n - 1 - i : i;
    const T v = a[at];
    a[at] = MODE == kSe3ScanInclusive ? run + v : run;
    run += v;
  }
  __syncthreads();
  return total;
}

// a[0, n) counts -> exclusive offsets, a[n] = total (int64, on `stream`; csrc/capi_common.hip holds the kernel)
void se3_exclusive_scan_i64(int64_t* a, int64_t n, hipStream_t stream);

// ---- bounding box over one workgroup of THREADS threads ----------------------------------------------------------------------------------
// Every thread hands in the min and max of the points it met (+inf / -inf if none: fmin and fmax drop a NaN, so neither is ever NaN) and
// gets back the workgroup's.  The maxima are reduced as the minima of their negatives.  sh: THREADS / 64 entries of LDS.
__device__ __forceinline__ float se3_fmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double se3_fmin(double a, double b) { return fmin(a, b); }

template <class T, int THREADS>
__device__ __forceinline__ void se3_block_bounds(T* mn, T* mx, T* sh) {
#pragma unroll
  for (int d = 0; d < 6; d++) {
    T v = d < 3 ? mn[d] : -mx[d - 3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = se3_fmin(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = sh[0];
    for (int w = 1; w < THREADS / 64; w++) t = se3_fmin(t, sh[w]);
    if (d < 3) mn[d] = t;
    else mx[d - 3] = -t;
  }
}

// ---- host side: a workspace as a sequence of 256-byte aligned arrays -----------------------------------------------------------------------
inline size_t se3_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// take<T>(count) hands out the next array; a null base only measures.  bytes(): the size of everything taken, rounded up.
struct Se3Carver {
  char* base;
  size_t off = 0;
  explicit Se3Carver(void* b) : base((char*)b) {}
  template <class T>
  T* take(size_t count) {
    off = se3_align256(off);
    T* p = base ? (T*)(base + off) : nullptr;
    off += sizeof(T) * count;
    return p;
  }
  size_t bytes() const { return se3_align256(off); }
};
