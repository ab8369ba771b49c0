// cfa_grad_common.h — what the TF1 model-graph kernels share below the graphs themselves
// (cfa_tf1_graph.h has the graphs' phases and geometry): the clip bounds of the cost, TF's SAME
// padding, the softmax lane width, the workgroup size, the global -> LDS copy and the dynamic-LDS
// limit of a kernel. Not installed, not an ABI.
#pragma once
#include "cfa_internal.h"

namespace {

constexpr float kClipLo = 1e-15f, kClipHi = 0.99f;

__host__ __device__ inline int same_left(int L, int k, int s) {
  const int out = (L + s - 1) / s;
  const int total = max((out - 1) * s + k - L, 0);
  return total / 2;
}

// lanes per sample of softmax_xent: the power of two >= C (C <= 64, checked on the host)
inline int softmax_width(int C) {
  int w = 1;
  while (w < C) w <<= 1;
  return w;
}

constexpr int kGradBlock = 512;  // 8 waves: these graphs are latency-bound, not ALU-bound

// Copy n floats global -> LDS with every load of a thread issued before its first store (the
// graphs are tiny, so serialized global latency, not bandwidth, would dominate). The tail is
// predicated rather than looped, so a copy of up to U * T floats is one round trip.
__device__ __forceinline__ void stage(float* dst, const float* src, int n, int tid, int T) {
  constexpr int U = 8;
  for (int i = tid; i < n; i += U * T) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = i + u * T < n ? src[i + u * T] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * T < n) dst[i + u * T] = v[u];
  }
}

constexpr int kMaxTaps = 32;  // conv filter taps held in registers (larger filters read LDS)

// Kernels of one translation unit whose granted limit raise_lds_limit remembers. A kernel beyond
// them gets no slot and asks the runtime again at every launch above 64 KiB, which a capture must
// not do: a file's kernel table static_asserts its size against this.
constexpr int kLdsLimitSlots = 8;

// Raise a kernel's dynamic-LDS limit to `bytes` once per (kernel, device); false if refused.
bool raise_lds_limit(const void* kernel, int bytes) {
  static const void* keys[kLdsLimitSlots] = {nullptr};
  static int granted[kLdsLimitSlots][64] = {{0}};  // per kernel slot and device: the limit granted so far
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  int slot = -1;
  for (int i = 0; i < kLdsLimitSlots && dev >= 0; ++i) {
    const void* k = __atomic_load_n(&keys[i], __ATOMIC_ACQUIRE);
    if (k == kernel) { slot = i; break; }
    if (!k) {
      const void* expected = nullptr;
      if (__atomic_compare_exchange_n(&keys[i], &expected, kernel, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE) ||
          expected == kernel) {
        slot = i;
        break;
      }
    }
  }
  if (slot >= 0 && __atomic_load_n(&granted[slot][dev], __ATOMIC_RELAXED) >= bytes) return true;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (slot >= 0) __atomic_store_n(&granted[slot][dev], bytes, __ATOMIC_RELAXED);
  return true;
}

}  // namespace
