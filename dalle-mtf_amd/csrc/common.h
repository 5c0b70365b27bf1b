// common.h -- shared device helpers for libdalle_hip (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/dalle_hip.h"

typedef uint16_t bf16_t;  // raw bfloat16 bits

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define WAVE 64

// s_setprio(1) around an MFMA cluster (cdna_hip_programming.md T5): with several blocks per CU in different phases the
// scheduler then prefers the wave that is feeding the matrix pipe over co-resident waves issuing DMA / LDS traffic.
// Measured in the dalle_example step (profiles/r03_ab_setprio_groupm.log, same-call A/B): NT GEMMs 16.84 -> 16.74 ms/step
// (the BK = 64 kernel +3 % on the K >= 1536 shapes, the 256x128 kernel neutral); the same around the attention kernels'
// S / PV clusters: neutral to -0.5 % (not applied).
#define MFMA_PRIO(x) __builtin_amdgcn_s_setprio(x)

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;  // RNE (v_cvt_pk_bf16_f32 on gfx950)
  return __builtin_bit_cast(unsigned short, b);
}
typedef float pk_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 pk_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
  const pk_f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, pk_bf16x2));  // one v_cvt_pk_bf16_f32 (RNE)
}
__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(v[i] << 16);
    f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = pack2bf(f[2 * i], f[2 * i + 1]);
  return v;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}

// ------------------------------------------------------------------ stateless dropout mask (DESIGN.md §4 "Dropout")
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// One dropout site: element e of the site's tensor (row-major) is kept iff ((splitmix64(key + (e >> 2)) >> 16 (e & 3)) & 0xffff)
// >= thresh, kept elements are multiplied by scale = fp32(65536 / (65536 - thresh)), dropped ones are +0.  One hash serves
// four elements; nothing is stored: forward, its re-run under recompute_grad and backward restate the mask from the key.
struct DropSite {
  uint64_t key;
  unsigned thresh;
  float scale;
};
static inline DropSite drop_site(uint64_t key, int thresh) { return DropSite{key, (unsigned)thresh, (float)(65536.0 / (65536 - thresh))}; }
// f[0..8) = the eight elements starting at element index e0 (a multiple of 8); the product is rounded on its own (never fused into
// a following add), so a numpy float32 restatement gives the same bits
__host__ __device__ __forceinline__ void drop8(float* f, const DropSite& s, int64_t e0) {
#pragma clang fp contract(off)
  const uint64_t g = (uint64_t)e0 >> 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t r = splitmix64(s.key + g + h);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = f[4 * h + j] * s.scale;
      f[4 * h + j] = ((unsigned)(r >> (16 * j)) & 0xffffu) >= s.thresh ? t : 0.f;
    }
  }
}
__host__ __device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// ------------------------------------------------------------------ host-side error plumbing
void dmi_set_error(const char* fmt, ...);
#define DMI_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      dmi_set_error(__VA_ARGS__);         \
      return DMI_ERR_INVALID;             \
    }                                     \
  } while (0)
#define DMI_CHECK_LAUNCH(name)                                              \
  do {                                                                      \
    hipError_t e__ = hipGetLastError();                                     \
    if (e__ != hipSuccess) {                                                \
      dmi_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return DMI_ERR_LAUNCH;                                                \
    }                                                                       \
  } while (0)

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// One-time host setup, safe from any host thread: a function-local static is initialised once, under the compiler's guard.
// raise_lds_once<kernel>(bytes): lift the kernel's dynamic LDS limit before its first launch (the same bytes at every call site).
template <auto KERNEL>
static inline void raise_lds_once(int bytes) {
  static const hipError_t once = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)once;
}
// CUs of the current device as the launch plans count them (gemm_plan.h, attn_plan.h): 256, the MI355X's count, where no device
// answers or one reports fewer than 8
static inline int num_cus() {
  static const int n = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    return prop.multiProcessorCount >= 8 ? prop.multiProcessorCount : 256;
  }();
  return n;
}