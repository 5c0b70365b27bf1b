// attn_plan.h -- what an attention entry point accepts, which kernel it runs, on what grid and with how much LDS: the one place a
// launch rule of attention.hip lives.  Host-only plain C++17 with nothing from HIP, so a CPU compiler builds it alone (tests/host/
// attn_plan_check.cpp).  Every function is pure: the options and the CU count are arguments.
#pragma once
#include "gemm_plan.h"   // GemmOptions::reserve_cus, persistent_blocks

// ------------------------------------------------------------------ options (dmi_get_option / dmi_set_option)
struct AttnOptions {
  int attn_fwd = 1;          // forward kernel: 0 the round-2 program-order form, 1 the software-pipelined round-6 kernel (A/B switch)
  int attn_bwd = 1;          // backward kernels: bit 0 = whole-row epilogue stores through LDS (A/B switch)
  int attn_xcd = 8;          // block order: 0 one serpentine over the whole grid, otherwise per-XCD ranges where the shape divides by 8
  int attn_mask_force = 0;   // 1: a causal mask plan runs the masked kernels too (tests, tools/attn_mask_bench.py)
};

// ------------------------------------------------------------------ shapes
inline bool attn_head_dim_ok(int head_dim) { return head_dim == 64 || head_dim == 128; }
inline bool attn_sizes_ok(int B, int H, int S) { return B > 0 && H > 0 && S > 0; }
// the tiled kernels (forward, dQ, dK/dV) take S % 8 == 0
inline bool attn_shape_ok(int B, int H, int S) { return attn_sizes_ok(B, H, S) && S % 8 == 0; }
// 32-bit limits.  The tiled kernels address a (batch, head)'s rows of the [S, 3 H head_dim] bf16 projection through buffer descriptors
// with 32-bit byte offsets; the head-dim-64 kernels' tiles may start at the last row and reach 64 rows past it.
inline bool attn_offsets_fit(int H, int S, int head_dim) {
  return head_dim == 64 ? ((int64_t)S + 64) * 3 * H * 64 * 2 < 0x7fffffff : (int64_t)S * 3 * H * 128 * 2 < 0x7fffffff;
}
// The FP8 decode's row offset inside a batch element's [S, 2, H, head_dim] byte cache.
inline bool kv8_offsets_fit(int H, int S, int head_dim) { return (int64_t)S * 2 * H * head_dim < 0x7fffffff; }

// ------------------------------------------------------------------ mask plans: the header words and the route
// (the sections these words point to: "attention-mask plans" in attention.hip)
#define AMP_MAGIC 0x504d4144
#define AMP_HDR 32
enum {
  AMP_S = 1, AMP_NB, AMP_W, AMP_CAUSAL, AMP_FPTR, AMP_FLIST, AMP_KPTR, AMP_KLIST, AMP_FORDER, AMP_KORDER, AMP_ROWBITS, AMP_COLBITS,
  AMP_WORDS, AMP_LIVE_F, AMP_CAUSAL_F, AMP_LIVE_K, AMP_CAUSAL_K
};
// The host copy of the plan (its header) decides the route of a *_masked entry: a causal plan runs the causal entry points (so the
// default kernels, at either head dim) unless attn_mask_force is set; the masked kernels are built for head dim 128.  Tested in
// this order; everything from NULL_PLAN on is an error.
enum class AttnRoute { MASKED, CAUSAL, NULL_PLAN, NOT_A_PLAN, WRONG_S, HEAD_DIM };
inline AttnRoute attn_route(const void* plan, const int32_t* plan_host, int S, int head_dim, const AttnOptions& o) {
  if (!plan || !plan_host) return AttnRoute::NULL_PLAN;
  if (plan_host[0] != AMP_MAGIC) return AttnRoute::NOT_A_PLAN;
  if (plan_host[AMP_S] != S) return AttnRoute::WRONG_S;
  if (plan_host[AMP_CAUSAL] && !o.attn_mask_force) return AttnRoute::CAUSAL;
  return head_dim == 128 ? AttnRoute::MASKED : AttnRoute::HEAD_DIM;
}

// ------------------------------------------------------------------ launch geometry of the persistent kernels
enum class AttnOp { FWD, DQ, DKV };
// work items of every operation: (128-position tile, batch * head) -- query blocks for FWD / DQ, key blocks for DKV
inline int attn_items(int B, int H, int S) { return ((S + 127) / 128) * B * H; }
// blocks of 256 threads per CU = waves per SIMD a kernel is built for (its __launch_bounds__)
constexpr int A64_FWD_WAVES = 3, A64_DQ_WAVES = 3, A64_DKV_WAVES = 2;   // head dim 64: 168 registers (at four, 128 registers, both spilled)
inline int attn_blocks_per_cu(AttnOp op, int head_dim) {
  if (head_dim == 64) return op == AttnOp::FWD ? A64_FWD_WAVES : op == AttnOp::DQ ? A64_DQ_WAVES : A64_DKV_WAVES;
  return op == AttnOp::DKV ? 1 : 2;
}
// dynamic LDS.  128: two K | V stages of 32768 (FWD, DQ); the V tile + four Q | dO | stats stages of 16640 (DKV).  64: two stages of
// 16384; the larger of the four waves' epilogue strips (32 rows x 144 B) and two stages of 8448.
constexpr int ATTN_QK_LDS = 2 * 32768, ATTN_DKV_LDS = 32768 + 4 * 16640, A64_QK_LDS = 2 * 16384, A64_DKV_LDS = 4 * 32 * 144;
inline int attn_lds_bytes(AttnOp op, int head_dim) {
  if (head_dim == 64) return op == AttnOp::DKV ? A64_DKV_LDS : A64_QK_LDS;
  return op == AttnOp::DKV ? ATTN_DKV_LDS : ATTN_QK_LDS;
}
struct AttnLaunch {
  int grid;     // persistent blocks: blocks_per_cu per CU left to these kernels, at most one per item
  int perxcd;   // the kernels' schedule argument: each XCD deals its own eighth of the (batch, head) pairs (attn_sched)
  int lds;
};
inline AttnLaunch attn_launch(AttnOp op, int B, int H, int S, int head_dim, const AttnOptions& o, const GemmOptions& g, int cus) {
  const int items = attn_items(B, H, S), cap = attn_blocks_per_cu(op, head_dim) * persistent_blocks(g, cus);
  const int grid = items < cap ? items : cap;
  return {grid, o.attn_xcd && (B * H) % 8 == 0 && grid % 8 == 0, attn_lds_bytes(op, head_dim)};
}

// ------------------------------------------------------------------ which head-dim-128 kernel (head dim 64 has one per operation)
// forward: a mask plan runs the round-2 form's masked instance; otherwise option attn_fwd picks the form
inline bool attn_fwd_pipelined(bool masked, const AttnOptions& o) { return !masked && o.attn_fwd != 0; }
// backward, the `rowstore` template argument of both kernels: the masked instances exist with the whole-row epilogue only
inline int attn_bwd_rowstore(bool masked, const AttnOptions& o) { return masked ? 1 : (o.attn_bwd & 1); }
