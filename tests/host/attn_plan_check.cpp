// attn_plan_check.cpp -- the launch rules of csrc/attn_plan.h on their own: a stand-alone host program (no HIP, no device), built
// with -fsanitize=address,undefined by tests/test_attn_plan.py.  Exit status 0 when every check holds.  Every expected value is a
// literal worked out by hand from the expressions the entry points of attention.hip spelled out before the header existed:
//   items = ceil(S / 128) B H;  grid = min(items, k ((cus - reserve_cus) & ~7, at least 8)), k blocks per CU;
//   perxcd = attn_xcd && (B H) % 8 == 0 && grid % 8 == 0.
#include "../../dalle-mtf_amd/csrc/attn_plan.h"
#include <stdio.h>

static int g_failed = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      printf("FAILED %s: ", #cond);          \
      printf(__VA_ARGS__);                   \
      printf("\n");                          \
      ++g_failed;                            \
    }                                        \
  } while (0)

constexpr int CUS = 256;

static void check_launch(const char* what, AttnOp op, int B, int H, int S, int hd, const AttnOptions& o, const GemmOptions& g, int grid,
                         int perxcd, int lds) {
  const AttnLaunch l = attn_launch(op, B, H, S, hd, o, g, CUS);
  CHECK(l.grid == grid && l.perxcd == perxcd && l.lds == lds, "%s: grid %d (%d) perxcd %d (%d) lds %d (%d)", what, l.grid, grid, l.perxcd,
        perxcd, l.lds, lds);
}

static void check_geometry() {
  const AttnOptions o;
  const GemmOptions g;
  CHECK(o.attn_fwd == 1 && o.attn_bwd == 1 && o.attn_xcd == 8 && o.attn_mask_force == 0, "option defaults");
  // the headline shape: 10 tiles x 128 (batch, head) pairs; two blocks per CU for forward / dQ, one for dK/dV
  CHECK(attn_items(32, 4, 1280) == 1280, "headline items %d", attn_items(32, 4, 1280));
  check_launch("headline fwd", AttnOp::FWD, 32, 4, 1280, 128, o, g, 512, 1, 65536);
  check_launch("headline dQ", AttnOp::DQ, 32, 4, 1280, 128, o, g, 512, 1, 65536);
  check_launch("headline dK/dV", AttnOp::DKV, 32, 4, 1280, 128, o, g, 256, 1, 99328);
  GemmOptions reserve;
  reserve.reserve_cus = 16;   // 240 CUs left
  check_launch("reserve fwd", AttnOp::FWD, 32, 4, 1280, 128, o, reserve, 480, 1, 65536);
  check_launch("reserve dQ", AttnOp::DQ, 32, 4, 1280, 128, o, reserve, 480, 1, 65536);
  check_launch("reserve dK/dV", AttnOp::DKV, 32, 4, 1280, 128, o, reserve, 240, 1, 99328);
  reserve.reserve_cus = 13;   // (256 - 13) & ~7 = 240 as well
  check_launch("reserve 13", AttnOp::DKV, 32, 4, 1280, 128, o, reserve, 240, 1, 99328);
  reserve.reserve_cus = 255;  // never fewer than 8 CUs
  check_launch("reserve 255", AttnOp::FWD, 32, 4, 1280, 128, o, reserve, 16, 1, 65536);
  AttnOptions plain;
  plain.attn_xcd = 0;
  check_launch("attn_xcd 0 fwd", AttnOp::FWD, 32, 4, 1280, 128, plain, g, 512, 0, 65536);
  check_launch("attn_xcd 0 dK/dV", AttnOp::DKV, 32, 4, 1280, 128, plain, g, 256, 0, 99328);
  // fewer items than blocks: one block per item
  check_launch("(1, 1, 128) fwd", AttnOp::FWD, 1, 1, 128, 128, o, g, 1, 0, 65536);
  check_launch("(1, 1, 128) dK/dV", AttnOp::DKV, 1, 1, 128, 128, o, g, 1, 0, 99328);
  check_launch("(1, 1, 136) dQ", AttnOp::DQ, 1, 1, 136, 128, o, g, 2, 0, 65536);        // a ragged second tile
  // B H = 12 does not divide by 8: 10 x 12 = 120 items, one serpentine
  check_launch("B H 12 fwd", AttnOp::FWD, 3, 4, 1280, 128, o, g, 120, 0, 65536);
  check_launch("B H 12 dK/dV", AttnOp::DKV, 3, 4, 1280, 128, o, g, 120, 0, 99328);
  check_launch("B H 16, 16 items", AttnOp::DKV, 2, 8, 8, 128, o, g, 16, 1, 99328);
  // head dim 64: three, three and two blocks per CU; 32768 B of stages, 18432 B of epilogue strips (> two 8448-B stages)
  CHECK(attn_blocks_per_cu(AttnOp::FWD, 64) == 3 && attn_blocks_per_cu(AttnOp::DQ, 64) == 3 && attn_blocks_per_cu(AttnOp::DKV, 64) == 2,
        "head dim 64 blocks per CU");
  CHECK(attn_blocks_per_cu(AttnOp::FWD, 128) == 2 && attn_blocks_per_cu(AttnOp::DQ, 128) == 2 && attn_blocks_per_cu(AttnOp::DKV, 128) == 1,
        "head dim 128 blocks per CU");
  check_launch("hd 64 (2, 8, 256) fwd", AttnOp::FWD, 2, 8, 256, 64, o, g, 32, 1, 32768);
  check_launch("hd 64 (2, 8, 256) dQ", AttnOp::DQ, 2, 8, 256, 64, o, g, 32, 1, 32768);
  check_launch("hd 64 (2, 8, 256) dK/dV", AttnOp::DKV, 2, 8, 256, 64, o, g, 32, 1, 18432);
  check_launch("hd 64 (32, 8, 1280) fwd", AttnOp::FWD, 32, 8, 1280, 64, o, g, 768, 1, 32768);   // 2560 items
  check_launch("hd 64 (32, 8, 1280) dQ", AttnOp::DQ, 32, 8, 1280, 64, o, g, 768, 1, 32768);
  check_launch("hd 64 (32, 8, 1280) dK/dV", AttnOp::DKV, 32, 8, 1280, 64, o, g, 512, 1, 18432);
  reserve.reserve_cus = 16;
  check_launch("hd 64 reserve dK/dV", AttnOp::DKV, 32, 8, 1280, 64, o, reserve, 480, 1, 18432);
}

static void check_shapes() {
  CHECK(attn_head_dim_ok(64) && attn_head_dim_ok(128) && !attn_head_dim_ok(0) && !attn_head_dim_ok(96) && !attn_head_dim_ok(256), "head dims");
  CHECK(attn_shape_ok(1, 1, 8) && attn_shape_ok(32, 4, 1280), "accepted shapes");
  CHECK(!attn_shape_ok(0, 4, 1280) && !attn_shape_ok(32, 0, 1280) && !attn_shape_ok(32, 4, 0) && !attn_shape_ok(32, 4, -8) &&
            !attn_shape_ok(32, 4, 1284) && !attn_shape_ok(-1, 4, 1280),
        "refused shapes");
  CHECK(attn_sizes_ok(1, 1, 5) && !attn_sizes_ok(1, 1, 0) && !attn_sizes_ok(0, 1, 5) && !attn_sizes_ok(1, 0, 5), "decode sizes (any S > 0)");
  // the 32-bit rules at H = 16: the largest accepted multiple of 8 and the next one
  //   head dim 128: S 3 H 128 2 = 12288 S < 2^31 - 1:  174760 -> 2147450880, 174768 -> 2147549184
  CHECK(attn_offsets_fit(16, 174760, 128) && !attn_offsets_fit(16, 174768, 128), "head dim 128 offsets");
  //   head dim 64: (S + 64) 3 H 64 2 = 6144 (S + 64):  349456 -> 2147450880, 349464 -> 2147500032
  CHECK(attn_offsets_fit(16, 349456, 64) && !attn_offsets_fit(16, 349464, 64), "head dim 64 offsets");
  CHECK(!attn_offsets_fit(16, 349464, 128), "the head-dim-128 rule is the tighter one in S");
  //   kv8 decode: S 2 H head_dim: 4096 S at 128 (524280 -> 2147450880, 524288 -> 2^31), 2048 S at 64
  CHECK(kv8_offsets_fit(16, 524280, 128) && !kv8_offsets_fit(16, 524288, 128), "kv8 offsets, head dim 128");
  CHECK(kv8_offsets_fit(16, 1048568, 64) && !kv8_offsets_fit(16, 1048576, 64), "kv8 offsets, head dim 64");
}

static void check_route() {
  const AttnOptions o;
  AttnOptions force;
  force.attn_mask_force = 1;
  int32_t causal[AMP_HDR] = {0x504d4144, 256, 2, 8, 1}, custom[AMP_HDR] = {0x504d4144, 256, 2, 8, 0}, junk[AMP_HDR] = {0x12345678, 256, 2, 8, 0};
  const int dev = 0;   // stands for the device copy: only tested for null
  CHECK(AMP_S == 1 && AMP_CAUSAL == 4 && AMP_COLBITS == 12 && AMP_CAUSAL_K == 17, "header word numbers");
  CHECK(attn_route(nullptr, custom, 256, 128, o) == AttnRoute::NULL_PLAN && attn_route(&dev, nullptr, 256, 128, o) == AttnRoute::NULL_PLAN, "null plan");
  CHECK(attn_route(&dev, junk, 256, 128, o) == AttnRoute::NOT_A_PLAN, "wrong magic");
  CHECK(attn_route(&dev, custom, 264, 128, o) == AttnRoute::WRONG_S && attn_route(&dev, causal, 264, 128, o) == AttnRoute::WRONG_S, "S mismatch");
  CHECK(attn_route(&dev, causal, 256, 128, o) == AttnRoute::CAUSAL && attn_route(&dev, causal, 256, 64, o) == AttnRoute::CAUSAL, "causal plan");
  CHECK(attn_route(&dev, causal, 256, 128, force) == AttnRoute::MASKED, "causal plan, attn_mask_force");
  CHECK(attn_route(&dev, causal, 256, 64, force) == AttnRoute::HEAD_DIM, "causal plan, attn_mask_force, head dim 64");
  CHECK(attn_route(&dev, custom, 256, 128, o) == AttnRoute::MASKED && attn_route(&dev, custom, 256, 128, force) == AttnRoute::MASKED, "custom plan");
  CHECK(attn_route(&dev, custom, 256, 64, o) == AttnRoute::HEAD_DIM, "custom plan, head dim 64");
  // the order of the tests: a null plan before the magic, the magic before S, S before the head dim
  CHECK(attn_route(nullptr, junk, 264, 64, o) == AttnRoute::NULL_PLAN && attn_route(&dev, junk, 264, 64, o) == AttnRoute::NOT_A_PLAN &&
            attn_route(&dev, custom, 264, 64, o) == AttnRoute::WRONG_S,
        "order of the route's tests");
}

static void check_kernel_choice() {
  AttnOptions o;
  for (int fwd = 0; fwd <= 1; ++fwd)
    for (int bwd = 0; bwd <= 1; ++bwd) {
      o.attn_fwd = fwd; o.attn_bwd = bwd;
      CHECK(attn_fwd_pipelined(false, o) == (fwd == 1), "attn_fwd %d", fwd);
      CHECK(!attn_fwd_pipelined(true, o), "a mask plan runs the round-2 form (attn_fwd %d)", fwd);
      CHECK(attn_bwd_rowstore(false, o) == bwd, "attn_bwd %d", bwd);
      CHECK(attn_bwd_rowstore(true, o) == 1, "the masked backward has the whole-row epilogue only (attn_bwd %d)", bwd);
    }
  o.attn_bwd = 2;
  CHECK(attn_bwd_rowstore(false, o) == 0, "attn_bwd 2: bit 0 decides");
}

int main() {
  check_geometry();
  check_shapes();
  check_route();
  check_kernel_choice();
  if (g_failed) {
    printf("attn_plan_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  printf("attn_plan_check: ok\n");
  return 0;
}
