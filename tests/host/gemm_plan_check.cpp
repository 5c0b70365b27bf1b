// gemm_plan_check.cpp -- the dispatch plans of csrc/gemm_plan.h on their own: a stand-alone host program (no HIP, no device),
// built with -fsanitize=address,undefined by tests/test_gemm_plan.py.  Exit status 0 when every check holds.
//   1. the step's products land on the kernels they are measured on (256 CUs, default options), and every option removes /
//      forces its arm;
//   2. soundness of the weight-gradient workspace: whatever tn_plan / tn_group_plan writes lies inside tn_workspace_bytes(M, I, J),
//      which is all a caller allocates -- the kernels' memory safety rests on it.
#include "../../dalle-mtf_amd/csrc/gemm_plan.h"
#include <initializer_list>
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
// the traits gemm.hip builds from an epilogue's FLAGS:     skinny ntr   regs  nt4   softmax
constexpr NtTraits PLAIN = {true, true, true, true, false};      // 0, bias, bias + ReLU, bias + residual
constexpr NtTraits ROWSCALE = {false, true, true, true, false};  // row scale, ReLU mask, residual alone
constexpr NtTraits SOFTMAX = {false, false, true, true, true};   // the vocabulary projection
constexpr NtTraits GELU = {true, false, true, true, false};      // the GELU epilogues: not in the full-row kernel
constexpr NtTraits OUT_F32 = {false, false, false, false, false};    // split-K slabs
static const NtTraits ALL_TRAITS[] = {PLAIN, ROWSCALE, SOFTMAX, GELU, OUT_F32};

static NtPlan plan(const NtTraits& t, int M, int N, int K, const GemmOptions& o = GemmOptions()) { return nt_plan(t, M, N, K, K, K, K, 1, o, CUS); }

static const int MS[] = {64, 2560, 40960, 163840};
static const int WIDTHS[] = {128, 256, 384, 512, 768, 1024, 1536, 2048, 50816, 58368};

static void check_step_products() {
  NtPlan p = plan(PLAIN, 40960, 1536, 512);                       // QKV
  CHECK(p.kernel == NtKernel::NT8P && p.grid_x == 256 && p.tiles_m == 160 && p.tiles_n == 6 && p.lds == 131072, "QKV");
  p = plan(SOFTMAX, 40960, 50816, 512);                           // vocabulary projection
  CHECK(p.kernel == NtKernel::NT8P, "vocabulary projection");
  p = plan(PLAIN, 40960, 512, 512);                               // out-projection
  CHECK(p.kernel == NtKernel::NTR && p.grid_x == 256 && p.block == 512 && p.pf == 2, "out-projection: %d blocks", p.grid_x);
  p = plan(PLAIN, 40960, 512, 2048);                              // FFN-2
  CHECK(p.kernel == NtKernel::NTR && p.grid_x == 256, "FFN-2: %d blocks", p.grid_x);
  p = plan(ROWSCALE, 32768, 512, 50816);                          // head input gradient, its whole-residency rows
  CHECK(p.kernel == NtKernel::NT8 && p.grid_x * p.grid_y == 256, "head input gradient: %d blocks", p.grid_x * p.grid_y);
  CHECK(plan(ROWSCALE, 40960, 512, 50816).kernel != NtKernel::NT8, "head input gradient at M 40960");
  p = plan(PLAIN, 4, 384, 128);                                   // decode
  CHECK(p.kernel == NtKernel::SKINNY && p.grid_x == 384 / 16, "decode: %d blocks", p.grid_x);
  CHECK(plan(PLAIN, 40960, 2048, 192).kernel == NtKernel::NT4, "M 40960 N 2048 K 192");
  p = plan(PLAIN, 256, 256, 64);
  CHECK(p.kernel == NtKernel::NT2 && p.grid_x == 4 && p.lds == 65536, "M 256 N 256 K 64");
  CHECK(plan(GELU, 40960, 512, 512).kernel != NtKernel::NTR && plan(SOFTMAX, 40960, 512, 512).kernel != NtKernel::NTR, "no full-row GELU / softmax");
  CHECK(plan(OUT_F32, 40960, 1536, 512).kernel == NtKernel::NT2, "fp32 output keeps the 128x128 kernel");
}

static void check_options() {
  GemmOptions reserve, off, force;
  reserve.reserve_cus = 16;
  off.nt4 = off.nt8 = off.nt8p = off.ntr = off.skinny = 0;
  for (const NtTraits& t : ALL_TRAITS)
    for (int M : {4, 64, 2560, 32768, 40960, 163840})
      for (int N : WIDTHS)
        for (int K : WIDTHS) {
          CHECK(plan(t, M, N, K, reserve).kernel != NtKernel::NTR, "reserve_cus 16 ran full-row tiles (M=%d N=%d K=%d)", M, N, K);
          CHECK(plan(t, M, N, K, off).kernel == NtKernel::NT2, "all arms off (M=%d N=%d K=%d)", M, N, K);
          const NtPlan d = plan(t, M, N, K);     // whatever kernel the defaults choose: its own option at 0 removes it
          GemmOptions o;
          o.nt4 = d.kernel == NtKernel::NT4 ? 0 : 1; o.nt8 = d.kernel == NtKernel::NT8 ? 0 : 1; o.nt8p = d.kernel == NtKernel::NT8P ? 0 : 1;
          o.ntr = d.kernel == NtKernel::NTR ? 0 : 1; o.skinny = d.kernel == NtKernel::SKINNY ? 0 : 1;
          CHECK(d.kernel == NtKernel::NT2 || plan(t, M, N, K, o).kernel != d.kernel, "option 0 kept its arm (M=%d N=%d K=%d)", M, N, K);
        }
  // 2 forces an arm where the shape allows it (shapes the automatic rules leave on other kernels)
  force = GemmOptions(); force.ntr = 2;
  CHECK(plan(PLAIN, 320, 512, 64, force).kernel == NtKernel::NTR && plan(PLAIN, 320, 512, 64).kernel != NtKernel::NTR, "ntr = 2");
  CHECK(plan(PLAIN, 320, 384, 64, force).kernel != NtKernel::NTR && plan(GELU, 320, 512, 64, force).kernel != NtKernel::NTR, "ntr = 2 needs N = 512 and the epilogue");
  force = GemmOptions(); force.nt8p = 2;
  CHECK(plan(PLAIN, 256, 256, 128, force).kernel == NtKernel::NT8P && plan(PLAIN, 256, 256, 128).kernel != NtKernel::NT8P, "nt8p = 2");
  CHECK(plan(PLAIN, 256, 256, 64, force).kernel != NtKernel::NT8P && plan(OUT_F32, 256, 256, 128, force).kernel != NtKernel::NT8P, "nt8p = 2 needs K %% 128 == 0 and bf16 output");
  force = GemmOptions(); force.nt8p = 3;
  CHECK(plan(SOFTMAX, 40960, 50816, 512, force).kernel == NtKernel::NT8P && plan(PLAIN, 40960, 1536, 512, force).kernel != NtKernel::NT8P, "nt8p = 3: the head only");
  force = GemmOptions(); force.nt8 = 2;
  CHECK(plan(PLAIN, 256, 256, 64, force).kernel == NtKernel::NT8 && plan(OUT_F32, 256, 256, 64, force).kernel == NtKernel::NT8, "nt8 = 2");
  force = GemmOptions(); force.nt4 = 2;
  CHECK(plan(PLAIN, 256, 256, 64, force).kernel == NtKernel::NT4 && plan(OUT_F32, 256, 256, 64, force).kernel == NtKernel::NT2, "nt4 = 2");
  force.nt4_lds = 98304;
  CHECK(plan(PLAIN, 256, 256, 64, force).lds == 98304, "nt4_lds");
}

// a plan's own numbers agree with each other and stay inside the workspace every caller allocates
static void check_tn(int M, int I, int J, const GemmOptions& o) {
  const TnPlan p = tn_plan(M, I, J, o, CUS);
  const int64_t ws = tn_workspace_bytes(M, I, J);
  CHECK(p.ws_used <= ws, "tn_plan writes %lld of %lld workspace bytes (M=%d I=%d J=%d tn8=%d tn_wide=%d tn_tail=%d kernel %d)", (long long)p.ws_used,
        (long long)ws, M, I, J, o.tn8, o.tn_wide, o.tn_tail, (int)p.kernel);
  CHECK(p.nsplit >= 1 && (int64_t)p.m_per_split * p.nsplit >= M && p.m_per_split % TN_STEP == 0, "row splits do not cover M=%d (I=%d J=%d)", M, I, J);
  if (p.kernel == TnKernel::TAIL)
    CHECK(p.nsplit == 1 && p.W > 0 && p.c0 + p.W == J && p.c0 % TN_TILE == 0 && (int64_t)p.mps * p.S >= M && p.tail_tiles * p.S <= TN_SLOTS,
          "tail geometry (M=%d I=%d J=%d)", M, I, J);
  if (p.kernel == TnKernel::WIDE_SK) CHECK(p.nsplit == 1 && p.gangs % 8 == 0 && p.gangs * p.tiles_i <= 2 * CUS && p.ws_used == 0, "gangs (M=%d I=%d J=%d)", M, I, J);
}
static void check_group(const int* I, const int* J, int n, int M, const GemmOptions& o) {
  const TnGroupPlan g = tn_group_plan(I, J, n, M, o);
  CHECK(g.S >= 1 && (int64_t)g.m_per_split * g.S >= M && g.first_tile[n] == g.T && (!g.wide || g.S >= 2), "group plan (n=%d M=%d)", n, M);
  for (int k = 0; k < n; ++k) {
    const int64_t used = g.S > 1 ? tn_layout(g.S, I[k], J[k]).slab_bytes + (int64_t)g.S * J[k] * 4 : 0, ws = tn_workspace_bytes(M, I[k], J[k]);
    CHECK(used <= ws, "tn_group_plan writes %lld of %lld workspace bytes (problem %d of %d: M=%d I=%d J=%d, S=%d wide=%d)", (long long)used, (long long)ws,
          k, n, M, I[k], J[k], g.S, (int)g.wide);
  }
}
static void check_workspace_soundness() {
  for (int tn8 = 0; tn8 <= 2; ++tn8)
    for (int wide = 0; wide <= 1; ++wide)
      for (int tail = 0; tail <= 1; ++tail)
        for (int reserve : {0, 16}) {
          GemmOptions o;
          o.tn8 = tn8; o.tn_wide = wide; o.tn_tail = tail; o.reserve_cus = reserve;
          for (int M : MS) {
            for (int I : WIDTHS)
              for (int J : WIDTHS)
                if (tn8 < 2 || (I >= 256 && J >= 256)) check_tn(M, I, J, o);    // the 256x256 kernel is forced only where it can be chosen
            for (int d : {128, 256, 512, 1024, 2048}) {     // a block's FFN-1, FFN-2, out-projection, QKV gradients
              const int I[4] = {4 * d, d, d, d}, J[4] = {d, 4 * d, d, 3 * d};
              check_group(I, J, 4, M, o); check_group(I, J, 2, M, o); check_group(I + 2, J + 2, 2, M, o); check_group(I, J, 1, M, o);
            }
          }
        }
  const TnPlan head = tn_plan(40960, 512, 50816, GemmOptions(), CUS);     // the head's gradient: the gang stream-K
  CHECK(head.kernel == TnKernel::WIDE_SK && head.gangs == 128 && head.grid == 512, "head gradient: kernel %d, %d gangs", (int)head.kernel, head.gangs);
  const TnPlan qkv = tn_plan(40960, 512, 1536, GemmOptions(), CUS);
  CHECK(qkv.kernel == TnKernel::TN && qkv.nsplit == 10 && qkv.grid == 480, "QKV gradient: %d splits", qkv.nsplit);
  CHECK(tn_workspace_bytes(40960, 512, 50816) == 312823552 && tn_workspace_bytes(40960, 2048, 512) == 67141888, "workspace bytes");
}

static void check_option_table() {
  GemmOptions o;
  int flag = 0;
  const OptionSlot table[] = {{"nt4_lds", &o.nt4_lds, 49152, 163840}, {"reserve_cus", &o.reserve_cus, 0, INT32_MAX}, {"nt8p", &o.nt8p}, {"flag", &flag, INT32_MIN, INT32_MAX, true}};
  CHECK(option_get(table, "nt4_lds") == 49152 && option_get(table, "nope") == -1 && option_set(table, "nope", 1) == -1, "lookup");
  CHECK(option_set(table, "nt4_lds", 1) == -1 && option_set(table, "nt4_lds", 163841) == -1 && o.nt4_lds == 49152, "nt4_lds range");
  CHECK(option_set(table, "nt4_lds", 65536) == 0 && o.nt4_lds == 65536, "nt4_lds set");
  CHECK(option_set(table, "reserve_cus", -1) == -1 && option_set(table, "reserve_cus", 16) == 0 && o.reserve_cus == 16, "reserve_cus");
  CHECK(option_set(table, "nt8p", -5) == 0 && o.nt8p == -5, "unranged option");
  CHECK(option_set(table, "flag", 7) == 0 && flag == 1 && option_set(table, "flag", 0) == 0 && flag == 0, "flag normalised");
}

int main() {
  check_step_products();
  check_options();
  check_workspace_soundness();
  check_option_table();
  // the queries of the public ABI (the values of the commit before this header existed)
  CHECK(relu_bits_auto(40960, 2048, 512, GemmOptions(), CUS) && nt_ln_auto(40960, 512, 2048, GemmOptions()), "queries");
  CHECK(!nt_ln_auto(163840, 512, 50816, GemmOptions()) && !nt_ln_auto(4194304, 512, 512, GemmOptions()) && !nt_ln_auto(40960, 384, 512, GemmOptions()), "ln_auto limits");
  printf(g_failed ? "%d checks FAILED\n" : "gemm_plan_check: ok\n", g_failed);
  return g_failed ? 1 : 0;
}
