// gemm_plan.h -- which kernel runs a GEMM, on what grid, with how many splits and how much workspace: the one place a dispatch
// rule of gemm.hip lives.  Host-only plain C++17 with nothing from HIP, so a CPU compiler builds it alone (tests/host/
// gemm_plan_check.cpp).  Every function is pure: the options and the CU count are arguments.
#pragma once
#include <stdint.h>
#include <string.h>

// ------------------------------------------------------------------ options (dmi_get_option / dmi_set_option)
struct GemmOptions {
  int nt4 = 1;        // 256x128 NT tile: 0 never, 1 auto (>= 3 residencies and K <= 1024), 2 always (tests)
  int nt8 = 1;        // 256x256 NT tile (8 waves): 0 never, 1 auto (K >= nt8_min_k, whole residencies), 2 always (tests)
  int nt8_min_k = 2048;   // auto mode of the 256x256 NT tile: minimum K.  2048 (was 4096): the 1.3B dimensions' K = 2048 products
                          // run 354 -> 339 ms/step (profiles/r03_ab_nt8_min_k.log); K = 1024 measured equal, K = 512 slower
  int nt8p = 1;       // persistent 256x256 NT kernel with the register epilogue (gemm_nt8p_kernel): 0 never, 1 auto (short K, >= 2
                      // tiles per CU), 2 whenever the shape allows it (tests, tools/kbench.py), 3 auto for the softmax head only
                      // (tests: its register epilogue adds the row-sum partials in its own fixed order, so a step that is to be
                      // compared bit for bit with the 128x128 kernels keeps the head where it is)
  int nt8p_max_k = 1024;  // auto mode: K above this keeps the one-tile-per-block kernels (the main loop then dominates a tile)
  int ntr = 1;        // full-row 160x512 tiles for N = 512 products (gemm_ntr_kernel): 0 never, 1 auto, 2 whenever the shape allows
  int nt4_lds = 49152;    // dynamic LDS requested by the 256x128 NT kernel: 49152 = what it uses (3 blocks / CU); 65536 / 98304
                          // cap the residency at 2 / 1 blocks per CU (tools/phases.py: a block's phases without co-resident blocks)
  int skinny = 1;     // M <= 32 products (the decode step) on the weight-streaming kernel: 0 never, 1 auto
  int res16 = 1;      // register epilogue: the residual as 16-byte pieces through the row swap (1) or 8-byte pieces in the accumulator layout (0)
  int relu_bits = 1;  // FFN ReLU mask as one bit per element (dmi_gemm_nt_relu_bits / _mask_bits) where the persistent kernel runs: 0 never, 1 auto
  int cstream = 1;    // bf16 outputs stored write-through (sc1; + non-temporal from cstream_nt_min_mb MiB): 0 never, 1 auto (outputs >=
                      // cstream_min_mb MiB: they cannot be re-read from L2 anyway, and as plain stores they evict the operands the concurrent
                      // tiles share), 2 always sc1, 3 always sc1 nt, 4 auto with sc1 only (A/B)
  int cstream_min_mb = 256;
  int cstream_nt_min_mb = 1024;
  int tn8 = 0;        // 256x256 weight-gradient tile (8 waves, still on 32x32x16 MFMAs): 0 never (default since the 128x128 kernel
                      // moved to 16x16x32: 45 / 76 us vs 60 / 86 us on the 512x512 / 512x1536 gradients), 1 auto (few tiles), 2 always (tests)
  int tn8_max_tiles = 16;   // auto mode: use the 256x256 weight-gradient kernel below this many tiles (A/B hook)
  int tn_wide = 1;    // [r06] unsplit weight gradients with many column stripes (the head) as a gang stream-K on 128 x 256 tiles: 0 never, 1 auto
  int tn_tail = 1;    // weight gradients: row-split the tiles of a ragged last residency (see gemm_tn_tail_kernel)
  int reserve_cus = 0;    // CUs the persistent kernels (256x256 NT, attention) leave free, and which switch the one-tile-per-CU
                          // full-row kernel off: a block of those kernels whose CU is held by a concurrent kernel (the RCCL channels
                          // of the gradient exchange) starts late and stretches the whole launch -- measured with the token sort as
                          // the intruder (layer 0's forward 687 us instead of 410 us).  The engine sets 16 when world_size > 1.
};

// one row per option name: where it lives, the values it accepts (outside -> -1), and whether it is normalised to 0 / 1
struct OptionSlot {
  const char* name;
  int* value;
  int lo = INT32_MIN, hi = INT32_MAX;
  bool flag = false;
};
template <int N>
inline int option_get(const OptionSlot (&table)[N], const char* name) {
  for (const OptionSlot& s : table)
    if (!strcmp(s.name, name)) return *s.value;
  return -1;     // unknown name
}
template <int N>
inline int option_set(const OptionSlot (&table)[N], const char* name, int value) {
  for (const OptionSlot& s : table)
    if (!strcmp(s.name, name)) {
      if (value < s.lo || value > s.hi) return -1;
      *s.value = s.flag ? (value ? 1 : 0) : value;
      return 0;
    }
  return -1;
}

// ------------------------------------------------------------------ small arithmetic and the tile geometry of the kernels
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int64_t round_up64(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
constexpr int NT_BK = 64;                       // K step of the 128x128 kernel: every NT entry needs K % 64 == 0
constexpr int NT2_TILE = 128, NT4_TILE_M = 256, NT8_TILE = 256, NTR_ROWS = 160, NTR_N = 512;
constexpr int NTR_LDS = 3 * (NTR_ROWS * 64 + 32768);
constexpr int TN_TILE = 128, TN8_TILE = 256, TNW_TILE_I = 128, TNW_TILE_J = 256, TNW_STEP = 32, TN_STEP = 64;
constexpr int TN_SLOTS = 512;                   // two 256-thread weight-gradient blocks per CU on 256 CUs
constexpr int TN_GROUP_N = 4, TN_GROUP_ORDER = 8;   // problems of a grouped launch; GROUP_M, the tile order's group height

// blocks of a one-per-CU persistent kernel: a multiple of 8 (block id % 8 = XCD), the reserved CUs left free
inline int persistent_blocks(const GemmOptions& o, int cus) {
  const int n = (cus - o.reserve_cus) & ~7;
  return n < 8 ? 8 : n;
}

// ------------------------------------------------------------------ 32-bit limits, each written once
// The kernels address an operand through a buffer descriptor whose size (num_records) and per-lane offsets are 32-bit byte counts.
// Weights Bt[N, ldb] bf16 behind one descriptor: N * ldb * 2 bytes < 2^31.
inline bool b_fits(int64_t N, int64_t ldb) { return N * ldb < (1 << 30); }
// Activations A[M, lda] bf16 behind descriptors sized to the end of the operand (persistent 256x256 kernel): bytes < 2^31.
inline bool a_fits(int64_t M, int64_t lda) { return M * lda < (1 << 30); }
// The same operand in the fused full-row forms, whose descriptors start at the block's first row: M * lda elements < 2^31.
inline bool a_fits_rows(int64_t M, int64_t lda) { return M * lda < ((int64_t)1 << 31); }
// The LayerNorm backward's x / dx [M, N] bf16, row offsets in bytes: M * N * 2 < 2^31.
inline bool c_fits(int64_t M, int64_t N) { return M * N * 2 < ((int64_t)1 << 31); }
// Weight gradients step TN_STEP rows of X [M, ldx] / dY [M, ldy] at a time: one step's byte offset stays below 2^31.
inline bool tn_ld_fits(int ldx, int ldy) { return (int64_t)TN_STEP * (ldx > ldy ? ldx : ldy) * 2 < 0x7fffffff; }
// The write-through / non-temporal store policies are used below 4 GiB of bf16 output only.
inline bool cpol_fits(int64_t cbytes) { return cbytes < (int64_t)0xffffffff; }

// ------------------------------------------------------------------ NT products: C[M, N] = A[M, K] . Bt[N, K]^T
enum class NtKernel { SKINNY, NTR, NT8P, NT8, NT4, NT2 };
struct NtTraits {     // the compile-time facts of an epilogue FLAGS value: which kernels are built for it
  bool skinny;        // the weight-streaming decode kernel has this epilogue
  bool ntr;           // the full-row kernel has it (register epilogue; not the softmax and GELU ones)
  bool regs;          // the register epilogue serves it (bf16 output): the persistent kernel
  bool nt4;           // the 256x128 kernel has it (bf16 output)
  bool softmax;       // the vocabulary projection's softmax-numerator epilogue (option nt8p = 3)
};
struct NtPlan {
  NtKernel kernel;
  int tiles_m, tiles_n;       // as the chosen kernel reads them from its arguments
  int grid_x, grid_y, block, lds;
  int pf;                     // GemmArgs::pf
};

// what the persistent 256x256 kernel needs of a launch, and whether the automatic choice takes it (short K, >= 2 tiles per CU)
inline bool nt8p_can(int M, int N, int K, int lda, int ldb, int k_per_split) {
  return k_per_split == K && K % 128 == 0 && a_fits(M, lda) && b_fits(N, ldb);
}
inline bool nt8p_auto(int M, int N, int K, const GemmOptions& o, int cus) {
  return K <= o.nt8p_max_k && cdiv(M, NT8_TILE) * cdiv(N, NT8_TILE) >= 2 * cus;
}
inline NtPlan nt8p_plan(int M, int N, const GemmOptions& o, int cus) {
  return {NtKernel::NT8P, cdiv(M, NT8_TILE), cdiv(N, NT8_TILE), persistent_blocks(o, cus), 1, 512, 131072, 0};
}
// The four full-row sites check different sets of the limits above.  They are kept exactly as they were; one set is a follow-up.
//   the dispatch's arm (ntr_can)   b_fits only: the A operand passes no range check on this arm
//   dmi_gemm_nt_ln                 b_fits + a_fits_rows            (nt_ln_can)
//   dmi_gemm_nt_lnbwd              b_fits + a_fits_rows + c_fits   (nt_lnbwd_can)
//   dmi_gemm_nt_ln_auto            all three at lda = ldb = K      (nt_ln_auto): stricter than the arm it describes
inline bool ntr_can(int N, int K, int ldb, int k_per_split, int nsplit) {
  return N == NTR_N && nsplit == 1 && k_per_split == K && K % 32 == 0 && b_fits(N, ldb);
}
inline NtPlan ntr_plan(int M, int pf) {
  return {NtKernel::NTR, cdiv(M, NT2_TILE), cdiv(NTR_N, NT2_TILE), cdiv(M, NTR_ROWS), 1, 512, NTR_LDS, pf};
}

inline NtPlan nt_plan(const NtTraits& t, int M, int N, int K, int lda, int ldb, int k_per_split, int nsplit, const GemmOptions& o, int cus) {
  const int tm = cdiv(M, NT2_TILE), tn = cdiv(N, NT2_TILE), t8m = cdiv(M, NT8_TILE), t8n = cdiv(N, NT8_TILE);
  if (t.skinny && o.skinny && M <= 32 && nsplit == 1 && N % 16 == 0) return {NtKernel::SKINNY, tm, tn, N / 16, 1, 512, 0, 0};
  // full-row tiles, one 160-row tile per block: at least half a residency, and not the head's input gradient (K = 50816: 1.83 ms
  // here vs 1.32 ms on 256x256 tiles)
  if (t.ntr && o.ntr && ntr_can(N, K, ldb, k_per_split, nsplit) && (o.ntr == 2 || (M >= NTR_ROWS * (cus / 2) && K <= 4096 && o.reserve_cus == 0)))
    return ntr_plan(M, o.res16 ? 2 : 0);     // residual rows as 16-byte pieces (A/B switch)
  if (t.regs && nsplit == 1 && nt8p_can(M, N, K, lda, ldb, k_per_split)) {
    const bool auto_ok = nt8p_auto(M, N, K, o, cus);
    if ((o.nt8p == 1 && auto_ok) || o.nt8p == 2 || (o.nt8p == 3 && t.softmax && auto_ok)) return nt8p_plan(M, N, o, cus);
  }
  // 256x256 tiles (one 8-wave block per CU): main-loop-bound shapes only -- long K and whole residencies of 256 blocks
  if ((o.nt8 == 1 && k_per_split >= o.nt8_min_k && (t8m * t8n * nsplit) % 256 == 0) || o.nt8 == 2)
    return {NtKernel::NT8, t8m, t8n, t8m * t8n, nsplit, 512, 131072, 0};
  // 256x128 tiles when the grid still covers >= 3 residencies; long-K shapes prefer the BK = 64 kernel
  const int tiles4 = cdiv(M, NT4_TILE_M) * tn;
  if (t.nt4 && o.nt4 && nsplit == 1 && k_per_split == K && ((tiles4 >= 1536 && K <= 1024) || o.nt4 == 2))
    return {NtKernel::NT4, cdiv(M, NT4_TILE_M), tn, tiles4, 1, 256, o.nt4_lds, 0};
  return {NtKernel::NT2, tm, tn, tm * tn, nsplit, 256, 65536, 0};
}

// cache policy of the bf16 output stores (GemmArgs::cpol): 0 plain, 1 sc1, 2 sc1 nt.  Option cstream 1 (default): auto by size --
// sc1 from cstream_min_mb, sc1 nt from cstream_nt_min_mb (a stream far larger than the 256-MB Infinity Cache: the 4-GB softmax
// numerators; outputs of a few hundred MB that the next kernel re-reads were measured with sc1 only and keep it); 2: always sc1;
// 3: always sc1 nt; 4: auto by size, sc1 only (A/B).  The fp32 forms do not use the policy.
inline int nt_cpol(int M, int N, int ldc, const GemmOptions& o) {
  const int64_t cbytes = ((int64_t)(M - 1) * ldc + N) * 2;
  const bool big = cbytes >= ((int64_t)o.cstream_min_mb << 20), huge = cbytes >= ((int64_t)o.cstream_nt_min_mb << 20);
  const int pol = (o.cstream == 1 && big) ? (huge ? 2 : 1) : (o.cstream == 2) ? 1 : (o.cstream == 3) ? 2 : (o.cstream == 4 && big) ? 1 : 0;
  return cpol_fits(cbytes) ? pol : 0;
}

// the queries behind dmi_relu_bits_auto, the bit entries' own check, and dmi_gemm_nt_ln_auto
inline bool relu_bits_auto(int M, int N, int K, const GemmOptions& o, int cus) {
  return o.relu_bits && o.nt8p == 1 && N % 64 == 0 && K % 128 == 0 && nt8p_auto(M, N, K, o, cus);
}
inline bool relu_bits_can(int M, int N, int K, int lda, int ldb) { return N % 64 == 0 && nt8p_can(M, N, K, lda, ldb, K); }
inline bool nt_ln_can(int M, int N, int lda, int ldb) { return N == NTR_N && b_fits(N, ldb) && a_fits_rows(M, lda); }
inline bool nt_lnbwd_can(int M, int N, int lda, int ldb) { return nt_ln_can(M, N, lda, ldb) && c_fits(M, N); }
inline bool nt_ln_auto(int M, int N, int K, const GemmOptions& o) {
  return M > 0 && K > 0 && K % NT_BK == 0 && nt_lnbwd_can(M, N, K, K) && o.reserve_cus == 0;
}

// ------------------------------------------------------------------ TN products (weight gradients): dW[I, J] = X[M, I]^T . dY[M, J]
enum class TnKernel { TN, TN8, WIDE_SK, TAIL };

// Row splits that fill the TN_SLOTS block slots with `tiles` tiles: whole multiples of the residency (a 1.5x grid leaves a
// quarter of the chip idle in the tail), at least 4 steps per block; fewer splits also means fewer fp32 slabs to write and reduce.
inline int tn_fill_splits(int tiles, int M) {
  const int max_s = cdiv(M, 4 * TN_STEP);
  int s = tiles >= 384 ? 1 : TN_SLOTS / tiles;
  if (s > max_s) s = max_s;
  return s < 1 ? 1 : s;
}
inline int tn_splits(int M, int I, int J) { return tn_fill_splits(cdiv(I, TN_TILE) * cdiv(J, TN_TILE), M); }
// 256x256-tile weight-gradient kernel (8 waves, one block per CU): used when both dimensions fill 256-wide tiles
// (measured in the dalle_example step, profiles/r02c_*: it wins where the 128x128 plan needs many row splits -- 512x512: 64 -> 57 us,
// 512x1536: 88 -> 79 us incl. the slab reduce -- and ties or loses from 16 tiles up, where its 64-row steps give the LDS-DMA
// no more cover than the two co-resident blocks of the 128x128 kernel have)
inline bool tn8_eligible(int M, int I, int J, const GemmOptions& o) {
  if (o.tn8 == 2) return true;
  return o.tn8 == 1 && I >= 256 && J >= 256 && M >= 2048 && cdiv(I, TN8_TILE) * cdiv(J, TN8_TILE) < o.tn8_max_tiles;
}
inline int tn8_splits(int M, int I, int J) {
  const int tiles = cdiv(I, TN8_TILE) * cdiv(J, TN8_TILE);
  const int max_s = cdiv(M, 8 * TN_STEP);   // at least 8 k-steps per block
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= 64 && s <= max_s; ++s) {
    // makespan in units of one unsplit block: rounds of 256 resident blocks, each 1/s long, + the fp32 slab round trip
    // (write + read of s x I x J x 4 bytes at ~4 TB/s vs the block's 2 x 256 x 256 x M flops at ~4.5 TFLOP/s per CU)
    const double rounds = (double)(((int64_t)tiles * s + 255) / 256) / s;
    const double slab = (s > 1) ? (double)s * I * J * 8.0 / 4.0e12 / (2.0 * 256 * 256 * (double)M / 4.5e12) : 0.0;
    if (rounds + slab < best_cost - 1e-9) { best_cost = rounds + slab; best = s; }
  }
  return best;
}

// The workspace of a split gradient: `nsplit` fp32 slabs [I, J], then [nsplit][J] bias partials, each rounded to 256 bytes.
struct TnLayout {
  int64_t slab_bytes;   // = the byte offset of the bias partials
  int64_t bytes;        // what a workspace for this split count holds (+ 256 spare)
};
inline TnLayout tn_layout(int nsplit, int I, int J) {
  const int64_t slabs = nsplit > 1 ? round_up64((int64_t)nsplit * I * J * 4, 256) : 0;
  return {slabs, slabs + round_up64((int64_t)nsplit * J * 4, 256) + 256};
}
// What dmi_gemm_tn_workspace_bytes answers, whatever the options say at launch time: the larger of the 128x128 plan's layout,
// the 256x256 plan's (shapes that kernel can be chosen for: I, J >= 256), and the tail slabs of an unsplit shape with a ragged
// last residency (< 512 tiles x 64 KiB, + bias rows).  Every plan below writes inside it (tests/host/gemm_plan_check.cpp).
inline int64_t tn_workspace_bytes(int M, int I, int J) {
  int64_t base = tn_layout(tn_splits(M, I, J), I, J).bytes;
  if (I >= 256 && J >= 256) {
    const int64_t b8 = tn_layout(tn8_splits(M, I, J), I, J).bytes;
    if (b8 > base) base = b8;
  }
  const int64_t tiles = (int64_t)cdiv(I, TN_TILE) * cdiv(J, TN_TILE);
  const int64_t tail = (tn_splits(M, I, J) == 1 && tiles > TN_SLOTS) ? (TN_SLOTS * 65536 + TN_SLOTS * 128 * 4 * (int64_t)cdiv(I, TN_TILE)) : 0;
  return base > tail + 256 ? base : tail + 256;
}

struct TnPlan {
  TnKernel kernel;
  int nsplit, tiles_i, tiles_j, m_per_split;
  TnLayout layout;
  int grid, block;
  int n_whole, tail_tiles, S, c0, W, mps;   // TAIL: whole-residency tiles; the stripe [c0, c0 + W) of dW in S row splits of mps rows
  int gangs, nsteps;                        // WIDE_SK
  int64_t ws_used;                          // bytes of the workspace the launch writes (with a bias gradient)
};
inline TnPlan tn_plan(int M, int I, int J, const GemmOptions& o, int cus) {
  TnPlan p{};
  const bool use8 = tn8_eligible(M, I, J, o);
  const int tile = use8 ? TN8_TILE : TN_TILE;
  p.kernel = use8 ? TnKernel::TN8 : TnKernel::TN;
  p.nsplit = use8 ? tn8_splits(M, I, J) : tn_splits(M, I, J);
  p.tiles_i = cdiv(I, tile); p.tiles_j = cdiv(J, tile);
  p.m_per_split = (int)round_up64(cdiv(M, p.nsplit), TN_STEP);
  p.layout = tn_layout(p.nsplit, I, J);
  const int tiles = p.tiles_i * p.tiles_j;
  p.grid = tiles * p.nsplit; p.block = use8 ? 512 : 256;
  p.ws_used = p.nsplit > 1 ? p.layout.slab_bytes + (int64_t)p.nsplit * J * 4 : 0;
  if (use8 || p.nsplit != 1) return p;
  if (o.tn_wide) {   // [r06] gang stream-K on the 128 x 256 tile (gemm_tn_wide_sk_kernel): unsplit gradients with many stripes
    const int wti = cdiv(I, TNW_TILE_I), wtj = cdiv(J, TNW_TILE_J), nsteps = cdiv(M, TNW_STEP);
    const int gangs = (2 * persistent_blocks(o, cus) / wti) & ~7;   // two blocks per CU, the reserved CUs left free; whole gangs per XCD
    if (gangs >= 8 && wtj >= gangs && (int64_t)(wtj + 1) * nsteps < 0x7fffffff) {   // (the kernel counts (stripe, step) units in 32 bits)
      p.kernel = TnKernel::WIDE_SK; p.tiles_i = wti; p.tiles_j = wtj; p.gangs = gangs; p.nsteps = nsteps; p.grid = gangs * wti;
      return p;
    }
  }
  // tiles are numbered ti-fastest: with tiles_i | n_whole the tail is the column stripe [c0, J) of dW
  p.tail_tiles = tiles % TN_SLOTS; p.n_whole = tiles - p.tail_tiles;
  p.S = p.tail_tiles ? TN_SLOTS / p.tail_tiles : 1;
  if (o.tn_tail && tiles > TN_SLOTS && p.S >= 2 && p.tiles_i <= TN_GROUP_ORDER && p.n_whole % p.tiles_i == 0 && J % 4 == 0) {
    p.kernel = TnKernel::TAIL;
    p.c0 = (p.n_whole / p.tiles_i) * TN_TILE; p.W = J - p.c0;
    p.mps = (int)round_up64(cdiv(M, p.S), TN_STEP);
    p.grid = p.n_whole + p.tail_tiles * p.S;
    p.ws_used = ((int64_t)p.S * I * p.W + (int64_t)p.S * p.W) * 4;   // [S][I][W] slabs, then [S][W] bias partials
  }
  return p;
}

// Weight gradients that share M in one launch.  The group splits the union of its tiles as a single gradient would split its
// own, so never finer than the single launch: every problem's own workspace (tn_workspace_bytes(M, I, J)) has the slabs.  On
// 128 x 256 tiles (`wide`) where the union of those tiles fills (>= 448 of) the block slots with a split count >= 2 that every
// problem's workspace has slabs for.
struct TnGroupPlan {
  bool wide;
  int S, T, m_per_split;
  int first_tile[TN_GROUP_N + 1], tiles_i[TN_GROUP_N], tiles_j[TN_GROUP_N];
};
inline TnGroupPlan tn_group_plan(const int* I, const int* J, int n, int M, const GemmOptions& o) {
  TnGroupPlan g{};
  int Tw = 0, smin = 1 << 30;
  for (int k = 0; k < n; ++k) {
    g.T += cdiv(I[k], TN_TILE) * cdiv(J[k], TN_TILE);
    Tw += cdiv(I[k], TNW_TILE_I) * cdiv(J[k], TNW_TILE_J);
    const int sk = tn_splits(M, I[k], J[k]);
    if (sk < smin) smin = sk;
  }
  g.S = tn_fill_splits(g.T, M);
  const int Sw = o.tn_wide ? tn_fill_splits(Tw, M) : 0;
  if (Sw >= 2 && Sw <= smin && Tw * Sw >= 448) { g.wide = true; g.S = Sw; g.T = Tw; }
  g.m_per_split = (int)round_up64(cdiv(M, g.S), TN_STEP);
  int T = 0;
  for (int k = 0; k <= TN_GROUP_N; ++k) {
    g.first_tile[k] = T;
    if (k < n) {
      g.tiles_i[k] = cdiv(I[k], TN_TILE); g.tiles_j[k] = cdiv(J[k], g.wide ? TNW_TILE_J : TN_TILE);
      T += g.tiles_i[k] * g.tiles_j[k];
    }
  }
  return g;
}
