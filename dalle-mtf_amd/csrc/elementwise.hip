// elementwise.hip -- HBM-bound kernels of the DALL-E train step (SURVEY.md §2.2 K1,K2,K7-K10).
// All loads/stores are 16 B per lane (8 bf16 / 4 fp32), one wave64 per row where rows are short,
// wave-shuffle reductions, deterministic two-stage reductions for gradients of shared parameters.
#include "common.h"
#include <stdarg.h>

// ------------------------------------------------------------------ error plumbing
static thread_local char g_err[512] = "ok";
void dmi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* dmi_last_error_string(void) { return g_err; }
extern "C" int dmi_version(void) { return 100; }

// =====================================================================================
// K1 embedding   (src/dalle_mtf/models.py:186-219)
// =====================================================================================
// DROP (dmi_embed_fwd_dropout, training forwards): x = bf16(drop_tok(wte[tok]) + drop_pos(wpe[s])); the token mask is indexed by
// (b S + s) d + c, the positional mask by s d + c -- shared over the batch, as the reference's pos_emb is [seq, embd] when
// mtf.dropout sees it (src/dalle_mtf/models.py:215-217)
template <bool DROP>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int* __restrict__ tokens,
                                                        const bf16_t* __restrict__ wte,
                                                        const bf16_t* __restrict__ wpe, bf16_t* __restrict__ x,
                                                        int64_t rows, int S, int d, int vocab, const int* __restrict__ pos_dev,
                                                        DropSite dtok, DropSite dpos) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  int tok = tokens[row];
  tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
  int s = (int)(row % S);
  if (pos_dev) {                                        // the decode step: every row sits at that one position (clamped to the table)
    s = *pos_dev;
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);
  }
  const u32x4* a = (const u32x4*)(wte + (int64_t)tok * d);
  const u32x4* p = (const u32x4*)(wpe + (int64_t)s * d);
  u32x4* o = (u32x4*)(x + row * d);
  for (int c = lane; c < d / 8; c += 64) {
    float fa[8], fp[8];
    unpack8(a[c], fa);
    unpack8(p[c], fp);
    if constexpr (DROP) {
      drop8(fa, dtok, row * d + c * 8);
      drop8(fp, dpos, (int64_t)s * d + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) fa[j] = add_rn(fa[j], fp[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) fa[j] += fp[j];
    }
    o[c] = pack8(fa);
  }
}

extern "C" int dmi_embed_fwd(const int32_t* tokens, const uint16_t* wte, const uint16_t* wpe, uint16_t* x,
                             int64_t rows, int S, int d, int vocab, const int* pos_dev, void* stream) {
  DMI_REQUIRE(tokens && wte && wpe && x, "embed_fwd: null pointer");
  DMI_REQUIRE(d % 8 == 0 && rows > 0 && S > 0, "embed_fwd: d %% 8 != 0 or empty (d=%d rows=%lld)", d, (long long)rows);
  embed_fwd_kernel<false><<<dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, (hipStream_t)stream>>>(tokens, wte, wpe, x, rows, S, d, vocab, pos_dev,
                                                                                                 DropSite{}, DropSite{});
  DMI_CHECK_LAUNCH("embed_fwd");
  return DMI_OK;
}

#define DMI_REQUIRE_THRESH(name, thresh) \
  DMI_REQUIRE((thresh) >= 0 && (thresh) <= 65535, name ": thresh must lie in [0, 65535] (thresh=%d)", (int)(thresh))

extern "C" int dmi_embed_fwd_dropout(const int32_t* tokens, const uint16_t* wte, const uint16_t* wpe, uint16_t* x, int64_t rows, int S,
                                     int d, int vocab, uint64_t key_tok, uint64_t key_pos, int thresh, void* stream) {
  DMI_REQUIRE(tokens && wte && wpe && x, "embed_fwd_dropout: null pointer");
  DMI_REQUIRE(d % 8 == 0 && rows > 0 && S > 0, "embed_fwd_dropout: d %% 8 != 0 or empty (d=%d rows=%lld)", d, (long long)rows);
  DMI_REQUIRE_THRESH("embed_fwd_dropout", thresh);
  embed_fwd_kernel<true><<<dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, (hipStream_t)stream>>>(
      tokens, wte, wpe, x, rows, S, d, vocab, nullptr, drop_site(key_tok, thresh), drop_site(key_pos, thresh));
  DMI_CHECK_LAUNCH("embed_fwd_dropout");
  return DMI_OK;
}

// dwpe[s, :] = sum_b dx[b, s, :]      (one wave per position; deterministic)
// DROP: ... times the positional mask of row s (the same for every b), applied to the finished sum
template <bool DROP>
__global__ __launch_bounds__(256) void embed_bwd_wpe_kernel(const bf16_t* __restrict__ dx, float* __restrict__ dwpe,
                                                            int B, int S, int d, DropSite dpos) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int s = blockIdx.x * 4 + wid;
  if (s >= S) return;
  for (int c = lane; c < d / 8; c += 64) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      float f[8];
      unpack8(*(const u32x4*)(dx + ((int64_t)b * S + s) * d + c * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
    if constexpr (DROP) drop8(acc, dpos, (int64_t)s * d + c * 8);
    float* o = dwpe + (int64_t)s * d + c * 8;
    *(f32x4*)o = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}
// ---- stable sort of the token ids (index plumbing for the scatter-add below) -----------------------------------------
// LSD radix sort with 4-bit digits over SORT_T = 2048 threads (8 blocks): thread g owns the contiguous chunk
// [g*cpt, (g+1)*cpt) of the current order.  Per pass three short launches: COUNT (every thread counts its digits into its own
// column of hist[16][SORT_T], no atomics), SCAN (one block: exclusive scan of the 16 * SORT_T counts in (digit, thread) order =
// the destinations), SCATTER (every thread writes its chunk in order) -> stable and deterministic.  ceil(log2(vocab) / 4)
// passes ping-pong between (sorted, perm) and the workspace; the last pass lands in the outputs.
// [r04] Rounds 2-3 ran this as ONE 1024-thread block for 0.62 ms on a side stream "hidden" under the forward.  It was not
// hidden: the forward's kernels are persistent (one or two blocks per CU, each with its own tile list), and the block whose CU
// the sort occupied started ~0.6 ms late -- a per-launch trace showed layer 0's forward taking 687 us instead of 410 us
// (attention 210 us instead of 70).  Moving it under the head's weight gradient moved the damage there (+340 us).  As 12
// launches of 3-5 us it disturbs nothing.
#define SORT_T 2048
#define SORT_BLK 256
__device__ __forceinline__ int sort_clamp(int k, int vocab) { return k < 0 ? 0 : (k >= vocab ? vocab - 1 : k); }
__global__ __launch_bounds__(SORT_BLK) void sort_count_kernel(const int* __restrict__ keys, int* __restrict__ hist, int n, int vocab,
                                                              int shift, int cpt) {
  __shared__ int col[16][SORT_BLK];
  const int t = threadIdx.x, g = blockIdx.x * SORT_BLK + t;
#pragma unroll
  for (int d = 0; d < 16; ++d) col[d][t] = 0;
  const int i0 = (int64_t)g * cpt < n ? g * cpt : n;
  const int i1 = i0 + cpt < n ? i0 + cpt : n;
  for (int i = i0; i < i1; ++i) col[(sort_clamp(keys[i], vocab) >> shift) & 15][t] += 1;
#pragma unroll
  for (int d = 0; d < 16; ++d) hist[d * SORT_T + g] = col[d][t];
}
// exclusive scan of hist[16 * SORT_T] in linear (digit-major) order, in place; thread t owns 16 * SORT_T / 1024 = 32 entries
__global__ __launch_bounds__(1024) void sort_scan_kernel(int* __restrict__ hist) {
  __shared__ int wtot[16];
  constexpr int PER = 16 * SORT_T / 1024;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  int* h = hist + t * PER;
  int tot = 0;
  for (int j = 0; j < PER; j += 4) {
    const int4 v = *(const int4*)(h + j);
    tot += (v.x + v.y) + (v.z + v.w);
  }
  int inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wtot[wid] = inc;
  __syncthreads();
  int base = inc - tot;
  for (int w = 0; w < wid; ++w) base += wtot[w];
  for (int j = 0; j < PER; j += 4) {
    int4 v = *(const int4*)(h + j);
    const int4 o = {base, base + v.x, base + v.x + v.y, base + v.x + v.y + v.z};
    base += (v.x + v.y) + (v.z + v.w);
    *(int4*)(h + j) = o;
  }
}
__global__ __launch_bounds__(SORT_BLK) void sort_scatter_kernel(const int* __restrict__ keys, const int* __restrict__ perm_in,
                                                                int* __restrict__ keys_out, int* __restrict__ perm_out,
                                                                const int* __restrict__ hist, int n, int vocab, int shift, int cpt) {
  __shared__ int col[16][SORT_BLK];
  const int t = threadIdx.x, g = blockIdx.x * SORT_BLK + t;
#pragma unroll
  for (int d = 0; d < 16; ++d) col[d][t] = hist[d * SORT_T + g];
  const int i0 = (int64_t)g * cpt < n ? g * cpt : n;
  const int i1 = i0 + cpt < n ? i0 + cpt : n;
  for (int i = i0; i < i1; ++i) {
    const int k = sort_clamp(keys[i], vocab);
    const int d = (k >> shift) & 15;
    const int pos = col[d][t];
    col[d][t] = pos + 1;
    keys_out[pos] = k;
    perm_out[pos] = perm_in ? perm_in[i] : i;
  }
}
extern "C" int64_t dmi_sort_tokens_workspace_bytes(int64_t n) { return 2 * n * 4 + (int64_t)16 * SORT_T * 4 + 256; }
extern "C" int dmi_sort_tokens(const int32_t* tokens, int32_t* sorted_tokens, int32_t* perm, int64_t n, int vocab,
                               void* workspace, void* stream) {
  DMI_REQUIRE(tokens && sorted_tokens && perm && workspace, "sort_tokens: null pointer");
  DMI_REQUIRE(n > 0 && n < (1ll << 30) && vocab > 0, "sort_tokens: bad sizes");
  int bits = 1;
  while ((1ll << bits) < vocab) ++bits;
  const int npass = (bits + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  int* tk = (int*)workspace;           // [n] keys | [n] perm | [16 * SORT_T] counts
  int* tp = tk + n;
  int* hist = (int*)(((uintptr_t)(tp + n) + 15) & ~(uintptr_t)15);      // 16-B aligned (vector loads in the scan)
  const int cpt = (int)((n + SORT_T - 1) / SORT_T);
  const dim3 grid(SORT_T / SORT_BLK), blk(SORT_BLK);
  for (int p = 0; p < npass; ++p) {
    const bool to_out = ((npass - 1 - p) & 1) == 0;          // the last pass lands in the outputs
    const int* sk = (p == 0) ? tokens : (to_out ? tk : sorted_tokens);
    const int* sp = (p == 0) ? nullptr : (to_out ? tp : perm);
    int* dk = to_out ? sorted_tokens : tk;
    int* dp = to_out ? perm : tp;
    sort_count_kernel<<<grid, blk, 0, st>>>(sk, hist, (int)n, vocab, 4 * p, cpt);
    sort_scan_kernel<<<dim3(1), dim3(1024), 0, st>>>(hist);
    sort_scatter_kernel<<<grid, blk, 0, st>>>(sk, sp, dk, dp, hist, (int)n, vocab, 4 * p, cpt);
  }
  DMI_CHECK_LAUNCH("sort_tokens");
  return DMI_OK;
}

// ---- scatter-add = gradient of mtf.gather (Appendix A.6), deterministic, no atomics -------------------------------
// Positions are visited in token-id order (sorted_tok ascending, perm = source row).  One wave per chunk of 32 sorted
// positions accumulates each run of equal ids in registers.  A run that lies entirely inside its chunk is stored
// directly (single writer).  The chunk's first / last run may continue in the neighbouring chunks (the padding id fills
// hundreds of chunks): those partial sums go to part[chunk][0 / 1][d], and a second kernel lets the wave of the chunk
// where such a run STARTS add the partials of the following chunks in chunk order.  dwte is zeroed here (ids absent
// from the batch have zero gradient).
#define EB_CH 32
__device__ __forceinline__ int eb_clamp(int t, int vocab) { return t < 0 ? 0 : (t >= vocab ? vocab - 1 : t); }
// DROP: every dx row is masked and scaled with the token mask of its own position (perm[i]) before it is added
template <bool DROP>
__global__ __launch_bounds__(256) void embed_bwd_wte_sorted_kernel(const int* __restrict__ sorted_tok,
                                                                   const int* __restrict__ perm,
                                                                   const bf16_t* __restrict__ dx,
                                                                   float* __restrict__ dwte, float* __restrict__ part,
                                                                   int64_t n, int d, int vocab, DropSite dtok) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + wid;
  const int64_t i0 = chunk * EB_CH;
  if (i0 >= n) return;
  const int64_t i1 = (i0 + EB_CH < n) ? i0 + EB_CH : n;
  const int first_tok = sorted_tok[i0];
  const bool head_open = (i0 > 0) && (sorted_tok[i0 - 1] == first_tok);
  for (int c = lane; c < d / 8; c += 64) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int cur = first_tok;
    bool open = head_open;   // the run being accumulated started before this chunk
    bool first = true;       // ... and is the chunk's first run
    for (int64_t i = i0; i < i1; ++i) {
      const int t = sorted_tok[i];
      if (t != cur) {   // run [.., i) ended inside the chunk
        float* dst = open ? part + ((int64_t)chunk * 2 + 0) * d + c * 8 : dwte + (int64_t)eb_clamp(cur, vocab) * d + c * 8;
        *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *(f32x4*)(dst + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        cur = t;
        open = false;
        first = false;
      }
      float f[8];
      const int64_t e0 = (int64_t)perm[i] * d + c * 8;
      unpack8(*(const u32x4*)(dx + e0), f);
      if constexpr (DROP) drop8(f, dtok, e0);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
    const bool tail_open = (i1 < n) && (sorted_tok[i1] == cur);
    float* dst;
    if (open || tail_open) dst = part + ((int64_t)chunk * 2 + (first ? 0 : 1)) * d + c * 8;
    else dst = dwte + (int64_t)eb_clamp(cur, vocab) * d + c * 8;
    *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(dst + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}
// the chunk's LAST run, if it continues into the next chunk and did not start before this chunk, owns the row: add the
// slot-0 partials of the following chunks while they continue the same id (fixed order -> deterministic)
__global__ __launch_bounds__(256) void embed_bwd_wte_combine_kernel(const int* __restrict__ sorted_tok, float* __restrict__ dwte,
                                                                    const float* __restrict__ part, int64_t n, int d, int vocab) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + wid;
  const int64_t i0 = chunk * EB_CH;
  if (i0 >= n) return;
  const int64_t i1 = (i0 + EB_CH < n) ? i0 + EB_CH : n;
  if (i1 >= n) return;                                  // last chunk: nothing continues
  const int tok = sorted_tok[i1 - 1];
  if (sorted_tok[i1] != tok) return;                    // last run is closed at the tail
  const bool single = sorted_tok[i0] == tok;            // the whole chunk is one run
  if (single && i0 > 0 && sorted_tok[i0 - 1] == tok) return;   // a continuation, not a start
  const int slot = single ? 0 : 1;
  const int64_t nchunks = (n + EB_CH - 1) / EB_CH;
  // number of following chunks that continue the run: chunk k continues iff it starts with tok; it is the last one iff
  // the run ends inside it.  64 chunks are classified per ballot (the padding id spans hundreds of chunks; a serial walk
  // with two dependent loads per chunk cost 110 us on the dalle_example batch).
  int64_t cnt = 0;
  for (int64_t base = chunk + 1; base < nchunks; base += 64) {
    const int64_t k = base + lane;
    bool cont = false, last = true;
    if (k < nchunks) {
      const int64_t k0 = k * EB_CH, k1 = (k0 + EB_CH < n) ? k0 + EB_CH : n;
      cont = sorted_tok[k0] == tok;
      last = !(sorted_tok[k1 - 1] == tok && k1 < n && sorted_tok[k1] == tok);
    }
    const unsigned long long stop = __ballot(!cont || last);   // first chunk that is not a full continuation
    if (stop == 0ull) { cnt += 64; continue; }
    const int f = __ffsll((long long)stop) - 1;
    const unsigned long long contb = __ballot(cont);
    cnt += f + (((contb >> f) & 1ull) ? 1 : 0);                   // chunk f still contributes if it starts with tok
    break;
  }
  const float* p0 = part + ((int64_t)chunk * 2 + slot) * d;
  const float* pk = part + ((int64_t)(chunk + 1) * 2) * d;   // slot 0 of the following chunks, stride 2 d
  for (int c = lane; c < d / 4; c += 64) {
    f32x4 acc = *(const f32x4*)(p0 + c * 4);
    int64_t k = 0;
    for (; k + 4 <= cnt; k += 4) {   // four independent loads in flight, summed in chunk order
      const f32x4 v0 = *(const f32x4*)(pk + (k + 0) * 2 * d + c * 4);
      const f32x4 v1 = *(const f32x4*)(pk + (k + 1) * 2 * d + c * 4);
      const f32x4 v2 = *(const f32x4*)(pk + (k + 2) * 2 * d + c * 4);
      const f32x4 v3 = *(const f32x4*)(pk + (k + 3) * 2 * d + c * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = (((acc[j] + v0[j]) + v1[j]) + v2[j]) + v3[j];
    }
    for (; k < cnt; ++k) {
      const f32x4 v = *(const f32x4*)(pk + k * 2 * d + c * 4);
      acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
    }
    *(f32x4*)(dwte + (int64_t)eb_clamp(tok, vocab) * d + c * 4) = acc;
  }
}

extern "C" int64_t dmi_embed_bwd_workspace_bytes(int B, int S, int d) {
  return (((int64_t)B * S + EB_CH - 1) / EB_CH) * 2 * d * 4 + 256;
}
template <bool DROP>
static int embed_bwd_launch(const int32_t* sorted_tokens, const int32_t* perm, const uint16_t* dx, float* dwte, float* dwpe, int B, int S,
                            int d, int vocab, void* workspace, DropSite dtok, DropSite dpos, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  embed_bwd_wpe_kernel<DROP><<<dim3((S + 3) / 4), dim3(256), 0, st>>>(dx, dwpe, B, S, d, dpos);
  DMI_CHECK_LAUNCH("embed_bwd_wpe");
  DMI_REQUIRE(hipMemsetAsync(dwte, 0, (size_t)vocab * d * 4, st) == hipSuccess, "embed_bwd: memset failed");
  const int64_t n = (int64_t)B * S;
  const int64_t chunks = cdiv64(n, EB_CH);
  embed_bwd_wte_sorted_kernel<DROP><<<dim3((unsigned)cdiv64(chunks, 4)), dim3(256), 0, st>>>(sorted_tokens, perm, dx, dwte, (float*)workspace, n,
                                                                                         d, vocab, dtok);
  DMI_CHECK_LAUNCH("embed_bwd_wte_sorted");
  embed_bwd_wte_combine_kernel<<<dim3((unsigned)cdiv64(chunks, 4)), dim3(256), 0, st>>>(sorted_tokens, dwte, (const float*)workspace, n, d, vocab);
  DMI_CHECK_LAUNCH("embed_bwd_wte_combine");
  return DMI_OK;
}
extern "C" int dmi_embed_bwd(const int32_t* sorted_tokens, const int32_t* perm, const uint16_t* dx, float* dwte,
                             float* dwpe, int B, int S, int d, int vocab, void* workspace, void* stream) {
  DMI_REQUIRE(sorted_tokens && perm && dx && dwte && dwpe && workspace, "embed_bwd: null pointer");
  DMI_REQUIRE(d % 8 == 0 && B > 0 && S > 0 && vocab > 0, "embed_bwd: bad sizes");
  return embed_bwd_launch<false>(sorted_tokens, perm, dx, dwte, dwpe, B, S, d, vocab, workspace, DropSite{}, DropSite{}, stream);
}
extern "C" int dmi_embed_bwd_dropout(const int32_t* sorted_tokens, const int32_t* perm, const uint16_t* dx, float* dwte, float* dwpe,
                                     int B, int S, int d, int vocab, void* workspace, uint64_t key_tok, uint64_t key_pos, int thresh,
                                     void* stream) {
  DMI_REQUIRE(sorted_tokens && perm && dx && dwte && dwpe && workspace, "embed_bwd_dropout: null pointer");
  DMI_REQUIRE(d % 8 == 0 && B > 0 && S > 0 && vocab > 0, "embed_bwd_dropout: bad sizes (d %% 8 != 0 or empty: d=%d B=%d S=%d)", d, B, S);
  DMI_REQUIRE_THRESH("embed_bwd_dropout", thresh);
  return embed_bwd_launch<true>(sorted_tokens, perm, dx, dwte, dwpe, B, S, d, vocab, workspace, drop_site(key_tok, thresh),
                                drop_site(key_pos, thresh), stream);
}

// =====================================================================================
// K2 LayerNorm (src/dalle_mtf/models.py:373-389, layers.py:30-33): biased variance of the
// centred row, eps inside rsqrt.  One wave per row, row cached in registers (d <= 512*NC).
// =====================================================================================
// the LayerNorm of one row held in registers (lane owns chunks lane + 64 i; sum = the lane's partial row sum): shared by
// ln_fwd_kernel and dropout_add_ln_kernel, so both compute the same bits from the same row
template <int NC>
__device__ __forceinline__ void ln_row(float (&v)[NC][8], float sum, const bf16_t* __restrict__ g, const bf16_t* __restrict__ b,
                                       bf16_t* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int64_t row, int d,
                                       float eps, int lane) {
  const int nch = d / 8;
  const float mu = wave_sum(sum) / (float)d;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[i][j] -= mu;
        sq += v[i][j] * v[i][j];
      }
    }
  }
  const float rs = rsqrtf(wave_sum(sq) / (float)d + eps);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      float fg[8], fb[8], o[8];
      unpack8(*(const u32x4*)(g + c * 8), fg);
      unpack8(*(const u32x4*)(b + c * 8), fb);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = v[i][j] * rs * fg[j] + fb[j];
      *(u32x4*)(y + row * d + c * 8) = pack8(o);
    }
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

template <int NC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ g,
                                                     const bf16_t* __restrict__ b, bf16_t* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     int64_t rows, int d, float eps) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  const int nch = d / 8;
  float v[NC][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      unpack8(*(const u32x4*)(x + row * d + c * 8), v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  ln_row<NC>(v, sum, g, b, y, mean, rstd, row, d, eps, lane);
}

extern "C" int dmi_layernorm_fwd(const uint16_t* x, const uint16_t* g, const uint16_t* b, uint16_t* y, float* mean,
                                 float* rstd, int64_t rows, int d, float eps, void* stream) {
  DMI_REQUIRE(x && g && b && y && mean && rstd, "layernorm_fwd: null pointer");
  DMI_REQUIRE(d % 8 == 0 && d <= 4096 && rows > 0, "layernorm_fwd: unsupported d=%d (need d%%8==0, d<=4096)", d);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)cdiv64(rows, 4)), blk(256);
  if (d <= 512) ln_fwd_kernel<1><<<grid, blk, 0, st>>>(x, g, b, y, mean, rstd, rows, d, eps);
  else if (d <= 1024) ln_fwd_kernel<2><<<grid, blk, 0, st>>>(x, g, b, y, mean, rstd, rows, d, eps);
  else if (d <= 2048) ln_fwd_kernel<4><<<grid, blk, 0, st>>>(x, g, b, y, mean, rstd, rows, d, eps);
  else ln_fwd_kernel<8><<<grid, blk, 0, st>>>(x, g, b, y, mean, rstd, rows, d, eps);
  DMI_CHECK_LAUNCH("layernorm_fwd");
  return DMI_OK;
}

// ---- residual dropout (src/dalle_mtf/models.py:312-314, 322-323): x_out = bf16(residual + drop(a)), then the LayerNorm that
// follows it from the ROUNDED row, which never leaves the registers -- one pass, 8 bytes of HBM traffic per element where the
// bias-only product + dropout + add + LayerNorm as separate kernels would move 16.  g == NULL: x_out only.
template <int NC>
__global__ __launch_bounds__(256) void dropout_add_ln_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ res,
                                                             bf16_t* __restrict__ x, const bf16_t* __restrict__ g,
                                                             const bf16_t* __restrict__ b, bf16_t* __restrict__ y,
                                                             float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, int d,
                                                             float eps, DropSite site) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  const int nch = d / 8;
  float v[NC][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const int64_t e0 = row * d + c * 8;
      float fr[8];
      unpack8(*(const u32x4*)(a + e0), v[i]);
      unpack8(*(const u32x4*)(res + e0), fr);
      drop8(v[i], site, e0);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = add_rn(fr[j], v[i][j]);
      const u32x4 packed = pack8(v[i]);
      *(u32x4*)(x + e0) = packed;
      unpack8(packed, v[i]);      // the LayerNorm sees what was stored
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  if (g) ln_row<NC>(v, sum, g, b, y, mean, rstd, row, d, eps, lane);
}

extern "C" int dmi_dropout_add_ln(const uint16_t* a, const uint16_t* residual, uint16_t* x_out, const uint16_t* gamma,
                                  const uint16_t* beta, uint16_t* y, float* mean, float* rstd, int64_t M, int d, uint64_t key,
                                  int thresh, float eps, void* stream) {
  DMI_REQUIRE(a && residual && x_out, "dropout_add_ln: null pointer (a, residual or x_out)");
  DMI_REQUIRE(!gamma || (beta && y && mean && rstd), "dropout_add_ln: null pointer (beta, y, mean or rstd with gamma given)");
  DMI_REQUIRE(d > 0 && d % 8 == 0 && d <= 4096 && M > 0, "dropout_add_ln: unsupported shape (need d %% 8 == 0, d <= 4096, M > 0: d=%d M=%lld)",
              d, (long long)M);
  DMI_REQUIRE_THRESH("dropout_add_ln", thresh);
  DMI_REQUIRE((((uintptr_t)a | (uintptr_t)residual | (uintptr_t)x_out | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) == 0,
              "dropout_add_ln: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const DropSite site = drop_site(key, thresh);
  dim3 grid((unsigned)cdiv64(M, 4)), blk(256);
  if (d <= 512) dropout_add_ln_kernel<1><<<grid, blk, 0, st>>>(a, residual, x_out, gamma, beta, y, mean, rstd, M, d, eps, site);
  else if (d <= 1024) dropout_add_ln_kernel<2><<<grid, blk, 0, st>>>(a, residual, x_out, gamma, beta, y, mean, rstd, M, d, eps, site);
  else if (d <= 2048) dropout_add_ln_kernel<4><<<grid, blk, 0, st>>>(a, residual, x_out, gamma, beta, y, mean, rstd, M, d, eps, site);
  else dropout_add_ln_kernel<8><<<grid, blk, 0, st>>>(a, residual, x_out, gamma, beta, y, mean, rstd, M, d, eps, site);
  DMI_CHECK_LAUNCH("dropout_add_ln");
  return DMI_OK;
}

// dy = drop(dx): the gradient of a dropped branch output.  A flat stream of 16-byte pieces (8 elements, two hashes) over M d elements.
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const bf16_t* __restrict__ dx, bf16_t* __restrict__ dy, int64_t n8, DropSite site) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    float f[8];
    unpack8(*(const u32x4*)(dx + i * 8), f);
    drop8(f, site, i * 8);
    *(u32x4*)(dy + i * 8) = pack8(f);
  }
}

extern "C" int dmi_dropout_bwd(const uint16_t* dx, uint16_t* dy, int64_t M, int d, uint64_t key, int thresh, void* stream) {
  DMI_REQUIRE(dx && dy, "dropout_bwd: null pointer");
  DMI_REQUIRE(d > 0 && d % 8 == 0 && M > 0, "dropout_bwd: unsupported shape (need d %% 8 == 0, M > 0: d=%d M=%lld)", d, (long long)M);
  DMI_REQUIRE_THRESH("dropout_bwd", thresh);
  DMI_REQUIRE((((uintptr_t)dx | (uintptr_t)dy) & 15) == 0, "dropout_bwd: buffers must be 16-byte aligned");
  const int64_t n8 = M * (int64_t)d / 8;
  int64_t blocks = cdiv64(n8, 256);
  if (blocks > 256 * 8) blocks = 256 * 8;     // 8 blocks of 4 waves per CU hold a stream of 16-byte requests; the rest is the grid stride
  dropout_bwd_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(dx, dy, n8, drop_site(key, thresh));
  DMI_CHECK_LAUNCH("dropout_bwd");
  return DMI_OK;
}

// =====================================================================================
// Rotary position embeddings (DESIGN.md §4 "Rotary"): q and k rotated in place in the qkv layout
// =====================================================================================
// One 16-byte piece = 8 bf16 = four adjacent pairs (2c, 2c+1) of one head; their (cos, sin) are 32 contiguous bytes of the table
// row [n = head_dim / 2][2].  col = the piece's first column inside [0, 2 H head_dim); head_dim is 64 or 128, so the element's
// place in its head is col & (head_dim - 1) and the table offset (in floats) equals it.  sgn = +1 rotates, -1 rotates back.
__device__ __forceinline__ void rope_piece(bf16_t* __restrict__ p, const float* __restrict__ cs_row, int col, int head_dim, float sgn) {
  const f32x4* t = (const f32x4*)(cs_row + (col & (head_dim - 1)));
  const f32x4 t0 = t[0], t1 = t[1];
  const float c[4] = {t0[0], t0[2], t1[0], t1[2]};
  const float s[4] = {t0[1] * sgn, t0[3] * sgn, t1[1] * sgn, t1[3] * sgn};
  float x[8], y[8];
  unpack8(*(const u32x4*)p, x);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    y[2 * j] = x[2 * j] * c[j] - x[2 * j + 1] * s[j];
    y[2 * j + 1] = x[2 * j] * s[j] + x[2 * j + 1] * c[j];
  }
  *(u32x4*)p = pack8(y);
}

// One wave per row and pass of the grid; lane l takes pieces l, l + 64, .. of the row's 2 H head_dim / 8.  The table row r % S
// is carried along (one modulo per wave, then additions), the row offset r * ld is 64-bit.
__global__ __launch_bounds__(256) void rope_qk_kernel(bf16_t* __restrict__ qkv, int ld, const float* __restrict__ cs, int64_t rows, int S,
                                                      int pieces, int head_dim, float sgn) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t r = (int64_t)blockIdx.x * 4 + wid;
  if (r >= rows) return;
  int s = (int)(r % S);
  const int ds = (int)(stride % S);
  for (; r < rows; r += stride) {
    bf16_t* row = qkv + r * (int64_t)ld;
    const float* cs_row = cs + (int64_t)s * head_dim;
#pragma unroll 2
    for (int c = lane; c < pieces; c += 64) rope_piece(row + c * 8, cs_row, c * 8, head_dim, sgn);
    s += ds;
    if (s >= S) s -= S;
  }
}

// The decode step: B rows of the [B, 3 H head_dim] staging buffer, all at table row pos (from device memory when pos_dev is given);
// a position outside [0, S) writes nothing.  One block per row.
__global__ __launch_bounds__(256) void rope_qk_decode_kernel(bf16_t* __restrict__ fresh, int ld, const float* __restrict__ cs, int S, int pieces,
                                                             int head_dim, int pos, const int* __restrict__ pos_dev) {
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= S) return;
  bf16_t* row = fresh + (int64_t)blockIdx.x * ld;
  const float* cs_row = cs + (int64_t)pos * head_dim;
  for (int c = threadIdx.x; c < pieces; c += 256) rope_piece(row + c * 8, cs_row, c * 8, head_dim, 1.f);
}

#define DMI_REQUIRE_ROPE(name, H, head_dim)                                                                                  \
  do {                                                                                                                       \
    if ((head_dim) != 64 && (head_dim) != 128) {                                                                             \
      dmi_set_error(name ": head_dim must be 64 or 128 (head_dim=%d)", (int)(head_dim));                                     \
      return DMI_ERR_UNSUPPORTED;                                                                                            \
    }                                                                                                                        \
    DMI_REQUIRE((H) > 0 && (int64_t)(H) * (head_dim) * 3 < (1ll << 31), name ": H must be positive and 3 H head_dim < 2^31 (H=%d)", (int)(H)); \
  } while (0)

extern "C" int dmi_rope_qk(uint16_t* qkv, int ld, const float* cs, int64_t rows, int S, int H, int head_dim, int inverse, void* stream) {
  DMI_REQUIRE(qkv && cs, "rope_qk: null pointer");
  DMI_REQUIRE_ROPE("rope_qk", H, head_dim);
  DMI_REQUIRE(rows > 0 && S > 0, "rope_qk: empty shape (rows=%lld S=%d)", (long long)rows, S);
  DMI_REQUIRE(ld >= 2 * H * head_dim && ld % 8 == 0, "rope_qk: ld must be a multiple of 8 and at least 2 H head_dim (ld=%d)", ld);
  DMI_REQUIRE((((uintptr_t)qkv | (uintptr_t)cs) & 15) == 0, "rope_qk: buffers must be 16-byte aligned");
  int64_t blocks = cdiv64(rows, 4);
  if (blocks > 256 * 8) blocks = 256 * 8;     // as dmi_dropout_bwd: 8 blocks of 4 waves per CU, the rest is the grid stride
  rope_qk_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(qkv, ld, cs, rows, S, 2 * H * head_dim / 8, head_dim,
                                                                                inverse ? -1.f : 1.f);
  DMI_CHECK_LAUNCH("rope_qk");
  return DMI_OK;
}

extern "C" int dmi_rope_qk_decode(uint16_t* fresh, const float* cs, int B, int S, int H, int head_dim, int pos, const int* pos_dev,
                                  void* stream) {
  DMI_REQUIRE(fresh && cs, "rope_qk_decode: null pointer");
  DMI_REQUIRE_ROPE("rope_qk_decode", H, head_dim);
  DMI_REQUIRE(B > 0 && S > 0, "rope_qk_decode: empty shape (B=%d S=%d)", B, S);
  DMI_REQUIRE(pos_dev || (pos >= 0 && pos < S), "rope_qk_decode: pos outside [0, S) (pos=%d S=%d)", pos, S);
  DMI_REQUIRE((((uintptr_t)fresh | (uintptr_t)cs) & 15) == 0, "rope_qk_decode: buffers must be 16-byte aligned");
  rope_qk_decode_kernel<<<dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream>>>(fresh, 3 * H * head_dim, cs, S, 2 * H * head_dim / 8, head_dim,
                                                                                  pos, pos_dev);
  DMI_CHECK_LAUNCH("rope_qk_decode");
  return DMI_OK;
}

// =====================================================================================
// QK normalisation (DESIGN.md §4 "QK norm"): q and k RMS-normalised per head with learned gains, in place in the qkv layout
// =====================================================================================
// As the rotation: one wave per row, lane l takes 16-byte pieces l, l + 64, ..; a head is G = head_dim / 8 adjacent pieces, so the G
// lanes that hold it are an aligned group of the wave (64 % G == 0 and the row's piece count is a multiple of G) and the head's sum
// is G's log2 xor-exchanges inside the wave -- no LDS, no atomics.  Every lane of the wave runs the exchanges; lanes behind the
// row's last piece carry zeros and store nothing.  y = (x r) (g c), c = head_dim^(-1/2) for q and 1 for k.
#define QKN_EPS 1e-6f
template <int HD>
__device__ __forceinline__ constexpr float qkn_scale() { return HD == 64 ? 0.125f : 0.08838834764831845f; }

template <int G, typename T>
__device__ __forceinline__ T qkn_group_sum(T x) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// the rotation of rope_piece on eight fp32 values: t = the piece's 8 floats of the table row, sgn = +1 rotates, -1 rotates back
template <typename T>
__device__ __forceinline__ void qkn_rotate8(T* y, const float* __restrict__ t, T sgn) {
  const f32x4 t0 = ((const f32x4*)t)[0], t1 = ((const f32x4*)t)[1];
  const T c[4] = {(T)t0[0], (T)t0[2], (T)t1[0], (T)t1[2]};
  const T s[4] = {(T)t0[1] * sgn, (T)t0[3] * sgn, (T)t1[1] * sgn, (T)t1[3] * sgn};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const T a = y[2 * j], b = y[2 * j + 1];
    y[2 * j] = a * c[j] - b * s[j];
    y[2 * j + 1] = a * s[j] + b * c[j];
  }
}

// one piece of the forward; col = its first column inside [0, 2 H head_dim), Hhd = H head_dim (columns below it are q's).  pre_p
// (nullable): where the unnormalised piece also goes.  cs_row (nullable): the table row whose rotation follows in fp32, so the
// result is rounded once.  The full and the decode kernel share this body: the same values give the same bits.
template <int HD>
__device__ __forceinline__ void qkn_fwd_piece(bf16_t* __restrict__ p, bf16_t* __restrict__ pre_p, const bf16_t* __restrict__ gq,
                                              const bf16_t* __restrict__ gk, const float* __restrict__ cs_row, int col, int Hhd,
                                              bool active) {
  u32x4 raw = {0u, 0u, 0u, 0u};
  if (active) raw = *(const u32x4*)p;
  float x[8], g[8], y[8];
  unpack8(raw, x);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = fmaf(x[j], x[j], ss);
  ss = qkn_group_sum<HD / 8>(ss);
  if (!active) return;
  const float r = rsqrtf(ss * (1.f / HD) + QKN_EPS);
  const bool isq = col < Hhd;
  const int j0 = col & (HD - 1);
  unpack8(*(const u32x4*)((isq ? gq : gk) + j0), g);
  const float c = isq ? qkn_scale<HD>() : 1.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = (x[j] * r) * (g[j] * c);
  if (pre_p) *(u32x4*)pre_p = raw;
  if (cs_row) qkn_rotate8<float>(y, cs_row + j0, 1.f);
  *(u32x4*)p = pack8(y);
}

template <int HD>
__global__ __launch_bounds__(256) void qk_norm_fwd_kernel(bf16_t* __restrict__ qkv, int ld, bf16_t* __restrict__ pre,
                                                          const bf16_t* __restrict__ gq, const bf16_t* __restrict__ gk,
                                                          const float* __restrict__ cs, int64_t rows, int S, int pieces) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t r = (int64_t)blockIdx.x * 4 + wid;
  if (r >= rows) return;      // (a whole wave leaves: the exchanges below stay inside one wave)
  int s = (int)(r % S);
  const int ds = (int)(stride % S);
  const int Hhd = pieces * 4;
  for (; r < rows; r += stride) {
    bf16_t* row = qkv + r * (int64_t)ld;
    bf16_t* prow = pre ? pre + r * (int64_t)(pieces * 8) : nullptr;
    const float* cs_row = cs ? cs + (int64_t)s * HD : nullptr;
    for (int c0 = 0; c0 < pieces; c0 += 64) {
      const int c = c0 + lane;
      qkn_fwd_piece<HD>(row + c * 8, prow ? prow + c * 8 : nullptr, gq, gk, cs_row, c * 8, Hhd, c < pieces);
    }
    s += ds;
    if (s >= S) s -= S;
  }
}

// The decode step: one block per row of the [B, 3 H head_dim] staging buffer.  With a table every row sits at table row pos (from
// device memory when pos_dev is given; outside [0, S) the launch writes nothing); without one the position is not read.
template <int HD>
__global__ __launch_bounds__(256) void qk_norm_decode_kernel(bf16_t* __restrict__ fresh, int ld, const bf16_t* __restrict__ gq,
                                                             const bf16_t* __restrict__ gk, const float* __restrict__ cs, int S,
                                                             int pieces, int pos, const int* __restrict__ pos_dev) {
  const float* cs_row = nullptr;
  if (cs) {
    if (pos_dev) pos = *pos_dev;
    if (pos < 0 || pos >= S) return;
    cs_row = cs + (int64_t)pos * HD;
  }
  bf16_t* row = fresh + (int64_t)blockIdx.x * ld;
  for (int c0 = 0; c0 < pieces; c0 += 256) {
    const int c = c0 + threadIdx.x;
    qkn_fwd_piece<HD>(row + c * 8, nullptr, gq, gk, cs_row, c * 8, pieces * 4, c < pieces);
  }
}

// Backward, in place on the q | k columns of dqkv; x = the unnormalised q | k the forward kept in `pre` (packed [rows, 2 H head_dim]).
// With a table dy is first rotated back (the transpose of the forward's rotation).  With xh = x r(x), u = g c, a = u dy:
//   dx = r (a - xh mean_j(a_j xh_j))            fp32, rounded once to bf16
//   dg_j = c sum_{rows, heads} dy_j xh_j        accumulated in float64 from float64 terms: the sum of squares and r are float64 (r for
//                                               dx is that r rounded to fp32); dy_j x_j, the product of two bf16 values, is
//                                               exact in fp32, and with a table the rotation's cos r, sin r are float64
// 1 / sqrt(a) in float64: the hardware seed (good to about 2^-23) and two Newton steps, each squaring the error
__device__ __forceinline__ double qkn_rsqrt64(double a) {
  double y = __builtin_amdgcn_rsq(a);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double e = fma(-a * y, y, 1.0);
    y = fma(0.5 * y, e, y);
  }
  return y;
}

// one piece: dp = its place in dqkv, xp in pre, u = the lane's eight g c, cs_piece = its 8 floats of the table row (ROPE), acc = the
// lane's eight float64 gain sums of this half (q or k)
template <int HD, bool ROPE>
__device__ __forceinline__ void qkn_bwd_piece(bf16_t* __restrict__ dp, const bf16_t* __restrict__ xp, const float* u,
                                              const float* __restrict__ cs_piece, bool active, double* acc) {
  constexpr int G = HD / 8;
  u32x4 rdy = {0u, 0u, 0u, 0u}, rx = {0u, 0u, 0u, 0u};
  if (active) {
    rdy = *(const u32x4*)dp;
    rx = *(const u32x4*)xp;
  }
  float fy[8], x[8];
  unpack8(rdy, fy);
  unpack8(rx, x);
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = fma((double)x[j], (double)x[j], ss);
  ss = qkn_group_sum<G>(ss);
  const double rd = qkn_rsqrt64(ss * (1.0 / HD) + (double)QKN_EPS);
  const float rf = (float)rd;
  if constexpr (ROPE) {
    // dy rotated back is (a c + b s, b c - a s) over the pair (a, b): its terms are sums of the exact fp32 products a x, b x times
    // c r, s r in float64; the dx path below takes the same rotation in fp32
    const f32x4 t0 = ((const f32x4*)cs_piece)[0], t1 = ((const f32x4*)cs_piece)[1];
    const float cc[4] = {t0[0], t0[2], t1[0], t1[2]}, sn[4] = {t0[1], t0[3], t1[1], t1[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ya = fy[2 * i], yb = fy[2 * i + 1], x0 = x[2 * i], x1 = x[2 * i + 1];
      const double cr = (double)cc[i] * rd, sr = (double)sn[i] * rd;
      acc[2 * i] = fma((double)(ya * x0), cr, fma((double)(yb * x0), sr, acc[2 * i]));
      acc[2 * i + 1] = fma((double)(yb * x1), cr, fma(-(double)(ya * x1), sr, acc[2 * i + 1]));
      fy[2 * i] = ya * cc[i] + yb * sn[i];
      fy[2 * i + 1] = yb * cc[i] - ya * sn[i];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fma((double)(fy[j] * x[j]), rd, acc[j]);
  }
  float a[8], xh[8];
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xh[j] = x[j] * rf;
    a[j] = u[j] * fy[j];
    t = fmaf(a[j], xh[j], t);
  }
  const float m = qkn_group_sum<G>(t) * (1.f / HD);
  if (active) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = rf * (a[j] - xh[j] * m);
    *(u32x4*)dp = pack8(o);
  }
}

// A lane's channel inside its head, (8 lane) mod head_dim, is the same in every pass over a row (64 pieces are a multiple of
// head_dim, and so is the row's q half), so it keeps eight q and eight k sums in registers for all its rows; the q half and the k half
// of a row are walked one after the other, which makes q-or-k a property of the loop, not of the lane.  The sums are then added over
// the wave's lanes of equal channel (xor-exchanges at distances G .. 32), over the block's four waves through LDS in a fixed order,
// and leave as one partial row [dgq | dgk] of 2 head_dim doubles per block.
template <int HD, bool ROPE>
__global__ __launch_bounds__(256) void qk_norm_bwd_kernel(bf16_t* __restrict__ dqkv, int ld, const bf16_t* __restrict__ pre,
                                                          const bf16_t* __restrict__ gq, const bf16_t* __restrict__ gk,
                                                          const float* __restrict__ cs, double* __restrict__ part, int64_t rows,
                                                          int S, int pieces) {
  constexpr int G = HD / 8;
  __shared__ double sm[4][2 * HD];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * 4;
  const int Q = pieces / 2;                       // the pieces of the q half; a multiple of G
  const int j0 = (lane * 8) & (HD - 1);
  float uq[8], uk[8];
  unpack8(*(const u32x4*)(gq + j0), uq);
  unpack8(*(const u32x4*)(gk + j0), uk);
#pragma unroll
  for (int j = 0; j < 8; ++j) uq[j] *= qkn_scale<HD>();
  double accq[8], acck[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) accq[j] = acck[j] = 0.0;
  int64_t r = (int64_t)blockIdx.x * 4 + wid;
  int s = (int)(r % S);
  const int ds = (int)(stride % S);
  for (; r < rows; r += stride) {
    bf16_t* drow = dqkv + r * (int64_t)ld;
    const bf16_t* prow = pre + r * (int64_t)(pieces * 8);
    const float* cs_piece = ROPE ? cs + (int64_t)s * HD + j0 : nullptr;
#pragma unroll 1
    for (int c = lane; c - lane < Q; c += 64) qkn_bwd_piece<HD, ROPE>(drow + c * 8, prow + c * 8, uq, cs_piece, c < Q, accq);
#pragma unroll 1
    for (int c = lane; c - lane < Q; c += 64)
      qkn_bwd_piece<HD, ROPE>(drow + (Q + c) * 8, prow + (Q + c) * 8, uk, cs_piece, c < Q, acck);
    s += ds;
    if (s >= S) s -= S;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
      accq[j] += __shfl_xor(accq[j], o, 64);
      acck[j] += __shfl_xor(acck[j], o, 64);
    }
  }
  if (lane < G) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sm[wid][j0 + j] = accq[j];
      sm[wid][HD + j0 + j] = acck[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * HD) {
    const int t = threadIdx.x;
    const double sum = (sm[0][t] + sm[1][t]) + (sm[2][t] + sm[3][t]);
    part[(int64_t)blockIdx.x * (2 * HD) + t] = t < HD ? sum * (HD == 64 ? 0.125 : 0.08838834764831845) : sum;   // c in float64
  }
}

// dgq | dgk = the column sums of the P partial rows, in a fixed order, rounded once to fp32: 16 columns x 16 row groups per block
__global__ __launch_bounds__(256) void qk_norm_bwd_finish_kernel(const double* __restrict__ part, float* __restrict__ dgq,
                                                                 float* __restrict__ dgk, int P, int hd) {
  __shared__ double sm[16][17];
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int nc = 2 * hd;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < nc) {
    int p = grp;
    for (; p + 48 < P; p += 64) {      // four independent loads in flight per thread
      const double* q = part + (int64_t)p * nc + c;
      a0 += q[0];
      a1 += q[16 * nc];
      a2 += q[32 * nc];
      a3 += q[48 * nc];
    }
    for (; p < P; p += 16) a0 += part[(int64_t)p * nc + c];
  }
  sm[grp][cl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (grp == 0 && c < nc) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += sm[q][cl];
    if (c < hd) dgq[c] = (float)s;
    else dgk[c - hd] = (float)s;
  }
}

// blocks of four rows, at most 8 per CU (as dmi_rope_qk); the backward leaves one partial row per block
static inline int64_t qkn_blocks(int64_t rows) {
  const int64_t blocks = cdiv64(rows, 4);
  return blocks > 256 * 8 ? 256 * 8 : blocks;
}

#define DMI_REQUIRE_QKN(name, ld, rows, S, H, head_dim)                                                                          \
  do {                                                                                                                           \
    DMI_REQUIRE_ROPE(name, H, head_dim);                                                                                         \
    DMI_REQUIRE((rows) > 0 && (S) > 0, name ": empty shape (rows=%lld S=%d)", (long long)(rows), (int)(S));                       \
    DMI_REQUIRE((ld) >= 2 * (H) * (head_dim) && (ld) % 8 == 0, name ": ld must be a multiple of 8 and at least 2 H head_dim (ld=%d)", \
                (int)(ld));                                                                                                      \
  } while (0)

extern "C" int dmi_qk_norm_fwd(uint16_t* qkv, int ld, uint16_t* pre, const uint16_t* gq, const uint16_t* gk, const float* cs,
                               int64_t rows, int S, int H, int head_dim, void* stream) {
  DMI_REQUIRE(qkv && gq && gk, "qk_norm_fwd: null pointer");
  DMI_REQUIRE_QKN("qk_norm_fwd", ld, rows, S, H, head_dim);
  DMI_REQUIRE((((uintptr_t)qkv | (uintptr_t)pre | (uintptr_t)gq | (uintptr_t)gk | (uintptr_t)cs) & 15) == 0,
              "qk_norm_fwd: buffers must be 16-byte aligned");
  const dim3 grid((unsigned)qkn_blocks(rows)), blk(256);
  const int pieces = 2 * H * head_dim / 8;
  if (head_dim == 64) qk_norm_fwd_kernel<64><<<grid, blk, 0, (hipStream_t)stream>>>(qkv, ld, pre, gq, gk, cs, rows, S, pieces);
  else qk_norm_fwd_kernel<128><<<grid, blk, 0, (hipStream_t)stream>>>(qkv, ld, pre, gq, gk, cs, rows, S, pieces);
  DMI_CHECK_LAUNCH("qk_norm_fwd");
  return DMI_OK;
}

extern "C" int64_t dmi_qk_norm_bwd_workspace_bytes(int64_t rows, int head_dim) {
  return rows > 0 && head_dim > 0 ? qkn_blocks(rows) * 2 * (int64_t)head_dim * 8 : 0;
}

extern "C" int dmi_qk_norm_bwd(uint16_t* dqkv, int ld, const uint16_t* pre, const uint16_t* gq, const uint16_t* gk, const float* cs,
                               float* dgq, float* dgk, void* workspace, int64_t rows, int S, int H, int head_dim, void* stream) {
  DMI_REQUIRE(dqkv && pre && gq && gk && dgq && dgk && workspace, "qk_norm_bwd: null pointer");
  DMI_REQUIRE_QKN("qk_norm_bwd", ld, rows, S, H, head_dim);
  DMI_REQUIRE((((uintptr_t)dqkv | (uintptr_t)pre | (uintptr_t)gq | (uintptr_t)gk | (uintptr_t)cs | (uintptr_t)dgq | (uintptr_t)dgk |
                (uintptr_t)workspace) & 15) == 0, "qk_norm_bwd: buffers must be 16-byte aligned");
  const int P = (int)qkn_blocks(rows);
  const dim3 grid((unsigned)P), blk(256);
  const int pieces = 2 * H * head_dim / 8;
  double* part = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (head_dim == 64 && cs) qk_norm_bwd_kernel<64, true><<<grid, blk, 0, st>>>(dqkv, ld, pre, gq, gk, cs, part, rows, S, pieces);
  else if (head_dim == 64) qk_norm_bwd_kernel<64, false><<<grid, blk, 0, st>>>(dqkv, ld, pre, gq, gk, cs, part, rows, S, pieces);
  else if (cs) qk_norm_bwd_kernel<128, true><<<grid, blk, 0, st>>>(dqkv, ld, pre, gq, gk, cs, part, rows, S, pieces);
  else qk_norm_bwd_kernel<128, false><<<grid, blk, 0, st>>>(dqkv, ld, pre, gq, gk, cs, part, rows, S, pieces);
  DMI_CHECK_LAUNCH("qk_norm_bwd");
  qk_norm_bwd_finish_kernel<<<dim3((2 * head_dim + 15) / 16), blk, 0, st>>>(part, dgq, dgk, P, head_dim);
  DMI_CHECK_LAUNCH("qk_norm_bwd_finish");
  return DMI_OK;
}

extern "C" int dmi_qk_norm_decode(uint16_t* fresh, const uint16_t* gq, const uint16_t* gk, const float* cs, int B, int S, int H,
                                  int head_dim, int pos, const int* pos_dev, void* stream) {
  DMI_REQUIRE(fresh && gq && gk, "qk_norm_decode: null pointer");
  DMI_REQUIRE_ROPE("qk_norm_decode", H, head_dim);
  DMI_REQUIRE(B > 0 && S > 0, "qk_norm_decode: empty shape (B=%d S=%d)", B, S);
  DMI_REQUIRE(!cs || pos_dev || (pos >= 0 && pos < S), "qk_norm_decode: pos outside [0, S) (pos=%d S=%d)", pos, S);
  DMI_REQUIRE((((uintptr_t)fresh | (uintptr_t)gq | (uintptr_t)gk | (uintptr_t)cs) & 15) == 0,
              "qk_norm_decode: buffers must be 16-byte aligned");
  const dim3 grid((unsigned)B), blk(256);
  const int ld = 3 * H * head_dim, pieces = 2 * H * head_dim / 8;
  if (head_dim == 64) qk_norm_decode_kernel<64><<<grid, blk, 0, (hipStream_t)stream>>>(fresh, ld, gq, gk, cs, S, pieces, pos, pos_dev);
  else qk_norm_decode_kernel<128><<<grid, blk, 0, (hipStream_t)stream>>>(fresh, ld, gq, gk, cs, S, pieces, pos, pos_dev);
  DMI_CHECK_LAUNCH("qk_norm_decode");
  return DMI_OK;
}

// =====================================================================================
// Token shift (DESIGN.md §4 "Token shift"): half of every row's channels gathered from an earlier row of its sequence
// =====================================================================================
// The row a 16-byte piece of sequence position s is read from, as an offset in rows; TS_ZERO: the piece is +0.  ch = the piece's
// first channel; a quarter of d is whole pieces (d % 32 == 0).  Caption positions s < T take both shifted quarters from the previous
// position; image token k = s - T of the G x G grid takes [0, d/4) from above (k - G) and [d/4, d/2) from the left (k - 1, not
// across the row's start).  inverse: the transpose, again a gather, from the next position / the row below / the right.
#define TS_ZERO 0x7fffffff
__device__ __forceinline__ int ts_source(int s, int ch, int T, int G, int d, bool inverse) {
  if (ch >= (d >> 1)) return 0;
  const bool up = ch < (d >> 2);
  if (s < T) return inverse ? (s + 1 < T ? 1 : TS_ZERO) : (s >= 1 ? -1 : TS_ZERO);
  const int k = s - T;
  if (up) return inverse ? (k + G < G * G ? G : TS_ZERO) : (k >= G ? -G : TS_ZERO);
  const int c = k % G;
  return inverse ? (c + 1 < G ? 1 : TS_ZERO) : (c >= 1 ? -1 : TS_ZERO);
}

// A flat stream of 16-byte pieces over rows * d elements, as dmi_dropout_bwd.  (row, piece in row, position in sequence) of a lane
// are carried along the grid stride by additions: the only divisions are 32-bit and happen once per lane.
__global__ __launch_bounds__(256) void token_shift_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, bf16_t* __restrict__ hist,
                                                          int64_t rows, int S, int T, int G, int d, int inverse) {
  const int vpr = d >> 3;                                   // pieces per row
  const unsigned first = blockIdx.x * 256u + threadIdx.x;   // < 2^19: the grid is capped
  const unsigned stride = gridDim.x * 256u;
  int64_t row = first / (unsigned)vpr;
  int v = (int)(first % (unsigned)vpr);
  int s = (int)((unsigned)row % (unsigned)S);
  const int drow = (int)(stride / (unsigned)vpr), dv = (int)(stride % (unsigned)vpr), ds = drow % S;
  const int half = d >> 1;
  while (row < rows) {
    const int ch = v * 8;
    const int off = ts_source(s, ch, T, G, d, inverse != 0);
    u32x4 val = {0u, 0u, 0u, 0u};
    if (off != TS_ZERO) val = *(const u32x4*)(x + (row + off) * (int64_t)d + ch);
    *(u32x4*)(y + row * (int64_t)d + ch) = val;
    if (hist != nullptr && ch < half) *(u32x4*)(hist + row * (int64_t)half + ch) = *(const u32x4*)(x + row * (int64_t)d + ch);
    v += dv;
    row += drow;
    s += ds;
    if (v >= vpr) { v -= vpr; ++row; ++s; }
    if (s >= S) s -= S;
  }
}

// The decode step: the row of position pos of B sequences (pos from device memory when pos_dev is given; outside [0, S) nothing
// is written).  y[b] = shift of x[b] with the neighbours' halves read from hist[B, S, d/2]; hist[b, pos] <- x[b, :d/2].  One block
// per sequence; the rows read (pos - 1, pos - G) are never the row written.
__global__ __launch_bounds__(256) void token_shift_decode_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ hist, bf16_t* __restrict__ y,
                                                                 int S, int T, int G, int d, int pos, const int* __restrict__ pos_dev) {
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= S) return;
  const int half = d >> 1;
  const bf16_t* xr = x + (int64_t)blockIdx.x * d;
  bf16_t* yr = y + (int64_t)blockIdx.x * d;
  bf16_t* hs = hist + (int64_t)blockIdx.x * S * half;
  for (int ch = threadIdx.x * 8; ch < d; ch += 256 * 8) {
    const u32x4 own = *(const u32x4*)(xr + ch);
    u32x4 val = own;
    if (ch < half) {
      const int off = ts_source(pos, ch, T, G, d, false);
      val = u32x4{0u, 0u, 0u, 0u};
      if (off != TS_ZERO) val = *(const u32x4*)(hs + (int64_t)(pos + off) * half + ch);
      *(u32x4*)(hs + (int64_t)pos * half + ch) = own;
    }
    *(u32x4*)(yr + ch) = val;
  }
}

#define DMI_REQUIRE_SHIFT(name, S, T, G, d)                                                                                   \
  do {                                                                                                                        \
    DMI_REQUIRE((T) >= 1 && (G) >= 1, name ": T and G must be at least 1 (T=%d G=%d)", (int)(T), (int)(G));                   \
    DMI_REQUIRE((int64_t)(S) == (int64_t)(T) + (int64_t)(G) * (G), name ": S must equal T + G * G (S=%d T=%d G=%d)", (int)(S), (int)(T), (int)(G)); \
    DMI_REQUIRE((d) >= 32 && (d) % 32 == 0, name ": d must be a positive multiple of 32 (d=%d)", (int)(d));                   \
  } while (0)

static inline bool ts_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + (uintptr_t)bytes && q < p + (uintptr_t)bytes;
}

extern "C" int dmi_token_shift(const uint16_t* x, uint16_t* y, uint16_t* hist, int64_t rows, int S, int T, int G, int d, int inverse,
                               void* stream) {
  DMI_REQUIRE(x && y, "token_shift: null pointer");
  DMI_REQUIRE(rows > 0 && S > 0 && d > 0, "token_shift: empty shape (rows=%lld S=%d d=%d)", (long long)rows, S, d);
  DMI_REQUIRE_SHIFT("token_shift", S, T, G, d);
  DMI_REQUIRE(rows % S == 0, "token_shift: rows must be a multiple of S (rows=%lld S=%d)", (long long)rows, S);
  DMI_REQUIRE(!(hist && inverse), "token_shift: hist goes with the forward only (inverse=%d)", inverse);
  DMI_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)hist) & 15) == 0, "token_shift: buffers must be 16-byte aligned");
  DMI_REQUIRE(!ts_overlap(x, y, rows * (int64_t)d * 2), "token_shift: x and y overlap (the shift is out of place)");
  const int64_t n8 = rows * (int64_t)(d / 8);
  int64_t blocks = cdiv64(n8, 256);
  if (blocks > 256 * 8) blocks = 256 * 8;     // as dmi_dropout_bwd: 8 blocks of 4 waves per CU, the rest is the grid stride
  token_shift_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(x, y, hist, rows, S, T, G, d, inverse);
  DMI_CHECK_LAUNCH("token_shift");
  return DMI_OK;
}

extern "C" int dmi_token_shift_decode(const uint16_t* x, uint16_t* hist, uint16_t* y, int B, int S, int T, int G, int d, int pos,
                                      const int* pos_dev, void* stream) {
  DMI_REQUIRE(x && hist && y, "token_shift_decode: null pointer");
  DMI_REQUIRE(B > 0 && S > 0 && d > 0, "token_shift_decode: empty shape (B=%d S=%d d=%d)", B, S, d);
  DMI_REQUIRE_SHIFT("token_shift_decode", S, T, G, d);
  DMI_REQUIRE(pos_dev || (pos >= 0 && pos < S), "token_shift_decode: pos outside [0, S) (pos=%d S=%d)", pos, S);
  DMI_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)hist) & 15) == 0, "token_shift_decode: buffers must be 16-byte aligned");
  DMI_REQUIRE(!ts_overlap(x, y, (int64_t)B * d * 2), "token_shift_decode: x and y overlap (the shift is out of place)");
  token_shift_decode_kernel<<<dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream>>>(x, hist, y, S, T, G, d, pos, pos_dev);
  DMI_CHECK_LAUNCH("token_shift_decode");
  return DMI_OK;
}

// ---- generic deterministic partial reduce: out[c] = sum_{p<P} part[p*ncols + c]
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                              int P, int ncols) {
  __shared__ float sm[4][64];
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float acc = 0.f;
  if (c < ncols) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // 4 independent chains keep 4+ loads in flight
    int p = grp;
    for (; p + 12 < P; p += 16) {
      a0 += part[(int64_t)p * ncols + c];
      a1 += part[(int64_t)(p + 4) * ncols + c];
      a2 += part[(int64_t)(p + 8) * ncols + c];
      a3 += part[(int64_t)(p + 12) * ncols + c];
    }
    for (; p < P; p += 4) a0 += part[(int64_t)p * ncols + c];
    acc = (a0 + a1) + (a2 + a3);
  }
  sm[grp][cl] = acc;
  __syncthreads();
  if (grp == 0 && c < ncols) out[c] = (sm[0][cl] + sm[1][cl]) + (sm[2][cl] + sm[3][cl]);
}

#define LN_BWD_RPB 32  // rows per block (8 per wave): 1280 blocks at M = 40960 -> ~20 waves/CU hide the per-row latency chain
extern "C" int64_t dmi_layernorm_bwd_workspace_bytes(int64_t rows, int d) {
  return cdiv64(rows, LN_BWD_RPB) * 2 * (int64_t)d * 4;
}

// dx = rstd * (dy*g - mean_j(dy*g) - xhat * mean_j(dy*g*xhat)) (+ dres);  partial dg/db per block.
template <int NC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                     const bf16_t* __restrict__ g, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const bf16_t* __restrict__ dres,
                                                     bf16_t* __restrict__ dx, float* __restrict__ part,
                                                     int64_t rows, int d) {
  extern __shared__ __attribute__((aligned(16))) float sm[];  // [4][2][d]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nch = d / 8;
  float ag[NC][8], ab[NC][8], fg[NC][8];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
#pragma unroll
    for (int j = 0; j < 8; ++j) ag[i][j] = ab[i][j] = 0.f;
    if (c < nch) unpack8(*(const u32x4*)(g + c * 8), fg[i]);
  }
  const int64_t r0 = (int64_t)blockIdx.x * LN_BWD_RPB;
  // software pipeline over this wave's rows: the raw loads of row it+1 are issued before the reductions of row it
  u32x4 rdy[NC], rx[NC], rr[NC];
  float mu_n = 0.f, rs_n = 0.f;
  auto fetch = [&](int64_t row) {
    if (row < rows) {
      mu_n = mean[row];
      rs_n = rstd[row];
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
          rdy[i] = *(const u32x4*)(dy + row * d + c * 8);
          rx[i] = *(const u32x4*)(x + row * d + c * 8);
          if (dres) rr[i] = *(const u32x4*)(dres + row * d + c * 8);
        }
      }
    }
  };
  fetch(r0 + wid);
  for (int it = 0; it < LN_BWD_RPB / 4; ++it) {
    const int64_t row = r0 + wid + 4 * it;
    if (row >= rows) break;
    const float mu = mu_n, rs = rs_n;
    float fy[NC][8], xh[NC][8], fr[NC][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        float fx[8];
        unpack8(rdy[i], fy[i]);
        unpack8(rx[i], fx);
        if (dres) unpack8(rr[i], fr[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[i][j] = (fx[j] - mu) * rs;
          ab[i][j] += fy[i][j];
          ag[i][j] += fy[i][j] * xh[i][j];
          fy[i][j] *= fg[i][j];  // dy*g
          s1 += fy[i][j];
          s2 += fy[i][j] * xh[i][j];
        }
      }
    }
    if (it + 1 < LN_BWD_RPB / 4) fetch(row + 4);
    s1 = wave_sum(s1) / (float)d;
    s2 = wave_sum(s2) / (float)d;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = rs * (fy[i][j] - s1 - xh[i][j] * s2);
        if (dres) {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += fr[i][j];
        }
        *(u32x4*)(dx + row * d + c * 8) = pack8(o);
      }
    }
  }
  // cross-wave combine, one partial row per block
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sm[(wid * 2 + 0) * d + c * 8 + j] = ag[i][j];
        sm[(wid * 2 + 1) * d + c * 8 + j] = ab[i][j];
      }
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * d; idx += 256) {
    const int which = idx / d, col = idx % d;
    float s = (sm[(0 * 2 + which) * d + col] + sm[(1 * 2 + which) * d + col]) +
              (sm[(2 * 2 + which) * d + col] + sm[(3 * 2 + which) * d + col]);
    part[(int64_t)blockIdx.x * 2 * d + idx] = s;
  }
}

// out layout of the reduce: [dg(d) | db(d)] -> two destination pointers.  16 columns x 16 row-groups per block
// (2d/16 blocks), 2 independent chains per thread.
__global__ __launch_bounds__(256) void ln_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ dg,
                                                            float* __restrict__ db, int P, int d) {
  __shared__ float sm[16][17];
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int64_t nc = 2 * (int64_t)d;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
  if (c < nc) {
    int p = grp;
    for (; p + 112 < P; p += 128) {  // eight independent loads in flight per thread
      const float* q = part + (int64_t)p * nc + c;
      a0 += q[0];
      a1 += q[16 * nc];
      a2 += q[32 * nc];
      a3 += q[48 * nc];
      a4 += q[64 * nc];
      a5 += q[80 * nc];
      a6 += q[96 * nc];
      a7 += q[112 * nc];
    }
    for (; p < P; p += 16) a0 += part[(int64_t)p * nc + c];
  }
  sm[grp][cl] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  __syncthreads();
  if (grp == 0 && c < nc) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += sm[q][cl];
    if (c < d) dg[c] = s;
    else db[c - d] = s;
  }
}

extern "C" int dmi_layernorm_bwd(const uint16_t* dy, const uint16_t* x, const uint16_t* g, const float* mean,
                                 const float* rstd, const uint16_t* dres, uint16_t* dx, float* dg, float* db,
                                 void* workspace, int64_t rows, int d, void* stream) {
  DMI_REQUIRE(dy && x && g && mean && rstd && dx && workspace && ((dg && db) || (!dg && !db)), "layernorm_bwd: null pointer");
  DMI_REQUIRE(d % 8 == 0 && d <= 2048 && rows > 0, "layernorm_bwd: unsupported d=%d (need d%%8==0, d<=2048)", d);
  hipStream_t st = (hipStream_t)stream;
  const int P = (int)cdiv64(rows, LN_BWD_RPB);
  const size_t shm = (size_t)4 * 2 * d * sizeof(float);
  float* part = (float*)workspace;
  dim3 grid(P), blk(256);
  if (d <= 512) ln_bwd_kernel<1><<<grid, blk, shm, st>>>(dy, x, g, mean, rstd, dres, dx, part, rows, d);
  else if (d <= 1024) ln_bwd_kernel<2><<<grid, blk, shm, st>>>(dy, x, g, mean, rstd, dres, dx, part, rows, d);
  else ln_bwd_kernel<4><<<grid, blk, shm, st>>>(dy, x, g, mean, rstd, dres, dx, part, rows, d);
  DMI_CHECK_LAUNCH("layernorm_bwd");
  if (dg == nullptr && db == nullptr) return DMI_OK;   // deferred: the caller reduces the partials with dmi_layernorm_bwd_finish_batch
  ln_bwd_finish_kernel<<<dim3((2 * d + 15) / 16), blk, 0, st>>>(part, dg, db, P, d);
  DMI_CHECK_LAUNCH("layernorm_bwd_finish");
  return DMI_OK;
}

// dg | db = column sums of P partial rows [2 d] (the reduce behind dmi_layernorm_bwd, for partials produced elsewhere: the fused
// LayerNorm backward of dmi_gemm_nt_lnbwd)
extern "C" int dmi_layernorm_bwd_finish_parts(const float* part, int P, float* dg, float* db, int d, void* stream) {
  DMI_REQUIRE(part && dg && db && P > 0 && d % 8 == 0 && d <= 2048, "layernorm_bwd_finish_parts: bad arguments");
  ln_bwd_finish_kernel<<<dim3((2 * d + 15) / 16), dim3(256), 0, (hipStream_t)stream>>>(part, dg, db, P, d);
  DMI_CHECK_LAUNCH("layernorm_bwd_finish_parts");
  return DMI_OK;
}

// The gain / bias gradients of several LayerNorms reduced in ONE launch: blockIdx.y = the LayerNorm.  Each of the 13 reduces of a
// dalle_example step is a 64-block kernel of ~7 us; the results are only needed by the gradient exchange / the optimizer.
#define LN_FINISH_MAX 16
struct LnFinishBatch {
  const float* part[LN_FINISH_MAX];
  float* dg[LN_FINISH_MAX];
  float* db[LN_FINISH_MAX];
  int P[LN_FINISH_MAX];
  int d;
};
__global__ __launch_bounds__(256) void ln_bwd_finish_batch_kernel(LnFinishBatch b) {
  __shared__ float sm[16][17];
  const int it = blockIdx.y;
  const float* __restrict__ part = b.part[it];
  const int P = b.P[it], d = b.d;
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int64_t nc = 2 * (int64_t)d;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
  if (c < nc) {   // the same fixed summation order as ln_bwd_finish_kernel: bit-identical results
    int p = grp;
    for (; p + 112 < P; p += 128) {
      const float* q = part + (int64_t)p * nc + c;
      a0 += q[0];
      a1 += q[16 * nc];
      a2 += q[32 * nc];
      a3 += q[48 * nc];
      a4 += q[64 * nc];
      a5 += q[80 * nc];
      a6 += q[96 * nc];
      a7 += q[112 * nc];
    }
    for (; p < P; p += 16) a0 += part[(int64_t)p * nc + c];
  }
  sm[grp][cl] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  __syncthreads();
  if (grp == 0 && c < nc) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += sm[q][cl];
    if (c < d) b.dg[it][c] = s;
    else b.db[it][c - d] = s;
  }
}
extern "C" int dmi_layernorm_bwd_finish_batch(const void* const* workspaces, float* const* dgs, float* const* dbs, const int64_t* rows,
                                              int n, int d, void* stream) {
  DMI_REQUIRE(workspaces && dgs && dbs && rows && n >= 1 && n <= LN_FINISH_MAX, "layernorm_bwd_finish_batch: 1..%d items", LN_FINISH_MAX);
  DMI_REQUIRE(d % 8 == 0 && d <= 2048, "layernorm_bwd_finish_batch: unsupported d=%d", d);
  LnFinishBatch b;
  b.d = d;
  for (int i = 0; i < n; ++i) {
    DMI_REQUIRE(workspaces[i] && dgs[i] && dbs[i] && rows[i] > 0, "layernorm_bwd_finish_batch: null pointer in item %d", i);
    b.part[i] = (const float*)workspaces[i]; b.dg[i] = dgs[i]; b.db[i] = dbs[i];
    b.P[i] = (int)cdiv64(rows[i], LN_BWD_RPB);
  }
  ln_bwd_finish_batch_kernel<<<dim3((2 * d + 15) / 16, n), dim3(256), 0, (hipStream_t)stream>>>(b);
  DMI_CHECK_LAUNCH("layernorm_bwd_finish_batch");
  return DMI_OK;
}

// =====================================================================================
// column sum (bias gradients)
// =====================================================================================
#define COLSUM_RPB 256
extern "C" int64_t dmi_colsum_workspace_bytes(int64_t M, int N) { return cdiv64(M, COLSUM_RPB) * (int64_t)N * 4; }

__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ Y, int ldy, float* __restrict__ part,
                                                     int64_t M, int N) {
  __shared__ float sm[4][64][8];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int cg = blockIdx.x * 64 + cl;  // group of 8 columns
  const int64_t r0 = (int64_t)blockIdx.y * COLSUM_RPB;
  const int64_t r1 = (r0 + COLSUM_RPB < M) ? r0 + COLSUM_RPB : M;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (cg * 8 < N) {
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      float f[8];
      unpack8(*(const u32x4*)(Y + r * ldy + cg * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sm[rl][cl][j] = acc[j];
  __syncthreads();
  if (rl == 0 && cg * 8 < N) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      part[(int64_t)blockIdx.y * N + cg * 8 + j] = (sm[0][cl][j] + sm[1][cl][j]) + (sm[2][cl][j] + sm[3][cl][j]);
  }
}

extern "C" int dmi_colsum(const uint16_t* Y, int ldy, float* out, int64_t M, int N, void* workspace, void* stream) {
  DMI_REQUIRE(Y && out && workspace, "colsum: null pointer");
  DMI_REQUIRE(N % 8 == 0 && ldy % 8 == 0 && M > 0, "colsum: N,ldy must be multiples of 8");
  hipStream_t st = (hipStream_t)stream;
  const int P = (int)cdiv64(M, COLSUM_RPB);
  colsum_kernel<<<dim3((N / 8 + 63) / 64, P), dim3(256), 0, st>>>(Y, ldy, (float*)workspace, M, N);
  DMI_CHECK_LAUNCH("colsum");
  reduce_partials_kernel<<<dim3((N + 63) / 64), dim3(256), 0, st>>>((const float*)workspace, out, P, N);
  DMI_CHECK_LAUNCH("colsum_reduce");
  return DMI_OK;
}

// =====================================================================================
// batched bf16 transpose: element (b,h,r,c) at in + b*sb + h*sh + r*sr + c  ->  out[((b*nh+h)*C + c)*R + r]
// =====================================================================================
// Rv = valid input rows, R = output row pitch (>= Rv; rows in [Rv, R) are written as zeros)
__device__ __forceinline__ void transpose_tile(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int Rv, int R,
                                               int C, int64_t sr, int r0, int c0, unsigned (*t)[33]) {
  const int tid = threadIdx.x;
  {
    const int chunk = tid & 7, rp = tid >> 3;
    const int ra = r0 + 2 * rp, c = c0 + 8 * chunk;
    u32x4 va = {0, 0, 0, 0}, vb = {0, 0, 0, 0};
    if (c < C) {
      if (ra < Rv) va = *(const u32x4*)(src + (int64_t)ra * sr + c);
      if (ra + 1 < Rv) vb = *(const u32x4*)(src + (int64_t)(ra + 1) * sr + c);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned lo = (va[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
      const unsigned hi = (vb[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
      t[8 * chunk + j][rp] = lo | (hi << 16);
    }
  }
  __syncthreads();
  {
    const int orow = tid >> 2, seg = tid & 3;
    const int c = c0 + orow, r = r0 + 16 * seg;
    if (c < C) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rr = r + 8 * q;
        if (rr < R) {
          u32x4 v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = t[orow][8 * seg + 4 * q + i];
          *(u32x4*)(dst + (int64_t)c * R + rr) = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void transpose_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                        int nh, int Rv, int R, int C, int64_t sb, int64_t sh, int64_t sr) {
  __shared__ unsigned t[64][33];
  const int bh = blockIdx.z, b = bh / nh, h = bh % nh;
  transpose_tile(in + b * sb + h * sh, out + (int64_t)bh * C * R, Rv, R, C, sr, blockIdx.y * 64, blockIdx.x * 64, t);
}

// Many independent [R,C] -> [C,R] transposes inside one pair of buffers in ONE launch (the per-step refresh of the
// forward GEMMs' [out,in] weight copies was 25 launches of ~5 us each).  table[i] = {in_off, out_off, R, C,
// first_tile} in elements / 64x64 tiles, first_tile ascending.
__global__ __launch_bounds__(256) void transpose_batch_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                              const int64_t* __restrict__ table, int n) {
  __shared__ unsigned t[64][33];
  const int64_t tile = blockIdx.x;
  int i = 0;
  while (i + 1 < n && table[(i + 1) * 5 + 4] <= tile) ++i;
  const int64_t in_off = table[i * 5], out_off = table[i * 5 + 1];
  const int R = (int)table[i * 5 + 2], C = (int)table[i * 5 + 3];
  const int local = (int)(tile - table[i * 5 + 4]);
  const int tc = (C + 63) / 64;
  transpose_tile(in + in_off, out + out_off, R, R, C, C, (local / tc) * 64, (local % tc) * 64, t);
}
extern "C" int dmi_transpose_bf16_batch(const uint16_t* in_base, uint16_t* out_base, const int64_t* table, int n,
                                        int64_t total_tiles, void* stream) {
  DMI_REQUIRE(in_base && out_base && table && n > 0 && total_tiles > 0, "transpose_batch: bad args");
  transpose_batch_kernel<<<dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream>>>(in_base, out_base, table, n);
  DMI_CHECK_LAUNCH("transpose_batch");
  return DMI_OK;
}

static int dmi_transpose_padded(const uint16_t* in, uint16_t* out, int nb, int nh, int Rv, int Rp, int C,
                         int64_t in_b_stride, int64_t in_h_stride, int64_t in_r_stride, void* stream) {
  DMI_REQUIRE(in && out, "transpose: null pointer");
  DMI_REQUIRE(Rp % 8 == 0 && Rp >= Rv && C % 8 == 0 && in_r_stride % 8 == 0 && in_h_stride % 8 == 0 && in_b_stride % 8 == 0,
              "transpose: R, C and strides must be multiples of 8 (R=%d C=%d)", Rp, C);
  transpose_kernel<<<dim3((C + 63) / 64, (Rp + 63) / 64, nb * nh), dim3(256), 0, (hipStream_t)stream>>>(
      in, out, nh, Rv, Rp, C, in_b_stride, in_h_stride, in_r_stride);
  DMI_CHECK_LAUNCH("transpose");
  return DMI_OK;
}
extern "C" int dmi_transpose_bf16_padded(const uint16_t* in, uint16_t* out, int R_valid, int R_pitch, int C, void* stream) {
  return dmi_transpose_padded(in, out, 1, 1, R_valid, R_pitch, C, 0, 0, C, stream);
}
extern "C" int dmi_transpose_bf16(const uint16_t* in, uint16_t* out, int batch, int R, int C, void* stream) {
  return dmi_transpose_padded(in, out, batch, 1, R, R, C, (int64_t)R * C, 0, C, stream);
}

// =====================================================================================
// integer paths (bit-exact): label shift (models.py:407-410), token assembly (model_fns.py:76-77,118-119)
// =====================================================================================
__global__ void shift_labels_kernel(const int* __restrict__ tokens, int* __restrict__ labels, int B, int S, int eos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * S) return;
  const int s = (int)(i % S);
  labels[i] = (s == S - 1) ? eos : tokens[i + 1];
}
extern "C" int dmi_shift_labels(const int32_t* tokens, int32_t* labels, int B, int S, int eos, void* stream) {
  DMI_REQUIRE(tokens && labels && B > 0 && S > 0, "shift_labels: bad args");
  const int64_t n = (int64_t)B * S;
  shift_labels_kernel<<<dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream>>>(tokens, labels, B, S, eos);
  DMI_CHECK_LAUNCH("shift_labels");
  return DMI_OK;
}

// one wave per (b, p): argmax over C fp32 logits, first max on ties (tf.math.argmax), + text_vocab
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const int* __restrict__ text,
                                                              const float* __restrict__ logits, int* __restrict__ out,
                                                              int B, int T, int P, int C, int text_vocab) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t idx = (int64_t)blockIdx.x * 4 + wid;
  const int S = T + P;
  if (idx >= (int64_t)B * S) return;
  const int b = (int)(idx / S), s = (int)(idx % S);
  if (s < T) {
    if (lane == 0) out[idx] = text[(int64_t)b * T + s];
    return;
  }
  const float* row = logits + ((int64_t)b * P + (s - T)) * C;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = row[c];
    if (v > best || (v == best && c < bi)) {
      best = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) out[idx] = (bi == 0x7fffffff ? 0 : bi) + text_vocab;
}
extern "C" int dmi_assemble_tokens(const int32_t* text, const float* vae_logits, int32_t* tokens_out, int B, int T,
                                   int P, int C, int text_vocab, void* stream) {
  DMI_REQUIRE(text && vae_logits && tokens_out && B > 0 && T >= 0 && P > 0 && C > 0, "assemble_tokens: bad args");
  const int64_t n = (int64_t)B * (T + P);
  assemble_tokens_kernel<<<dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, (hipStream_t)stream>>>(text, vae_logits, tokens_out, B, T, P, C, text_vocab);
  DMI_CHECK_LAUNCH("assemble_tokens");
  return DMI_OK;
}

// =====================================================================================
// K7 cross entropy over bf16 logits (models.py:348-359; mtf softmax_cross_entropy_with_logits A.5)
// one 256-thread block per row; pass 1 online max/sum; pass 2 (L2-resident re-read) writes dz in place.
// =====================================================================================
// General path: 256 threads per row, two passes (second pass re-reads the row through the caches).
__global__ __launch_bounds__(256) void cross_entropy_kernel(bf16_t* __restrict__ z, int ldz,
                                                            const int* __restrict__ labels,
                                                            float* __restrict__ loss_rows, float* __restrict__ lse_out,
                                                            int V, float dz_scale) {
  __shared__ float sm_m[4], sm_s[4];
  const int64_t row = blockIdx.x;
  bf16_t* zr = z + row * ldz;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nch = (V + 7) / 8;
  float m = -INFINITY, s = 0.f;
  for (int c = tid; c < nch; c += 256) {
    float f[8];
    unpack8(*(const u32x4*)(zr + c * 8), f);
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c * 8 + j >= V) f[j] = -INFINITY;
      cm = fmaxf(cm, f[j]);
    }
    if (cm > m) {
      s *= __expf(m - cm);
      m = cm;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s += __expf(f[j] - m);
  }
  float wm = wave_max(m);
  s *= (m == -INFINITY) ? 0.f : __expf(m - wm);
  s = wave_sum(s);
  if (lane == 0) {
    sm_m[wid] = wm;
    sm_s[wid] = s;
  }
  __syncthreads();
  const float bm = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
  float bs = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) bs += sm_s[w] * __expf(sm_m[w] - bm);
  const float lse = bm + __logf(bs);
  const int label = labels[row];
  if (tid == 0) {
    const float zl = (label >= 0 && label < V) ? bf2f(zr[label]) : 0.f;
    loss_rows[row] = lse - zl;
    if (lse_out) lse_out[row] = lse;
  }
  if (dz_scale == 0.f) return;
  __syncthreads();  // tid 0 read z[label] before anyone overwrites it
  for (int c = tid; c < ldz / 8; c += 256) {  // every column of the row incl. the pad: dz[pad] = 0
    float f[8];
    unpack8(*(const u32x4*)(zr + c * 8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c * 8 + j;
      float p = (col < V) ? __expf(f[j] - lse) : 0.f;
      if (col == label) p -= 1.f;
      f[j] = p * dz_scale;
    }
    *(u32x4*)(zr + c * 8) = pack8(f);
  }
}

// Large-vocabulary path: 1024 threads per row, the row (<= NC*1024 chunks of 16 B) stays in registers between the
// statistics pass and the dlogits pass: one HBM read + one HBM write per element.
template <int NC>
__global__ __launch_bounds__(1024) void cross_entropy_reg_kernel(bf16_t* __restrict__ z, int ldz,
                                                                 const int* __restrict__ labels,
                                                                 float* __restrict__ loss_rows, float* __restrict__ lse_out,
                                                                 int V, float dz_scale) {
  __shared__ float sm_m[16], sm_s[16];
  const int64_t row = blockIdx.x;
  bf16_t* zr = z + row * ldz;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nch = ldz / 8;
  // the row lives in registers as fp32 (NC x 8 per thread); each element costs one unpack, one max, one fma + v_exp
  // (kept: the probabilities are exp(x - max) * (scale / sum), no second exp), one mul and half a pack.  Columns >= V
  // are set to -inf once at load time so no later pass carries a mask.
  float f[NC][8];
  float m = -INFINITY;
  {
    u32x4 raw[NC];  // all loads in flight before the first use
    const u32x4 ninf = {0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = tid + 1024 * i;
      raw[i] = (c < nch) ? *(const u32x4*)(zr + c * 8) : ninf;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = tid + 1024 * i;
      unpack8(raw[i], f[i]);
      if (c * 8 + 8 > V) {  // only the chunk straddling V (and pad chunks); the empty asm keeps this a real branch
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < 8; ++j) f[i][j] = (c * 8 + j < V) ? f[i][j] : -INFINITY;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, f[i][j]);
    }
  }
  m = wave_max(m);
  if (lane == 0) sm_m[wid] = m;
  __syncthreads();
  float bm = sm_m[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) bm = fmaxf(bm, sm_m[w]);
  constexpr float LOG2E = 1.4426950408889634f;
  const float bm2 = bm * LOG2E;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[i][j] = __builtin_amdgcn_exp2f(__builtin_fmaf(f[i][j], LOG2E, -bm2));
      s += f[i][j];
    }
  s = wave_sum(s);
  if (lane == 0) sm_s[wid] = s;
  __syncthreads();
  float bs = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) bs += sm_s[w];
  const float lse = bm + __logf(bs);
  const int label = labels[row];
  if (tid == 0) {
    const float zl = (label >= 0 && label < V) ? bf2f(zr[label]) : 0.f;  // row not overwritten yet (barrier below)
    loss_rows[row] = lse - zl;
    if (lse_out) lse_out[row] = lse;
  }
  if (dz_scale == 0.f) return;
  __syncthreads();
  const float k = dz_scale / bs;
  const int lch = (label >= 0 && label < V) ? (label >> 3) : -1, lj = label & 7;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = tid + 1024 * i;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] *= k;
      if (c == lch) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < 8; ++j) f[i][j] -= (j == lj) ? dz_scale : 0.f;
      }
      *(u32x4*)(zr + c * 8) = pack8(f[i]);
    }
  }
}

extern "C" int dmi_cross_entropy(uint16_t* z, int ldz, const int32_t* labels, float* loss_rows, float* lse,
                                 int64_t M, int V, float dz_scale, void* stream) {
  DMI_REQUIRE(z && labels && loss_rows, "cross_entropy: null pointer");
  DMI_REQUIRE(ldz % 8 == 0 && ldz >= ((V + 7) / 8) * 8 && M > 0 && V > 0, "cross_entropy: ldz must be a multiple of 8 and >= round_up(V,8)");
  hipStream_t st = (hipStream_t)stream;
  const int nch = ldz / 8;
  if (nch > 2048 && nch <= 8 * 1024) {
    if (nch <= 4 * 1024) cross_entropy_reg_kernel<4><<<dim3((unsigned)M), dim3(1024), 0, st>>>(z, ldz, labels, loss_rows, lse, V, dz_scale);
    else if (nch <= 7 * 1024) cross_entropy_reg_kernel<7><<<dim3((unsigned)M), dim3(1024), 0, st>>>(z, ldz, labels, loss_rows, lse, V, dz_scale);
    else cross_entropy_reg_kernel<8><<<dim3((unsigned)M), dim3(1024), 0, st>>>(z, ldz, labels, loss_rows, lse, V, dz_scale);
  } else {
    cross_entropy_kernel<<<dim3((unsigned)M), dim3(256), 0, st>>>(z, ldz, labels, loss_rows, lse, V, dz_scale);
  }
  DMI_CHECK_LAUNCH("cross_entropy");
  return DMI_OK;
}

// =====================================================================================
// Fused softmax head (training path): the cross entropy of models.py:348-359 without a logits round trip.
//   dmi_label_logit      zl[m] = x[m,:] . Wt[label[m],:] + bias[label[m]]        (fp32; also the per-row shift of the exponent)
//   dmi_gemm_nt_softmax  E[m,v] = bf16(exp(logit[m,v] - zl[m])) + partial row sums  (gemm.hip)
//   dmi_softmax_finish   S[m] = sum_v exp(.) ;  loss_row[m] = log S[m] + shift[m] - zl[m]  (= logsumexp - label logit, exactly the
//                        reference's loss_batch);  rowscale[m] = dz_scale / S[m];  E[m,label] -= S[m]  (so that dlogits = rowscale * E);
//                        Xs[m,:] = bf16(rowscale[m] * x[m,:])  (the weight-gradient GEMM's left operand: dW = Xs^T E)
// No shift (the engine's choice): exp(logit) is exact to rounding for logits within +-87 -- floating point keeps its relative
// precision, the row maximum is not needed.  A row whose sum leaves [1e-18, 1e18] (some logit > 41, or all < -41 - ln V) is flagged and
// redone exactly by softmax_fixup_kernel with the row maximum as the shift.  With the label logit as shift (rowshift = zl) the
// label entry is 1 and only a logit exceeding the label's by > 88 (a row loss > 88 nats) takes the fix-up path.
// =====================================================================================
__global__ __launch_bounds__(256) void label_logit_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ Wt,
                                                          int ldw, const bf16_t* __restrict__ bias, const int* __restrict__ labels,
                                                          float* __restrict__ zl, int* __restrict__ flag, int64_t M, int K, int V) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) flag[0] = 0;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= M) return;
  int lab = labels[row];
  lab = lab < 0 ? 0 : (lab >= V ? V - 1 : lab);
  const bf16_t* xr = X + row * ldx;
  const bf16_t* wr = Wt + (int64_t)lab * ldw;
  float acc = 0.f;
  for (int c = lane; c < K / 8; c += 64) {
    float a[8], b[8];
    unpack8(*(const u32x4*)(xr + c * 8), a);
    unpack8(*(const u32x4*)(wr + c * 8), b);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(a[j], b[j], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) zl[row] = acc + bf2f(bias[lab]);
}
extern "C" int dmi_label_logit(const uint16_t* X, int ldx, const uint16_t* Wt, int ldw, const uint16_t* bias,
                               const int32_t* labels, float* zl, int32_t* flag, int64_t M, int K, int V, void* stream) {
  DMI_REQUIRE(X && Wt && bias && labels && zl && flag, "label_logit: null pointer");
  DMI_REQUIRE(M > 0 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && V > 0, "label_logit: bad sizes");
  label_logit_kernel<<<dim3((unsigned)cdiv64(M, 4)), dim3(256), 0, (hipStream_t)stream>>>(X, ldx, Wt, ldw, bias, labels, zl, flag, M, K, V);
  DMI_CHECK_LAUNCH("label_logit");
  return DMI_OK;
}

struct SoftmaxFinishArgs {
  const float* part; int nparts;
  const float* zl;        // label logits (dmi_label_logit)
  const float* rowshift;  // nullable: the shift the GEMM epilogue subtracted in the exponent
  const int* labels;
  const bf16_t* X; int ldx;
  bf16_t* E; int lde;
  float* loss_rows; float* rowscale; bf16_t* rowscale_bf16; bf16_t* Xs;
  int* flag;
  int64_t M; int K, V;
  float dz_scale;
};
#define SF_ROWS 64
#define SF_PARTS 16
// PW = PosWeight (dmi_softmax_finish_w): row m carries the static loss weight w[m % period] in its gradient scale,
// rowscale[m] = (dz_scale * w) / S[m]; loss_rows, the label patch of E and the flag logic never see the weight.  PW = NoWeight is an
// empty argument: that instance's kernel arguments and instructions are those of the untemplated kernel.
struct NoWeight { static constexpr bool on = false; };
struct PosWeight { static constexpr bool on = true; const float* w; int period; };
template <class PW>
__global__ __launch_bounds__(256) void softmax_finish_kernel(SoftmaxFinishArgs a, PW pw) {
  // 64 rows per block, the partials of a row summed by 16 threads (p = q mod 16) with 16-byte loads of 4 adjacent rows: 640
  // blocks x 4 waves for the dalle_example batch (the 160-block version left 2.5 waves per CU and ran latency-bound)
  __shared__ float sm[SF_PARTS][SF_ROWS];
  __shared__ float sc[SF_ROWS];
  const int tid = threadIdx.x, r4 = tid & 15, q = tid >> 4;   // thread: rows 4 r4 .. 4 r4 + 3, partials p = q (mod 16)
  const int64_t m0 = (int64_t)blockIdx.x * SF_ROWS, m = m0 + 4 * r4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (m + 3 < a.M && (a.M & 3) == 0) {
    for (int p = q; p < a.nparts; p += SF_PARTS) {   // fixed order: deterministic
      const f32x4 v = *(const f32x4*)(a.part + (int64_t)p * a.M + m);
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
  } else {
    for (int j = 0; j < 4; ++j)
      if (m + j < a.M)
        for (int p = q; p < a.nparts; p += SF_PARTS) s[j] += a.part[(int64_t)p * a.M + m + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sm[q][4 * r4 + j] = s[j];
  __syncthreads();
  if (tid < SF_ROWS) {
    const int r = tid;
    const int64_t mr = m0 + r;
    float scale = 0.f;
    if (mr < a.M) {
      float S = 0.f;
#pragma unroll
      for (int k = 0; k < SF_PARTS; ++k) S += sm[k][r];
      // accept window [1e-18, 1e18] (|logsumexp| <= 41): inf / nan (an exponent overflowed) and vanished rows fall outside, and
      // so do rows that are merely LARGE -- for S ~ 1e33..3e38 rowscale = dz_scale / S would be an fp32/bf16 denormal (Xs and
      // rowscale_bf16 flush to 0: a silently dropped row) and the E.W^T accumulators of the input gradient could overflow.
      // Inside the window rowscale >= 1e-18 * dz_scale and E <= 1e18 keep > 60 binades of headroom; outside, the exact fix-up.
      const bool bad = !(S > 1.0e-18f && S < 1.0e18f);
      if (bad) a.flag[0] = 1;
      // loss = logsumexp - label logit = log S + shift - zl   (models.py:348-359: the reference's loss_batch)
      a.loss_rows[mr] = bad ? INFINITY : __logf(S) + (a.rowshift ? a.rowshift[mr] : 0.f) - a.zl[mr];
      float dz = a.dz_scale;
      if constexpr (PW::on) dz *= pw.w[(int)(((int64_t)(m0 % pw.period) + r) % pw.period)];   // the product first, then the division
      scale = bad ? 0.f : dz / S;
      if (a.dz_scale != 0.f) {
        a.rowscale[mr] = scale;
        a.rowscale_bf16[mr] = f2bf(scale);
        int lab = a.labels[mr];
        lab = lab < 0 ? 0 : (lab >= a.V ? a.V - 1 : lab);
        bf16_t* el = a.E + mr * a.lde + lab;
        *el = f2bf(bf2f(*el) - S);   // dlogits[m, label] = rowscale * (e_label - S) = dz_scale * (p_label - 1)
      }
    }
    sc[r] = scale;
  }
  __syncthreads();
  if (a.dz_scale == 0.f) return;
  const int cpr = a.K / 8;
  for (int idx = tid; idx < SF_ROWS * cpr; idx += 256) {
    const int rr = idx / cpr, ch = idx - rr * cpr;
    const int64_t mm = m0 + rr;
    if (mm >= a.M) break;
    float f[8];
    unpack8(*(const u32x4*)(a.X + mm * a.ldx + ch * 8), f);
    const float k = sc[rr];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= k;
    *(u32x4*)(a.Xs + mm * a.K + ch * 8) = pack8(f);
  }
}
// Exact redo of the flagged rows (loss_rows[m] == inf): logits recomputed from x and Wt with the row maximum as the shift.
#define FIX_MAXK 8192
template <class PW>
__global__ __launch_bounds__(256) void softmax_fixup_kernel(SoftmaxFinishArgs a, const bf16_t* __restrict__ Wt, int ldw,
                                                            const bf16_t* __restrict__ bias, int N, PW pw) {
  if (a.flag[0] == 0) return;
  __shared__ float xs[FIX_MAXK];
  __shared__ float red[4];
  __shared__ float zlab;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int64_t m = blockIdx.x; m < a.M; m += gridDim.x) {
    if (a.loss_rows[m] < 3.0e38f) continue;   // block-uniform
    __syncthreads();
    for (int k = tid; k < a.K; k += 256) xs[k] = bf2f(a.X[m * a.ldx + k]);
    int lab = a.labels[m];
    lab = lab < 0 ? 0 : (lab >= a.V ? a.V - 1 : lab);
    __syncthreads();
    auto logit = [&](int v) {
      const bf16_t* wr = Wt + (int64_t)v * ldw;
      float acc = 0.f;
      for (int c = lane; c < a.K / 8; c += 64) {
        float b[8];
        unpack8(*(const u32x4*)(wr + c * 8), b);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(xs[c * 8 + j], b[j], acc);
      }
      return wave_sum(acc) + bf2f(bias[v]);
    };
    float mx = -INFINITY;
    for (int v = wid; v < a.V; v += 4) {
      const float z = logit(v);
      mx = fmaxf(mx, z);
      if (v == lab && lane == 0) zlab = z;
    }
    if (lane == 0) red[wid] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float zl = zlab;
    __syncthreads();
    float sum = 0.f;
    for (int v = wid; v < N; v += 4) {
      const float e = (v < a.V) ? __expf(logit(v) - mx) : 0.f;
      sum += e;
      if (lane == 0) a.E[m * a.lde + v] = f2bf(e);
    }
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    const float S = ((red[0] + red[1]) + red[2]) + red[3];
    float dz = a.dz_scale;
    if constexpr (PW::on) dz *= pw.w[(int)(m % pw.period)];   // a redone row keeps its weight (same arithmetic as softmax_finish_kernel)
    const float scale = dz / S;
    __syncthreads();   // E row complete (block scope) before the label entry is patched
    if (tid == 0) {
      a.loss_rows[m] = mx + __logf(S) - zl;
      if (a.dz_scale != 0.f) {
        a.rowscale[m] = scale;
        a.rowscale_bf16[m] = f2bf(scale);
        a.E[m * a.lde + lab] = f2bf(__expf(zl - mx) - S);
      }
    }
    if (a.dz_scale != 0.f)
      for (int k = tid * 8; k < a.K; k += 256 * 8) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = xs[k + j] * scale;
        *(u32x4*)(a.Xs + m * a.K + k) = pack8(f);
      }
  }
}
// pos_weight == nullptr: the unweighted entry point
static int softmax_finish_launch(const float* rowsum_part, int nparts, const float* label_logit, const float* rowshift,
                                 const int32_t* labels, const uint16_t* X, int ldx,
                                 const uint16_t* Wt, int ldw, const uint16_t* bias, uint16_t* E, int lde, int N,
                                 float* loss_rows, float* rowscale, uint16_t* rowscale_bf16, uint16_t* Xs, int32_t* flag,
                                 int64_t M, int K, int V, float dz_scale, const float* pos_weight, int period, void* stream) {
  DMI_REQUIRE(rowsum_part && label_logit && labels && X && Wt && bias && E && loss_rows && flag, "softmax_finish: null pointer");
  DMI_REQUIRE(dz_scale == 0.f || (rowscale && rowscale_bf16 && Xs), "softmax_finish: gradient outputs missing");
  DMI_REQUIRE(M > 0 && K % 8 == 0 && K <= FIX_MAXK && ldx % 8 == 0 && ldw % 8 == 0 && nparts > 0 && V > 0 && V <= N && N <= lde,
              "softmax_finish: bad sizes (K <= %d)", FIX_MAXK);
  SoftmaxFinishArgs a;
  a.part = rowsum_part; a.nparts = nparts; a.zl = label_logit; a.rowshift = rowshift; a.labels = labels; a.X = X; a.ldx = ldx; a.E = E; a.lde = lde;
  a.loss_rows = loss_rows; a.rowscale = rowscale; a.rowscale_bf16 = rowscale_bf16; a.Xs = Xs; a.flag = flag;
  a.M = M; a.K = K; a.V = V; a.dz_scale = dz_scale;
  hipStream_t st = (hipStream_t)stream;
  const PosWeight pw{pos_weight, period};
  if (pos_weight) softmax_finish_kernel<<<dim3((unsigned)cdiv64(M, SF_ROWS)), dim3(256), 0, st>>>(a, pw);
  else softmax_finish_kernel<<<dim3((unsigned)cdiv64(M, SF_ROWS)), dim3(256), 0, st>>>(a, NoWeight{});
  DMI_CHECK_LAUNCH("softmax_finish");
  // returns at once unless a row was flagged
  if (pos_weight) softmax_fixup_kernel<<<dim3(256), dim3(256), 0, st>>>(a, Wt, ldw, bias, N, pw);
  else softmax_fixup_kernel<<<dim3(256), dim3(256), 0, st>>>(a, Wt, ldw, bias, N, NoWeight{});
  DMI_CHECK_LAUNCH("softmax_fixup");
  return DMI_OK;
}
extern "C" int dmi_softmax_finish(const float* rowsum_part, int nparts, const float* label_logit, const float* rowshift,
                                  const int32_t* labels, const uint16_t* X, int ldx,
                                  const uint16_t* Wt, int ldw, const uint16_t* bias, uint16_t* E, int lde, int N,
                                  float* loss_rows, float* rowscale, uint16_t* rowscale_bf16, uint16_t* Xs, int32_t* flag,
                                  int64_t M, int K, int V, float dz_scale, void* stream) {
  return softmax_finish_launch(rowsum_part, nparts, label_logit, rowshift, labels, X, ldx, Wt, ldw, bias, E, lde, N, loss_rows, rowscale,
                               rowscale_bf16, Xs, flag, M, K, V, dz_scale, nullptr, 0, stream);
}
// Text/image loss weights (a project extension; the reference's loss is the plain mean, models.py:348-359): see the kernels above.
extern "C" int dmi_softmax_finish_w(const float* rowsum_part, int nparts, const float* label_logit, const float* rowshift,
                                    const int32_t* labels, const uint16_t* X, int ldx,
                                    const uint16_t* Wt, int ldw, const uint16_t* bias, uint16_t* E, int lde, int N,
                                    float* loss_rows, float* rowscale, uint16_t* rowscale_bf16, uint16_t* Xs, int32_t* flag,
                                    int64_t M, int K, int V, float dz_scale, const float* pos_weight, int period, void* stream) {
  DMI_REQUIRE(pos_weight, "softmax_finish_w: null pos_weight");
  DMI_REQUIRE(period > 0, "softmax_finish_w: period must be > 0");
  return softmax_finish_launch(rowsum_part, nparts, label_logit, rowshift, labels, X, ldx, Wt, ldw, bias, E, lde, N, loss_rows, rowscale,
                               rowscale_bf16, Xs, flag, M, K, V, dz_scale, pos_weight, period, stream);
}

// =====================================================================================
// reductions + optimizer (src/optimizers.py:11-16, 82-89, 154-177)
// =====================================================================================
__device__ __forceinline__ float block_sum_256(float x, float* sm) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// one block, 1024 threads, four independent float4 chains per thread (fixed order -> deterministic)
__global__ __launch_bounds__(1024) void sum_f32_kernel(const float* __restrict__ x, int64_t n, float scale,
                                                       float* __restrict__ out) {
  __shared__ float sm[16];
  const int tid = threadIdx.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if ((((uintptr_t)x) & 15) == 0) {
    const int64_t n4 = n / 4;
    const f32x4* x4 = (const f32x4*)x;
    int64_t i = tid;
    for (; i + 3072 < n4; i += 4096) {
      const f32x4 v0 = x4[i], v1 = x4[i + 1024], v2 = x4[i + 2048], v3 = x4[i + 3072];
      a0 += (v0[0] + v0[1]) + (v0[2] + v0[3]);
      a1 += (v1[0] + v1[1]) + (v1[2] + v1[3]);
      a2 += (v2[0] + v2[1]) + (v2[2] + v2[3]);
      a3 += (v3[0] + v3[1]) + (v3[2] + v3[3]);
    }
    for (; i < n4; i += 1024) {
      const f32x4 v0 = x4[i];
      a0 += (v0[0] + v0[1]) + (v0[2] + v0[3]);
    }
    if (tid < (n & 3)) a1 += x[n4 * 4 + tid];
  } else {
    for (int64_t i = tid; i < n; i += 1024) a0 += x[i];
  }
  float t = wave_sum((a0 + a1) + (a2 + a3));
  if ((tid & 63) == 0) sm[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) {
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) r += sm[w];
    out[0] = r * scale;
  }
}
extern "C" int dmi_sum_f32(const float* x, int64_t n, float scale, float* out, void* stream) {
  DMI_REQUIRE(x && out && n > 0, "sum_f32: bad args");
  sum_f32_kernel<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(x, n, scale, out);
  DMI_CHECK_LAUNCH("sum_f32");
  return DMI_OK;
}

// The weighted loss and its two per-modality means from the per-row losses, one block (fixed order -> deterministic, no atomics):
//   out3[0] = scale * sum_m w[m % period] * loss_rows[m];  out3[1] = mean over rows with m % period < split (text positions),
//   out3[2] = mean over the others (image positions); a mean over no rows is 0.
// Thread t owns rows t, t + 1024, ...; its position advances by 1024 mod period, so the loop has no division.
__global__ __launch_bounds__(1024) void loss_reduce_kernel(const float* __restrict__ loss_rows, int64_t M,
                                                           const float* __restrict__ pos_weight, int period, int split,
                                                           float scale, float inv_text, float inv_image, float* __restrict__ out3) {
  __shared__ float sm[3][16];
  const int tid = threadIdx.x;
  const int step = 1024 % period;
  int pos = tid % period;
  float aw = 0.f, at = 0.f, ai = 0.f;
  for (int64_t m = tid; m < M; m += 1024) {
    const float l = loss_rows[m];
    aw = __builtin_fmaf(pos_weight[pos], l, aw);
    if (pos < split) at += l; else ai += l;
    pos += step;
    if (pos >= period) pos -= period;
  }
  aw = wave_sum(aw); at = wave_sum(at); ai = wave_sum(ai);
  if ((tid & 63) == 0) { sm[0][tid >> 6] = aw; sm[1][tid >> 6] = at; sm[2][tid >> 6] = ai; }
  __syncthreads();
  if (tid < 3) {
    const float* s = sm[tid];
    const float r = (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) +
                    (((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15])));
    out3[tid] = r * (tid == 0 ? scale : tid == 1 ? inv_text : inv_image);
  }
}
extern "C" int dmi_loss_reduce(const float* loss_rows, int64_t M, const float* pos_weight, int period, int split, float scale,
                               float* out3, void* stream) {
  DMI_REQUIRE(loss_rows && pos_weight && out3, "loss_reduce: null pointer");
  DMI_REQUIRE(M > 0 && period > 0 && split >= 0 && split <= period, "loss_reduce: bad sizes (M > 0, period > 0, 0 <= split <= period)");
  const int64_t full = M / period, rem = M % period;
  const int64_t ntext = full * split + (rem < split ? rem : split), nimage = M - ntext;
  loss_reduce_kernel<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(loss_rows, M, pos_weight, period, split, scale,
                                                                      ntext ? (float)(1.0 / (double)ntext) : 0.f,
                                                                      nimage ? (float)(1.0 / (double)nimage) : 0.f, out3);
  DMI_CHECK_LAUNCH("loss_reduce");
  return DMI_OK;
}

// Padded caption positions ("loss_ignore_padding", a project extension): the weight of a row depends on its label.  Row m is a text
// row when m % period < split; a text row whose label is pad_id is ignored (keep = 0), every other row is kept.
//   counts[0] = n_t = the kept text rows, counts[1] = n_i = the image rows (exact, int32);
//   plain:    row_w[m] = keep / (n_t + n_i);   else: keep * ct / max(n_t, 1) on text rows, ci / n_i on image rows
// (the numerator in fp32, one correctly rounded division by the count converted to float; an ignored row is exactly 0).
// One block: every thread counts its rows m = t, t + 1024, ... (position advanced without a division, as in loss_reduce_kernel),
// the block adds the integer counts -- any order gives the same integers --, then every thread writes its rows.
__device__ __forceinline__ int wave_sum_i32(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__global__ __launch_bounds__(1024) void loss_mask_kernel(const int* __restrict__ labels, int64_t M, int period, int split, int pad_id,
                                                         float ct, float ci, int plain, int* __restrict__ counts,
                                                         float* __restrict__ row_w) {
  __shared__ int sm[2][16];
  const int tid = threadIdx.x;
  const int step = 1024 % period, pos0 = tid % period;
  int pos = pos0, nt = 0, ni = 0;
  for (int64_t m = tid; m < M; m += 1024) {
    if (pos < split) nt += labels[m] != pad_id; else ++ni;
    pos += step;
    if (pos >= period) pos -= period;
  }
  nt = wave_sum_i32(nt); ni = wave_sum_i32(ni);
  if ((tid & 63) == 0) { sm[0][tid >> 6] = nt; sm[1][tid >> 6] = ni; }
  __syncthreads();
  nt = ni = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { nt += sm[0][w]; ni += sm[1][w]; }
  if (tid == 0) { counts[0] = nt; counts[1] = ni; }
  const float wt = plain ? 1.f / (float)(nt + ni > 1 ? nt + ni : 1) : ct / (float)(nt > 1 ? nt : 1);
  const float wi = plain ? wt : (ni ? ci / (float)ni : 0.f);
  pos = pos0;
  for (int64_t m = tid; m < M; m += 1024) {
    row_w[m] = pos < split ? (labels[m] != pad_id ? wt : 0.f) : wi;
    pos += step;
    if (pos >= period) pos -= period;
  }
}
extern "C" int dmi_loss_mask(const int32_t* labels, int64_t M, int period, int split, int pad_id, float ct, float ci, int plain,
                             int32_t* counts, float* row_w, void* stream) {
  DMI_REQUIRE(labels && counts && row_w, "loss_mask: null pointer");
  DMI_REQUIRE(M > 0 && M < (1ll << 31), "loss_mask: M must lie in [1, 2^31) (the counts are int32)");
  DMI_REQUIRE(period > 0 && split >= 0 && split <= period, "loss_mask: bad sizes (period > 0, 0 <= split <= period: period=%d split=%d)",
              period, split);
  loss_mask_kernel<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(labels, M, period, split, pad_id, ct, ci, plain, counts, row_w);
  DMI_CHECK_LAUNCH("loss_mask");
  return DMI_OK;
}

// The masked loss and what is reported beside it, on loss_reduce_kernel's tree (one block, fixed order, no atomics):
//   out4[0] = scale * sum_m row_w[m] * loss_rows[m];  out4[1] = L_t = sum over kept text rows / max(n_t, 1);
//   out4[2] = L_i = mean over the image rows;  out4[3] = n_t / the number of text rows;  a mean over no rows is 0.
// n_t = counts[0] and n_i = counts[1] are dmi_loss_mask's (read from the device: no host sync).
__global__ __launch_bounds__(1024) void loss_reduce_masked_kernel(const float* __restrict__ loss_rows, const float* __restrict__ row_w,
                                                                  const int* __restrict__ labels, int64_t M, int period, int split,
                                                                  int pad_id, const int* __restrict__ counts, float scale,
                                                                  float ntext, float* __restrict__ out4) {
  __shared__ float sm[3][16];
  const int tid = threadIdx.x;
  const int step = 1024 % period;
  int pos = tid % period;
  float aw = 0.f, at = 0.f, ai = 0.f;
  for (int64_t m = tid; m < M; m += 1024) {
    const float l = loss_rows[m];
    aw = __builtin_fmaf(row_w[m], l, aw);
    if (pos < split) at += labels[m] != pad_id ? l : 0.f; else ai += l;
    pos += step;
    if (pos >= period) pos -= period;
  }
  aw = wave_sum(aw); at = wave_sum(at); ai = wave_sum(ai);
  if ((tid & 63) == 0) { sm[0][tid >> 6] = aw; sm[1][tid >> 6] = at; sm[2][tid >> 6] = ai; }
  __syncthreads();
  if (tid < 3) {
    const float* s = sm[tid];
    const float r = (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) +
                    (((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15])));
    const int n = counts[tid == 1 ? 0 : 1];
    out4[tid] = tid == 0 ? r * scale : (n > 0 ? r / (float)n : 0.f);
  } else if (tid == 3) {
    out4[3] = ntext > 0.f ? (float)counts[0] / ntext : 0.f;
  }
}
extern "C" int dmi_loss_reduce_masked(const float* loss_rows, const float* row_w, const int32_t* labels, int64_t M, int period,
                                      int split, int pad_id, const int32_t* counts, float scale, float* out4, void* stream) {
  DMI_REQUIRE(loss_rows && row_w && labels && counts && out4, "loss_reduce_masked: null pointer");
  DMI_REQUIRE(M > 0 && M < (1ll << 31) && period > 0 && split >= 0 && split <= period,
              "loss_reduce_masked: bad sizes (0 < M < 2^31, period > 0, 0 <= split <= period)");
  const int64_t full = M / period, rem = M % period;
  const int64_t ntext = full * split + (rem < split ? rem : split);
  loss_reduce_masked_kernel<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(loss_rows, row_w, labels, M, period, split, pad_id, counts,
                                                                             scale, (float)ntext, out4);
  DMI_CHECK_LAUNCH("loss_reduce_masked");
  return DMI_OK;
}

#define SUMSQ_BLOCKS 2048
extern "C" int64_t dmi_sumsq_workspace_bytes(int64_t n) { (void)n; return SUMSQ_BLOCKS * 4; }
// (A sweep from the END of the buffer -- the flat gradient buffer is laid out in backward's completion order, so its tail is what the 256-MB
// Infinity Cache should still hold at clip time -- measured -0.03 ms per step on one box over three alternations, 0.00 on another over four,
// and slightly slower with Adam behind it in isolation: neutral, not kept.  profiles/r06_ab_sumsq_rev.log)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  __shared__ float sm[4];
  float acc = 0.f;
  const int64_t n4 = n / 4;
  const f32x4* g4 = (const f32x4*)g;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = g4[i];
    acc += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = g[n4 * 4 + threadIdx.x];
    acc += v * v;
  }
  const float t = block_sum_256(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
extern "C" int dmi_sumsq(const float* g, int64_t n, float* out, void* workspace, void* stream) {
  DMI_REQUIRE(g && out && workspace && n > 0, "sumsq: bad args");
  DMI_REQUIRE(((uintptr_t)g & 15) == 0, "sumsq: g must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  sumsq_kernel<<<dim3(SUMSQ_BLOCKS), dim3(256), 0, st>>>(g, n, (float*)workspace);
  DMI_CHECK_LAUNCH("sumsq");
  sum_f32_kernel<<<dim3(1), dim3(1024), 0, st>>>((const float*)workspace, SUMSQ_BLOCKS, 1.0f, out);
  DMI_CHECK_LAUNCH("sumsq_finish");
  return DMI_OK;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16_t* __restrict__ pb, int64_t n,
                                                   const float* __restrict__ gnorm_sq, float clip, float lr, float b1,
                                                   float b2, float eps, float wd, float gscale,
                                                   const float* __restrict__ lr_dev) {
  if (lr_dev) lr = lr_dev[0];   // graph replay: the scheduled learning rate lives in device memory
  float mult = gscale;
  if (gnorm_sq != nullptr && clip > 0.f) {
    const float gn = sqrtf(gnorm_sq[0]) * gscale;  // norm of the scaled gradient
    mult = gscale * (clip / fmaxf(gn, clip));
  }
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = gv[j] * mult;
      mv[j] = b1 * mv[j] + (1.f - b1) * gg;
      vv[j] = b2 * vv[j] + (1.f - b2) * gg * gg;
      float upd = mv[j] / (sqrtf(vv[j]) + eps);
      upd += wd * pv[j];
      pv[j] -= lr * upd;
    }
    ((f32x4*)p)[i] = pv;
    ((f32x4*)m)[i] = mv;
    ((f32x4*)v)[i] = vv;
    if (pb) *(u32x2*)(pb + i * 4) = u32x2{pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    const float gg = g[i] * mult;
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    float pp = p[i];
    pp -= lr * (mm / (sqrtf(vv) + eps) + wd * pp);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
    if (pb) pb[i] = f2bf(pp);
  }
}
extern "C" int dmi_adam_step(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n,
                             const float* gnorm_sq, float clip, float lr, float beta1, float beta2, float eps,
                             float weight_decay, float grad_scale, const float* lr_dev, void* stream) {
  DMI_REQUIRE(p && g && m && v && n > 0, "adam_step: bad args");
  DMI_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && (((uintptr_t)p_bf16) & 7) == 0,
              "adam_step: buffers must be 16-byte aligned");
  int64_t blocks = cdiv64(n / 4 + 1, 256);
  if (blocks > 4096) blocks = 4096;
  adam_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(p, g, m, v, p_bf16, n, gnorm_sq, clip, lr, beta1, beta2, eps, weight_decay, grad_scale, lr_dev);
  DMI_CHECK_LAUNCH("adam_step");
  return DMI_OK;
}

__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = f2bf(in[i]);
}
extern "C" int dmi_cast_f32_bf16(const float* in, uint16_t* out, int64_t n, void* stream) {
  DMI_REQUIRE(in && out && n > 0, "cast: bad args");
  int64_t blocks = cdiv64(n, 256);
  if (blocks > 8192) blocks = 8192;
  cast_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(in, out, n);
  DMI_CHECK_LAUNCH("cast");
  return DMI_OK;
}

// =====================================================================================
// sampling of the next image token from one row of head logits
// =====================================================================================
// The reference stops at the logits (predict raises NotImplementedError, src/model_fns.py:135-136); the sampler around the
// incremental-inference hooks (src/dalle_mtf/models.py:246-254,281-285) is this repo's.  ONE draw body, draw_tokens<NUCLEUS, GUIDED>,
// and three kernels over it: sample_tokens_kernel <false, false>, sample_tokens_p_kernel <true, false> and
// sample_tokens_guided_kernel <true, true>.  One block per row (GUIDED: per pair of rows):
//   v[i] = (z[b, i] + bias[i]) * (1/temperature);  top-k filter: keep v[i] >= (k-th largest v)  (ties kept, as a masked_fill of
//   v < kth would);  choice ~ softmax(v) over the kept entries, drawn as argmax_i (v[i] + Gumbel noise) -- the Gumbel-max form of
//   the same categorical draw -- with counter-based noise hash(seed, position, b, i): reproducible, no RNG state.  The uniform
//   takes 23 random bits so that the + 0.5 is exact in fp32: u in [2^-24, 1 - 2^-24], strictly inside (0, 1) -- with 24 bits
//   16777215.5 rounds to 2^24, u == 1 and the noise -log(-log u) is +inf (the entry then wins regardless of its logit).
//   temperature <= 0: greedy (first maximum), top_k and top_p ignored.
// The k-th largest value is found without a sort: 32 steps of a bitwise binary search on order-preserving integer keys
// (count(key >= candidate) >= k), a block-wide count per step.
// NUCLEUS adds the top-p filter after the top-k one, and the row's log-likelihood:
//   q = softmax(v) over the top-k survivors, quantised: u[i] = floor(exp(v[i] - max v) * 2^31) (the maximum has u = 2^31), the
//   mass of a set is the 64-bit integer sum of its u, the whole survivor set has mass Z, and the target is
//   ceil(double(top_p) * double(Z)) (one IEEE double product: a numpy restatement reproduces it bit for bit);
//   tau = the largest u-candidate with mass(u >= tau) >= target, found by the same 32-step bitwise search as the k-th value (the
//   predicate "mass of entries with u >= candidate >= target") -- tau is the u of the last entry of the shortest descending prefix
//   that reaches top_p, and EVERY survivor with u >= tau is kept (ties at tau kept, as for top-k).  No sort; the kept set does not
//   depend on summation order.  Entries with u = 0 (q < 2^-31) are never in a nucleus with top_p < 1;
//   top_p >= 1 (or not in (0, 1), or a row whose maximum is not finite) skips the nucleus step: the kept set is the top-k set and
//   the choice is the plain instance's, bit for bit -- the same statements draw it;
//   logp (nullable): logp[b] += (z + bias)[c] - logsumexp_i (z + bias)[i] (fp32, temperature 1, unfiltered; c the choice).
// GUIDED (classifier-free guidance): z holds 2 * Bc rows, the conditional ones first; block b draws for the pair (b, Bc + b) from
//   zc = z[b] + bias, zu = z[Bc + b] + bias, g = zc + (scale - 1) * (zc - zu)  -- difference, product and sum each rounded to
//   fp32 on their own (no fused multiply-add: a numpy float32 restatement gives the same bits); scale - 1 == 0 takes g = zc itself,
//   so that scale 1 is the unguided draw on the conditional rows whatever the unconditional ones hold;
//   v = g * (1/temperature), and from there on everything is the nucleus draw, the noise hashed with the pair index b;
//   next_tok[b] = next_tok[Bc + b] (both halves of the KV cache are fed the drawn token), out has Bc rows, and logp scores the
//   choice under the conditional row alone: log softmax(zc)[c], the model's own likelihood, comparable across guidance scales.
// Everything that changes between calls may come from device memory (params_dev: {1/temperature or 0, top_k, seed lo, seed hi} and,
// NUCLEUS, {top_p, scale}: the plain instance reads four words; pos_dev), and the choice is written where the next decode step
// reads its input token, so that decode + sampling replay as one HIP graph with no host round trip per position.
// LDS: the keys, 32 KB at nv = 8192, and under NUCLEUS as much again for u -- at most two such blocks per CU, so a B <= 128
// launch is resident at once.
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// (splitmix64: common.h)
#define SAMPLE_MAX_VOCAB 8192
__device__ __forceinline__ float block_max_f32(float x, float* red, int lane, int wid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  if (lane == 0) red[wid] = x;
  __syncthreads();
  x = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return x;
}
__device__ __forceinline__ float block_sum_f32(float x, float* red, int lane, int wid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if (lane == 0) red[wid] = x;
  __syncthreads();
  x = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return x;
}
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t x, uint64_t* red, int lane, int wid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if (lane == 0) red[wid] = x;
  __syncthreads();
  x = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return x;
}
__device__ __forceinline__ float guided_logit(float zc, float zu, float sm1) {
#pragma clang fp contract(off)
  const float d = zc - zu;
  const float t = sm1 * d;
  return sm1 == 0.f ? zc : zc + t;
}
template <bool NUCLEUS, bool GUIDED>
__device__ __forceinline__ void draw_tokens(const bf16_t* __restrict__ z, int ldz, const bf16_t* __restrict__ bias, int nv, float inv_temp,
                                            int top_k, uint64_t seed, float top_p, float scale, const unsigned* __restrict__ params_dev,
                                            int pos_arg, int* pos_dev, int advance, int token_offset, int* __restrict__ next_tok,
                                            int* __restrict__ out, int out_ld, int out_col0, float* __restrict__ logp) {
  static_assert(NUCLEUS || !GUIDED, "the guided draw is a nucleus draw");
  __shared__ unsigned keys[SAMPLE_MAX_VOCAB];
  __shared__ unsigned qu[NUCLEUS ? SAMPLE_MAX_VOCAB : 1];   // (the one-element forms are never referenced and take no LDS)
  __shared__ int cnt[4];
  __shared__ uint64_t red64[NUCLEUS ? 4 : 1];
  __shared__ float redf[NUCLEUS ? 4 : 1];
  __shared__ float bval[4];
  __shared__ int bidx[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (params_dev) {
    inv_temp = __uint_as_float(params_dev[0]);
    top_k = (int)params_dev[1];
    seed = (uint64_t)params_dev[2] | ((uint64_t)params_dev[3] << 32);
    if constexpr (NUCLEUS) top_p = __uint_as_float(params_dev[4]);
    if constexpr (GUIDED) scale = __uint_as_float(params_dev[5]);
  }
  const int counter = pos_dev ? *pos_dev : pos_arg;
  const bool greedy = !(inv_temp > 0.f);
  unsigned kmax = 0u;
  for (int i = tid; i < nv; i += 256) {
    float v = bf2f(z[(int64_t)b * ldz + i]);
    if (bias) v += bf2f(bias[i]);
    if constexpr (GUIDED) {
      float vu = bf2f(z[(int64_t)(gridDim.x + b) * ldz + i]);
      if (bias) vu += bf2f(bias[i]);
      v = guided_logit(v, vu, scale - 1.f);
    }
    if (!greedy) v *= inv_temp;
    const unsigned k = order_key(v);
    keys[i] = k;
    if constexpr (NUCLEUS) kmax = max(kmax, k);
  }
  __syncthreads();
  unsigned thr = 0u;
  if (!greedy && top_k > 0 && top_k < nv) {
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = thr | (1u << bit);
      int c = 0;
      for (int i = tid; i < nv; i += 256) c += keys[i] >= cand;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      if (lane == 0) cnt[wid] = c;
      __syncthreads();
      const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3];
      __syncthreads();
      if (total >= top_k) thr = cand;   // block-uniform
    }
  }
  // nucleus threshold on the quantised probabilities (block-uniform; 0 = no nucleus step)
  unsigned qthr = 0u;
  if constexpr (NUCLEUS) {
    if (!greedy && top_p > 0.f && top_p < 1.f) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
      if (lane == 0) cnt[wid] = (int)kmax;
      __syncthreads();
      kmax = max(max((unsigned)cnt[0], (unsigned)cnt[1]), max((unsigned)cnt[2], (unsigned)cnt[3]));
      __syncthreads();
      const float vmax = key_value(kmax);
      if (isfinite(vmax)) {
        uint64_t part = 0;
        for (int i = tid; i < nv; i += 256) {
          const unsigned k = keys[i];
          unsigned u = 0u;
          if (k >= thr) {
            const float e = expf(key_value(k) - vmax);     // in [0, 1]; NaN entries compare false and weigh nothing
            u = e >= 0.f ? (unsigned)(e * 2147483648.0f) : 0u;
          }
          qu[i] = u;
          part += u;
        }
        const uint64_t mass = block_sum_u64(part, red64, lane, wid);   // __syncthreads inside: qu is complete
        const uint64_t target = (uint64_t)ceil((double)top_p * (double)mass);
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned cand = qthr | (1u << bit);
          uint64_t s = 0;
          for (int i = tid; i < nv; i += 256) {
            const unsigned u = qu[i];
            s += u >= cand ? u : 0u;
          }
          if (block_sum_u64(s, red64, lane, wid) >= target) qthr = cand;   // block-uniform
        }
      }
    }
  }
  const uint64_t stream_key = splitmix64(seed ^ ((uint64_t)(unsigned)counter * 0xD2B74407B1CE6E93ull));
  float best = -INFINITY;
  int besti = nv;
  for (int i = tid; i < nv; i += 256) {   // ascending i per thread: strict > keeps the first maximum
    const unsigned k = keys[i];
    if (k < thr) continue;
    if constexpr (NUCLEUS)
      if (qthr && qu[i] < qthr) continue;
    float s = key_value(k);
    if (!greedy) {
      const uint64_t h = splitmix64(stream_key + (((uint64_t)(unsigned)b << 32) | (unsigned)i));
      const float u = ((float)(unsigned)(h >> 41) + 0.5f) * (1.0f / 8388608.0f);   // 23 bits: u strictly in (0, 1), see above
      s -= __logf(-__logf(u));
    }
    if (s > best) { best = s; besti = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  if (lane == 0) { bval[wid] = best; bidx[wid] = besti; }
  __syncthreads();
  if constexpr (NUCLEUS) {
    if (logp) {   // log-softmax of the unscaled row at the choice (every thread takes the choice from the wave winners)
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (bval[w] > best || (bval[w] == best && bidx[w] < besti)) { best = bval[w]; besti = bidx[w]; }
      float m = -INFINITY;
      for (int i = tid; i < nv; i += 256) {
        float v = bf2f(z[(int64_t)b * ldz + i]);
        if (bias) v += bf2f(bias[i]);
        m = fmaxf(m, v);
      }
      m = block_max_f32(m, redf, lane, wid);
      float se = 0.f;
      for (int i = tid; i < nv; i += 256) {
        float v = bf2f(z[(int64_t)b * ldz + i]);
        if (bias) v += bf2f(bias[i]);
        se += expf(v - m);
      }
      se = block_sum_f32(se, redf, lane, wid);
      if (tid == 0) {
        const int c = besti >= nv ? 0 : besti;
        float vc = bf2f(z[(int64_t)b * ldz + c]);
        if (bias) vc += bf2f(bias[c]);
        logp[b] += (vc - m) - logf(se);
      }
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (bval[w] > best || (bval[w] == best && bidx[w] < besti)) { best = bval[w]; besti = bidx[w]; }
    if (besti >= nv) besti = 0;          // all-NaN row: defined output
    if (next_tok) next_tok[b] = token_offset + besti;
    if (GUIDED && next_tok) next_tok[gridDim.x + b] = token_offset + besti;
    const int col = counter - out_col0;
    if (out && col >= 0 && col < out_ld) out[(int64_t)b * out_ld + col] = besti;
    if (advance && pos_dev) {            // the last block to finish moves the position on (every block has read it by then)
      __threadfence();
      if (atomicAdd(pos_dev + 1, 1) == (int)gridDim.x - 1) {
        pos_dev[1] = 0;
        pos_dev[0] = counter + 1;
      }
    }
  }
}
__global__ __launch_bounds__(256) void sample_tokens_kernel(const bf16_t* __restrict__ z, int ldz, const bf16_t* __restrict__ bias, int nv,
                                                            float inv_temp, int top_k, uint64_t seed, const unsigned* __restrict__ params_dev,
                                                            int pos_arg, int* pos_dev, int advance, int token_offset,
                                                            int* __restrict__ next_tok, int* __restrict__ out, int out_ld, int out_col0) {
  draw_tokens<false, false>(z, ldz, bias, nv, inv_temp, top_k, seed, 1.f, 1.f, params_dev, pos_arg, pos_dev, advance, token_offset, next_tok,
                            out, out_ld, out_col0, nullptr);
}
__global__ __launch_bounds__(256) void sample_tokens_p_kernel(const bf16_t* __restrict__ z, int ldz, const bf16_t* __restrict__ bias, int nv,
                                                              float inv_temp, int top_k, uint64_t seed, float top_p,
                                                              const unsigned* __restrict__ params_dev, int pos_arg, int* pos_dev, int advance,
                                                              int token_offset, int* __restrict__ next_tok, int* __restrict__ out, int out_ld,
                                                              int out_col0, float* __restrict__ logp) {
  draw_tokens<true, false>(z, ldz, bias, nv, inv_temp, top_k, seed, top_p, 1.f, params_dev, pos_arg, pos_dev, advance, token_offset, next_tok,
                           out, out_ld, out_col0, logp);
}
__global__ __launch_bounds__(256) void sample_tokens_guided_kernel(const bf16_t* __restrict__ z, int ldz, const bf16_t* __restrict__ bias, int nv,
                                                                   float inv_temp, int top_k, uint64_t seed, float top_p, float scale,
                                                                   const unsigned* __restrict__ params_dev, int pos_arg, int* pos_dev,
                                                                   int advance, int token_offset, int* __restrict__ next_tok,
                                                                   int* __restrict__ out, int out_ld, int out_col0, float* __restrict__ logp) {
  draw_tokens<true, true>(z, ldz, bias, nv, inv_temp, top_k, seed, top_p, scale, params_dev, pos_arg, pos_dev, advance, token_offset, next_tok,
                          out, out_ld, out_col0, logp);
}
// the checks and the launch that the three entry points share; name prefixes the messages.  rows: B, or the Bc pairs of the guided
// form, which has checked them with nv under its own message
enum DrawKind { DRAW_PLAIN, DRAW_NUCLEUS, DRAW_GUIDED };
static int launch_draw(const char* name, DrawKind kind, const uint16_t* z, int ldz, const uint16_t* bias, int rows, int nv, float temperature,
                       int top_k, uint64_t seed, float top_p, float scale, const uint32_t* params_dev, int pos, int32_t* pos_dev,
                       int advance, int token_offset, int32_t* next_tok, int32_t* out, int out_ld, int out_col0, float* logp, void* stream) {
  DMI_REQUIRE(z && (next_tok || out), "%s: null pointer", name);
  DMI_REQUIRE(rows > 0 && nv > 0 && nv <= SAMPLE_MAX_VOCAB && ldz >= nv, "%s: need 0 < nv <= %d (nv=%d)", name, SAMPLE_MAX_VOCAB, nv);
  DMI_REQUIRE(!out || out_ld > 0, "%s: out_ld", name);
  DMI_REQUIRE(!advance || pos_dev, "%s: advance needs pos_dev", name);
  const float inv_temp = temperature > 0.f ? 1.f / temperature : 0.f;
  const dim3 grid((unsigned)rows), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (kind == DRAW_PLAIN)
    sample_tokens_kernel<<<grid, block, 0, s>>>(z, ldz, bias, nv, inv_temp, top_k, seed, params_dev, pos, pos_dev, advance, token_offset, next_tok,
                                                out, out_ld, out_col0);
  else if (kind == DRAW_NUCLEUS)
    sample_tokens_p_kernel<<<grid, block, 0, s>>>(z, ldz, bias, nv, inv_temp, top_k, seed, top_p, params_dev, pos, pos_dev, advance, token_offset,
                                                  next_tok, out, out_ld, out_col0, logp);
  else
    sample_tokens_guided_kernel<<<grid, block, 0, s>>>(z, ldz, bias, nv, inv_temp, top_k, seed, top_p, scale, params_dev, pos, pos_dev, advance,
                                                       token_offset, next_tok, out, out_ld, out_col0, logp);
  DMI_CHECK_LAUNCH(name);
  return DMI_OK;
}
extern "C" int dmi_sample_tokens(const uint16_t* z, int ldz, const uint16_t* bias, int B, int nv, float temperature, int top_k,
                                 uint64_t seed, const uint32_t* params_dev, int pos, int32_t* pos_dev, int advance, int token_offset,
                                 int32_t* next_tok, int32_t* out, int out_ld, int out_col0, void* stream) {
  return launch_draw("sample_tokens", DRAW_PLAIN, z, ldz, bias, B, nv, temperature, top_k, seed, 1.f, 1.f, params_dev, pos, pos_dev, advance,
                     token_offset, next_tok, out, out_ld, out_col0, nullptr, stream);
}
extern "C" int dmi_sample_tokens_p(const uint16_t* z, int ldz, const uint16_t* bias, int B, int nv, float temperature, int top_k,
                                   uint64_t seed, float top_p, const uint32_t* params_dev, int pos, int32_t* pos_dev, int advance,
                                   int token_offset, int32_t* next_tok, int32_t* out, int out_ld, int out_col0, float* logp, void* stream) {
  DMI_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_tokens_p: top_p must lie in (0, 1] (top_p=%g)", (double)top_p);
  return launch_draw("sample_tokens_p", DRAW_NUCLEUS, z, ldz, bias, B, nv, temperature, top_k, seed, top_p, 1.f, params_dev, pos, pos_dev,
                     advance, token_offset, next_tok, out, out_ld, out_col0, logp, stream);
}
extern "C" int dmi_sample_tokens_guided(const uint16_t* z, int ldz, const uint16_t* bias, int Bc, int nv, float temperature, int top_k,
                                        uint64_t seed, float top_p, float scale, const uint32_t* params_dev, int pos, int32_t* pos_dev,
                                        int advance, int token_offset, int32_t* next_tok, int32_t* out, int out_ld, int out_col0, float* logp,
                                        void* stream) {
  DMI_REQUIRE(Bc > 0 && nv > 0 && nv <= SAMPLE_MAX_VOCAB && ldz >= nv, "sample_tokens_guided: need Bc > 0 and 0 < nv <= %d (Bc=%d, nv=%d)",
              SAMPLE_MAX_VOCAB, Bc, nv);
  DMI_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_tokens_guided: top_p must lie in (0, 1] (top_p=%g)", (double)top_p);
  DMI_REQUIRE(scale >= 0.f && scale <= 3.402823466e38f, "sample_tokens_guided: scale must be finite and >= 0 (scale=%g)", (double)scale);
  return launch_draw("sample_tokens_guided", DRAW_GUIDED, z, ldz, bias, Bc, nv, temperature, top_k, seed, top_p, scale, params_dev, pos, pos_dev,
                     advance, token_offset, next_tok, out, out_ld, out_col0, logp, stream);
}

// fp32 logits of a head-output slice: out[b, i] = float(z[b, i]) + float(bias[i])  (src/dalle_mtf/models.py:394-395)
__global__ void logits_f32_kernel(const bf16_t* __restrict__ z, int ldz, const bf16_t* __restrict__ bias, float* __restrict__ out, int nv) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  float v = bf2f(z[(int64_t)b * ldz + i]);
  if (bias) v += bf2f(bias[i]);
  out[(int64_t)b * nv + i] = v;
}
extern "C" int dmi_logits_f32(const uint16_t* z, int ldz, const uint16_t* bias, float* out, int B, int nv, void* stream) {
  DMI_REQUIRE(z && out, "logits_f32: null pointer");
  DMI_REQUIRE(B > 0 && nv > 0 && ldz >= nv, "logits_f32: need B > 0, 0 < nv <= ldz (B=%d nv=%d ldz=%d)", B, nv, ldz);
  logits_f32_kernel<<<dim3((unsigned)((nv + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream>>>(z, ldz, bias, out, nv);
  DMI_CHECK_LAUNCH("logits_f32");
  return DMI_OK;
}
