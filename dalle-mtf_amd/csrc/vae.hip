// vae.hip -- data-movement and pointwise kernels of the discrete-VAE path (reference
// src/vae_tf/models.py:81-163, src/vae_tf/layers.py:4-25).
//
// Convolution lowering: every flavour the reference uses (tf.layers.conv2d 4x4 s2 / 3x3 s1 / 1x1 SAME,
// conv2d_transpose 4x4 s2 SAME; forward, input gradient, weight gradient) is a tap list feeding the MFMA GEMMs of
// gemm.hip (NT for fwd / dgrad, TN for wgrad).  Layers with C_in % 64 == 0 gather implicitly inside the GEMM
// (dmi_conv_gemm_nt / dmi_conv_wgrad_tn); the materialised im2col below serves the 3-channel input layer and is the
// bit-exact reference of the implicit kernels in the tests:
//   conv s1/s2 fwd      : taps (ky-pad, kx-pad), stride s           -> Y = col(X) . W^T
//   conv s1 dgrad       : taps (pad-ky, pad-kx) on dY               -> dX = col(dY) . Wd^T ,  Wd[ci][(k,co)]
//   conv s2 dgrad / conv-transpose fwd : 4 output-parity classes, 2x2 taps each, then a pixel interleave
//   wgrad               : dW[(k,ci)][co] = col(X)^T . dY   (TN GEMM; lands in the TF kernel layout)
// Activations are NHWC bf16 matrices [B*H*W, C] with C % 8 == 0 (the 3-channel image / reconstruction are padded
// to 8 channels with zeros), so every access is a 16-byte vector.
#include "common.h"

#define MAX_TAPS 16
struct TapList {
  int n;
  int dy[MAX_TAPS];
  int dx[MAX_TAPS];
};

// out[(b,oy,ox)][t*C + c] = x[b, oy*s + dy[t], ox*s + dx[t], c]   (0 outside the image); row pitch ldo >= n*C,
// columns [n*C, ldo) are zero-filled (K padding for the GEMM).
__global__ __launch_bounds__(256) void im2col_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, TapList taps,
                                                     int B, int H, int W, int C, int Ho, int Wo, int stride, int ldo) {
  const int cpr = ldo / 8;  // chunks per output row
  const int64_t total = (int64_t)B * Ho * Wo * cpr;
  const int cc = C / 8;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int ch = (int)(idx % cpr);
    const int64_t m = idx / cpr;
    const int t = ch / cc, c8 = ch % cc;
    u32x4 v = {0, 0, 0, 0};
    if (t < taps.n) {
      const int ox = (int)(m % Wo);
      const int oy = (int)((m / Wo) % Ho);
      const int b = (int)(m / ((int64_t)Wo * Ho));
      const int iy = oy * stride + taps.dy[t], ix = ox * stride + taps.dx[t];
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const u32x4*)(x + (((int64_t)b * H + iy) * W + ix) * C + c8 * 8);
    }
    *(u32x4*)(out + m * ldo + ch * 8) = v;
  }
}

extern "C" int dmi_im2col(const uint16_t* x, uint16_t* out, int B, int H, int W, int C, int Ho, int Wo, int stride,
                          int ntaps, const int* dy, const int* dx, int ldo, void* stream) {
  DMI_REQUIRE(x && out && dy && dx, "im2col: null pointer");
  DMI_REQUIRE(C % 8 == 0 && ldo % 8 == 0 && ntaps >= 1 && ntaps <= MAX_TAPS && ldo >= ntaps * C, "im2col: need C%%8==0, ldo%%8==0, ldo>=ntaps*C (C=%d ntaps=%d ldo=%d)", C, ntaps, ldo);
  TapList t;
  t.n = ntaps;
  for (int i = 0; i < ntaps; ++i) { t.dy[i] = dy[i]; t.dx[i] = dx[i]; }
  const int64_t total = (int64_t)B * Ho * Wo * (ldo / 8);
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 65536) blocks = 65536;
  im2col_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(x, out, t, B, H, W, C, Ho, Wo, stride, ldo);
  DMI_CHECK_LAUNCH("im2col");
  return DMI_OK;
}

// out[a][t*Bn + b] = in[idx[t]][a][b], row pitch ldo >= nsel*Bn, tail zero-filled
// (weight re-layouts: [k][ci][co] -> [ci][(k',co)] for dgrad / output-parity GEMMs)
__global__ __launch_bounds__(256) void weight_gather_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, TapList sel,
                                                            int A, int Bn, int ldo) {
  const int64_t total = (int64_t)A * ldo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % ldo);
    const int a = (int)(i / ldo);
    const int t = j / Bn, b = j % Bn;
    out[i] = (t < sel.n) ? in[((int64_t)sel.dy[t] * A + a) * Bn + b] : (bf16_t)0;
  }
}
extern "C" int dmi_weight_gather(const uint16_t* in, uint16_t* out, int A, int Bn, int nsel, const int* idx, int ldo, void* stream) {
  DMI_REQUIRE(in && out && idx && nsel >= 1 && nsel <= MAX_TAPS && A > 0 && Bn > 0 && ldo >= nsel * Bn, "weight_gather: bad args");
  TapList t;
  t.n = nsel;
  for (int i = 0; i < nsel; ++i) { t.dy[i] = idx[i]; t.dx[i] = 0; }
  const int64_t total = (int64_t)A * ldo;
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 4096) blocks = 4096;
  weight_gather_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(in, out, t, A, Bn, ldo);
  DMI_CHECK_LAUNCH("weight_gather");
  return DMI_OK;
}

// Every per-step weight re-layout of a model in ONE launch (the small VAE configurations spent 50 launches of ~3 us on them):
// table[i] = {in_off, out_off, A, Bn, nsel, ldo, first_block, idx[16]} (int64; offsets in elements of in_base / out_base,
// first_block ascending); a block covers 2048 consecutive output elements of its item.
#define WG_ROW 23
__global__ __launch_bounds__(256) void weight_gather_batch_kernel(const bf16_t* __restrict__ in_base, bf16_t* __restrict__ out_base,
                                                                  const int64_t* __restrict__ table, int n) {
  const int64_t blk = blockIdx.x;
  int i = 0;
  while (i + 1 < n && table[(i + 1) * WG_ROW + 6] <= blk) ++i;
  const int64_t* row = table + (int64_t)i * WG_ROW;
  const bf16_t* in = in_base + row[0];
  bf16_t* out = out_base + row[1];
  const int A = (int)row[2], Bn = (int)row[3], nsel = (int)row[4], ldo = (int)row[5];
  const int64_t total = (int64_t)A * ldo;
  const int64_t base = (blk - row[6]) * 2048;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t e = base + k * 256 + threadIdx.x;
    if (e >= total) break;
    const int j = (int)(e % ldo);
    const int a = (int)(e / ldo);
    const int t = j / Bn, b = j % Bn;
    out[e] = (t < nsel) ? in[((int64_t)row[7 + t] * A + a) * Bn + b] : (bf16_t)0;
  }
}
extern "C" int dmi_weight_gather_batch(const uint16_t* in_base, uint16_t* out_base, const int64_t* table, int n, int64_t total_blocks,
                                       void* stream) {
  DMI_REQUIRE(in_base && out_base && table && n > 0 && total_blocks > 0, "weight_gather_batch: bad args");
  weight_gather_batch_kernel<<<dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream>>>(in_base, out_base, table, n);
  DMI_CHECK_LAUNCH("weight_gather_batch");
  return DMI_OK;
}

// out[b, 2t+py, 2u+px, :] = in[p = py*2+px][b, t, u, :]
__global__ __launch_bounds__(256) void pixel_interleave_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int B,
                                                               int Ht, int Wt, int C) {
  const int cc = C / 8;
  const int64_t per = (int64_t)B * Ht * Wt * cc;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < 4 * per; idx += (int64_t)gridDim.x * 256) {
    const int p = (int)(idx / per);
    const int64_t r = idx % per;
    const int c8 = (int)(r % cc);
    const int64_t m = r / cc;
    const int u = (int)(m % Wt), t = (int)((m / Wt) % Ht), b = (int)(m / ((int64_t)Wt * Ht));
    const int py = p >> 1, px = p & 1;
    *(u32x4*)(out + ((((int64_t)b * 2 * Ht + 2 * t + py) * 2 * Wt) + 2 * u + px) * C + c8 * 8) = *(const u32x4*)(in + idx * 8);
  }
}
extern "C" int dmi_pixel_interleave(const uint16_t* in4, uint16_t* out, int B, int Ht, int Wt, int C, void* stream) {
  DMI_REQUIRE(in4 && out && C % 8 == 0, "pixel_interleave: bad args");
  const int64_t total = 4 * (int64_t)B * Ht * Wt * (C / 8);
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 65536) blocks = 65536;
  pixel_interleave_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(in4, out, B, Ht, Wt, C);
  DMI_CHECK_LAUNCH("pixel_interleave");
  return DMI_OK;
}

// image fp32 [N, Cin] -> bf16 [N, Cp] (zero padded channels)
__global__ __launch_bounds__(256) void pad_channels_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t N,
                                                           int Cin, int Cp) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N * Cp; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % Cp);
    const int64_t n = i / Cp;
    out[i] = c < Cin ? f2bf(in[n * Cin + c]) : (bf16_t)0;
  }
}
extern "C" int dmi_pad_channels(const float* in, uint16_t* out, int64_t N, int Cin, int Cp, void* stream) {
  DMI_REQUIRE(in && out && N > 0 && Cin <= Cp, "pad_channels: bad args");
  int64_t blocks = cdiv64(N * Cp, 256);
  if (blocks > 16384) blocks = 16384;
  pad_channels_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(in, out, N, Cin, Cp);
  DMI_CHECK_LAUNCH("pad_channels");
  return DMI_OK;
}

// =====================================================================================
// Gumbel-softmax (src/vae_tf/layers.py:4-21): g = -log(-log u); y = softmax((logits + g)/T); hard: one-hot of the
// argmax (first max), straight-through gradient.  One wave per row; T columns (T % 8 == 0).
// Uniform noise is an INPUT (TF's Philox stream cannot be reproduced; parity is on identical noise).
// =====================================================================================
template <int NC>  // NC = ceil(T/8/64) chunks per lane
__global__ __launch_bounds__(256) void gumbel_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ u,
                                                         bf16_t* __restrict__ y, bf16_t* __restrict__ y_soft,
                                                         int* __restrict__ index, int64_t M, int T, float inv_temp, int hard,
                                                         const float* __restrict__ temp_dev) {
  if (temp_dev) inv_temp = 1.f / temp_dev[0];   // graph replay: the annealed temperature lives in device memory
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= M) return;
  const int nch = T / 8;
  float v[NC][8];
  float mx = -INFINITY;
  int mi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 l = *(const f32x4*)(logits + row * T + c * 8 + 4 * q);
        const f32x4 uu = *(const f32x4*)(u + row * T + c * 8 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = -logf(-logf(uu[e]));
          const float z = (l[e] + g) * inv_temp;
          v[i][4 * q + e] = z;
          const int col = c * 8 + 4 * q + e;
          if (z > mx || (z == mx && col < mi)) { mx = z; mi = col; }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[i][e] = __expf(v[i][e] - mx);
        s += v[i][e];
      }
    }
  }
  const float inv = 1.f / wave_sum(s);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      float p[8], o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        p[e] = v[i][e] * inv;
        o[e] = hard ? ((c * 8 + e == mi) ? 1.f : 0.f) : p[e];
      }
      *(u32x4*)(y_soft + row * T + c * 8) = pack8(p);
      *(u32x4*)(y + row * T + c * 8) = pack8(o);
    }
  }
  if (lane == 0 && index) index[row] = mi;
}
extern "C" int dmi_gumbel_softmax_fwd(const float* logits, const float* u, uint16_t* y, uint16_t* y_soft, int32_t* index,
                                      int64_t M, int T, float temperature, int hard, const float* temperature_dev, void* stream) {
  DMI_REQUIRE(logits && u && y && y_soft && M > 0 && T % 8 == 0 && T <= 4096 && (temperature > 0.f || temperature_dev),
              "gumbel_fwd: bad args (T=%d)", T);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)cdiv64(M, 4)), blk(256);
  const float it = temperature_dev ? 0.f : 1.f / temperature;
  if (T <= 512) gumbel_fwd_kernel<1><<<grid, blk, 0, st>>>(logits, u, y, y_soft, index, M, T, it, hard, temperature_dev);
  else if (T <= 1024) gumbel_fwd_kernel<2><<<grid, blk, 0, st>>>(logits, u, y, y_soft, index, M, T, it, hard, temperature_dev);
  else if (T <= 2048) gumbel_fwd_kernel<4><<<grid, blk, 0, st>>>(logits, u, y, y_soft, index, M, T, it, hard, temperature_dev);
  else gumbel_fwd_kernel<8><<<grid, blk, 0, st>>>(logits, u, y, y_soft, index, M, T, it, hard, temperature_dev);
  DMI_CHECK_LAUNCH("gumbel_fwd");
  return DMI_OK;
}

// dlogits = (1/T) * y_soft * (dy - sum_j dy_j y_soft_j)   (hard: straight-through => same formula on y_soft)
__global__ __launch_bounds__(256) void gumbel_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y_soft,
                                                         bf16_t* __restrict__ dlogits, int64_t M, int T, float inv_temp,
                                                         const float* __restrict__ temp_dev) {
  if (temp_dev) inv_temp = 1.f / temp_dev[0];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= M) return;
  const int nch = T / 8;
  float dot = 0.f;
  for (int c = lane; c < nch; c += 64) {
    float a[8], p[8];
    unpack8(*(const u32x4*)(dy + row * T + c * 8), a);
    unpack8(*(const u32x4*)(y_soft + row * T + c * 8), p);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot += a[e] * p[e];
  }
  dot = wave_sum(dot);
  for (int c = lane; c < nch; c += 64) {
    float a[8], p[8], o[8];
    unpack8(*(const u32x4*)(dy + row * T + c * 8), a);
    unpack8(*(const u32x4*)(y_soft + row * T + c * 8), p);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = inv_temp * p[e] * (a[e] - dot);
    *(u32x4*)(dlogits + row * T + c * 8) = pack8(o);
  }
}
extern "C" int dmi_gumbel_softmax_bwd(const uint16_t* dy, const uint16_t* y_soft, uint16_t* dlogits, int64_t M, int T,
                                      float temperature, const float* temperature_dev, void* stream) {
  DMI_REQUIRE(dy && y_soft && dlogits && M > 0 && T % 8 == 0 && (temperature > 0.f || temperature_dev), "gumbel_bwd: bad args");
  gumbel_bwd_kernel<<<dim3((unsigned)cdiv64(M, 4)), dim3(256), 0, (hipStream_t)stream>>>(
      dy, y_soft, dlogits, M, T, temperature_dev ? 0.f : 1.f / temperature, temperature_dev);
  DMI_CHECK_LAUNCH("gumbel_bwd");
  return DMI_OK;
}

// =====================================================================================
// KL(q(z|x) || uniform) of the codebook posterior and codebook usage (DESIGN.md §4 "VAE: KL term and codebook statistics").
// Per row m of the fp32 logits [M, T], no noise, no temperature:
//   lse = logsumexp_k l_k,  q_k = exp(l_k - lse),  e = sum_k q_k ln q_k,  KL_m = e + ln T,  KL = mean_m KL_m
//   d loss / d l_j gains (beta_t / M) q_j (ln q_j - e)
// No float atomics anywhere: every sum has a fixed order (lane-serial, wave butterfly, block order), so two runs give equal bits.
// =====================================================================================
#define KL_MAX_T 4096
// One wave per row, the row in registers (as gumbel_fwd_kernel<NC>).  With d_k = l_k - max, t_k = exp(d_k), s = sum t_k:
// lse = max + ln s and e = (sum_k t_k d_k) / s - ln s: both sums have terms of one sign, and d_k is taken against the row's own
// maximum, so a common shift of the logits (normal + 1000) costs nothing but the final rounding of lse.  t_k = 0 (underflow)
// contributes 0 * d_k = 0 (d_k is finite).  exp is __expf (exp2 of d log2 e, as in gumbel_fwd_kernel); the error model
// of tests/vae_kl_ref.py counts the product's rounding.  part[block] = the block's four KL_m in the order (0 + 1) + (2 + 3).
template <int NC>
__global__ __launch_bounds__(256) void codebook_kl_fwd_kernel(const float* __restrict__ logits, float* __restrict__ rowstat,
                                                              float* __restrict__ part, int64_t M, int T, float ln_t) {
  __shared__ float sm[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  const bool live = row < M;
  const int nch = T / 8;
  float klm = 0.f;
  if (live) {
    float v[NC][8];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 l = *(const f32x4*)(logits + row * T + c * 8 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[i][4 * q + e] = l[e];
            mx = fmaxf(mx, l[e]);
          }
        }
      }
    }
    mx = wave_max(mx);
    float s = 0.f, a = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      if (c < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[i][e] - mx;
          const float t = __expf(d);
          s += t;
          a += t * d;
        }
      }
    }
    s = wave_sum(s);
    a = wave_sum(a);
    const float ls = logf(s);
    const float en = a / s - ls;
    klm = en + ln_t;
    if (lane == 0) {
      rowstat[row * 2] = mx + ls;
      rowstat[row * 2 + 1] = en;
    }
  }
  if (lane == 0) sm[wid] = klm;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
#define USAGE_MAX_BLOCKS 512   // row slabs of dmi_codebook_usage
#define USAGE_MIN_ROWS 32      // ... of at least this many rows each
static inline int64_t usage_blocks(int64_t M) {
  const int64_t nb = cdiv64(M, USAGE_MIN_ROWS);
  return nb > USAGE_MAX_BLOCKS ? USAGE_MAX_BLOCKS : nb;
}
// the larger of: one KL partial per four rows; [blocks][T] fp32 + [blocks][T] int32 usage partials
extern "C" int64_t dmi_codebook_kl_workspace_bytes(int64_t M, int T) {
  if (M <= 0 || T <= 0) return 0;
  const int64_t kl = cdiv64(M, 4) * 4, us = usage_blocks(M) * (int64_t)T * 8;
  return kl > us ? kl : us;
}
extern "C" int dmi_codebook_kl_fwd(const float* logits, float* rowstat, float* kl, int64_t M, int T, void* workspace, void* stream) {
  DMI_REQUIRE(logits && rowstat && kl && workspace, "codebook_kl_fwd: null pointer");
  DMI_REQUIRE(M > 0, "codebook_kl_fwd: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && T % 8 == 0 && T <= KL_MAX_T, "codebook_kl_fwd: T must be a multiple of 8 and at most %d (T=%d)", KL_MAX_T, T);
  DMI_REQUIRE(cdiv64(M, 4) <= 0x7fffffffLL, "codebook_kl_fwd: M too large (M=%lld)", (long long)M);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = cdiv64(M, 4);
  dim3 grid((unsigned)nb), blk(256);
  const float ln_t = (float)log((double)T);
  float* part = (float*)workspace;
  if (T <= 512) codebook_kl_fwd_kernel<1><<<grid, blk, 0, st>>>(logits, rowstat, part, M, T, ln_t);
  else if (T <= 1024) codebook_kl_fwd_kernel<2><<<grid, blk, 0, st>>>(logits, rowstat, part, M, T, ln_t);
  else if (T <= 2048) codebook_kl_fwd_kernel<4><<<grid, blk, 0, st>>>(logits, rowstat, part, M, T, ln_t);
  else codebook_kl_fwd_kernel<8><<<grid, blk, 0, st>>>(logits, rowstat, part, M, T, ln_t);
  DMI_CHECK_LAUNCH("codebook_kl_fwd");
  return dmi_sum_f32(part, nb, 1.f / (float)M, kl, stream);
}

// gumbel_bwd_kernel with the KL gradient added before the one bf16 rounding:
//   dlogits = bf16( (1/tau) y_soft (dy - sum_j dy_j y_soft_j) + (beta_t / M) q (ln q - e) ),  ln q = l - lse, q = exp(ln q)
// The Gumbel term is the expression of gumbel_bwd_kernel, formed first and on its own; with beta_t == 0 nothing is added to it
// (adding 0 would turn a -0 into +0), so that case gives gumbel_bwd_kernel's bits.
__global__ __launch_bounds__(256) void gumbel_bwd_kl_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y_soft,
                                                            const float* __restrict__ logits, const float* __restrict__ rowstat,
                                                            bf16_t* __restrict__ dlogits, int64_t M, int T, float inv_temp,
                                                            const float* __restrict__ temp_dev, float klw,
                                                            const float* __restrict__ klw_dev) {
  if (temp_dev) inv_temp = 1.f / temp_dev[0];
  if (klw_dev) klw = klw_dev[0];
  const float cw = klw / (float)M;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= M) return;
  const int nch = T / 8;
  float dot = 0.f;
  for (int c = lane; c < nch; c += 64) {
    float a[8], p[8];
    unpack8(*(const u32x4*)(dy + row * T + c * 8), a);
    unpack8(*(const u32x4*)(y_soft + row * T + c * 8), p);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot += a[e] * p[e];
  }
  dot = wave_sum(dot);
  const float lse = rowstat[row * 2], en = rowstat[row * 2 + 1];
  for (int c = lane; c < nch; c += 64) {
    float a[8], p[8], o[8];
    unpack8(*(const u32x4*)(dy + row * T + c * 8), a);
    unpack8(*(const u32x4*)(y_soft + row * T + c * 8), p);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = inv_temp * p[e] * (a[e] - dot);
    if (cw != 0.f) {
      const f32x4 l0 = *(const f32x4*)(logits + row * T + c * 8), l1 = *(const f32x4*)(logits + row * T + c * 8 + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float lq = (e < 4 ? l0[e & 3] : l1[e & 3]) - lse;
        o[e] += cw * __expf(lq) * (lq - en);
      }
    }
    *(u32x4*)(dlogits + row * T + c * 8) = pack8(o);
  }
}
extern "C" int dmi_gumbel_softmax_bwd_kl(const uint16_t* dy, const uint16_t* y_soft, const float* logits, const float* rowstat,
                                         uint16_t* dlogits, int64_t M, int T, float temperature, const float* temperature_dev,
                                         float kl_weight, const float* kl_weight_dev, void* stream) {
  DMI_REQUIRE(dy && y_soft && logits && rowstat && dlogits, "gumbel_bwd_kl: null pointer");
  DMI_REQUIRE(M > 0, "gumbel_bwd_kl: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && T % 8 == 0 && T <= KL_MAX_T, "gumbel_bwd_kl: T must be a multiple of 8 and at most %d (T=%d)", KL_MAX_T, T);
  DMI_REQUIRE(cdiv64(M, 4) <= 0x7fffffffLL, "gumbel_bwd_kl: M too large (M=%lld)", (long long)M);
  DMI_REQUIRE(temperature > 0.f || temperature_dev, "gumbel_bwd_kl: temperature must be positive (or given on the device)");
  DMI_REQUIRE(kl_weight_dev || (kl_weight >= 0.f && kl_weight <= 3.0e38f), "gumbel_bwd_kl: kl_weight must be finite and >= 0");
  gumbel_bwd_kl_kernel<<<dim3((unsigned)cdiv64(M, 4)), dim3(256), 0, (hipStream_t)stream>>>(
      dy, y_soft, logits, rowstat, dlogits, M, T, temperature_dev ? 0.f : 1.f / temperature, temperature_dev,
      kl_weight_dev ? 0.f : kl_weight, kl_weight_dev);
  DMI_CHECK_LAUNCH("gumbel_bwd_kl");
  return DMI_OK;
}

// loss[0] = recon[0] + beta_t * kl[0], one rounding (fused multiply-add); beta_t by value or from device memory
__global__ void elbo_loss_kernel(const float* __restrict__ recon, const float* __restrict__ kl, float klw,
                                 const float* __restrict__ klw_dev, float* __restrict__ loss) {
  if (klw_dev) klw = klw_dev[0];
  loss[0] = __fmaf_rn(klw, kl[0], recon[0]);
}
extern "C" int dmi_elbo_loss(const float* recon, const float* kl, float kl_weight, const float* kl_weight_dev, float* loss,
                             void* stream) {
  DMI_REQUIRE(recon && kl && loss, "elbo_loss: null pointer");
  DMI_REQUIRE(kl_weight_dev || (kl_weight >= 0.f && kl_weight <= 3.0e38f), "elbo_loss: kl_weight must be finite and >= 0");
  elbo_loss_kernel<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(recon, kl, kl_weight_dev ? 0.f : kl_weight, kl_weight_dev, loss);
  DMI_CHECK_LAUNCH("elbo_loss");
  return DMI_OK;
}

// Codebook usage.  Stage 1: block b owns rows [b*rpb, min(M, (b+1)*rpb)).  Its 1024 threads are four row groups of 256: group g takes
// rows r0 + g, r0 + g + 4, ...; a thread owns the 8-column chunks t and t + 256 and adds q = exp(l - lse) of its columns row by row in
// registers; groups 1..3 hand their sums over in LDS and group 0 adds the four as (0 + 1) + (2 + 3) -> qpart[b][T].  The block's
// picks index[m] are then counted in an LDS histogram over the same storage (integer adds: exact in any order) -> cpart[b][T].
// Stage 2: 16 columns per block, 64 groups of threads each add a 64th of the slabs in block order, then group 0 adds the 64 in
// order (T / 16 blocks: 128 at T = 2048, enough to spread the 8 MB of partials over the device).
__global__ __launch_bounds__(1024) void codebook_usage_part_kernel(const float* __restrict__ logits, const float* __restrict__ rowstat,
                                                                   const int* __restrict__ index, float* __restrict__ qpart,
                                                                   int* __restrict__ cpart, int64_t M, int T, int64_t rpb) {
  __shared__ float red[3 * KL_MAX_T];
  const int tid = threadIdx.x, ct = tid & 255, grp = tid >> 8;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < M ? r0 + rpb : M;
  const int nch = T / 8;
  if (qpart) {
    float acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
#pragma unroll 4
    for (int64_t r = r0 + grp; r < r1; r += 4) {
      const float lse = rowstat[r * 2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = ct + 256 * i;
        if (c < nch) {
          const f32x4 l0 = *(const f32x4*)(logits + r * T + c * 8), l1 = *(const f32x4*)(logits + r * T + c * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[i][e] += __expf(l0[e] - lse);
            acc[i][4 + e] += __expf(l1[e] - lse);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = ct + 256 * i;
      if (grp > 0 && c < nch) {
        float* dst = red + (grp - 1) * T + c * 8;
        *(f32x4*)dst = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        *(f32x4*)(dst + 4) = f32x4{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = ct + 256 * i;
      if (grp == 0 && c < nch) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (acc[i][e] + red[c * 8 + e]) + (red[T + c * 8 + e] + red[2 * T + c * 8 + e]);
        float* dst = qpart + (int64_t)blockIdx.x * T + c * 8;
        *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
        *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
      }
    }
    __syncthreads();     // red is the histogram from here on
  }
  if (cpart) {
    int* hist = (int*)red;
    for (int k = tid; k < T; k += 1024) hist[k] = 0;
    __syncthreads();
    for (int64_t r = r0 + tid; r < r1; r += 1024) {
      const int k = index[r];
      if (k >= 0 && k < T) atomicAdd(&hist[k], 1);
    }
    __syncthreads();
    for (int k = tid; k < T; k += 1024) cpart[(int64_t)blockIdx.x * T + k] = hist[k];
  }
}
__global__ __launch_bounds__(1024) void codebook_usage_sum_kernel(const float* __restrict__ qpart, const int* __restrict__ cpart,
                                                                  float* __restrict__ qsum, int* __restrict__ counts, int T, int nb) {
  __shared__ float fq[64][16];
  __shared__ int fc[64][16];
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + j;
  const int per = (nb + 63) / 64;
  const int b0 = grp * per, b1 = (b0 + per < nb) ? b0 + per : nb;
  float a = 0.f;
  int n = 0;
  if (col < T) {
    if (qpart)
      for (int b = b0; b < b1; ++b) a += qpart[(int64_t)b * T + col];
    if (cpart)
      for (int b = b0; b < b1; ++b) n += cpart[(int64_t)b * T + col];
  }
  fq[grp][j] = a;
  fc[grp][j] = n;
  __syncthreads();
  if (grp == 0 && col < T) {
    float q = fq[0][j];
    int c = fc[0][j];
#pragma unroll 8
    for (int g = 1; g < 64; ++g) {
      q += fq[g][j];
      c += fc[g][j];
    }
    if (qsum) qsum[col] = q;
    if (counts) counts[col] = c;
  }
}
extern "C" int dmi_codebook_usage(const float* logits, const float* rowstat, const int32_t* index, float* qsum, int32_t* counts,
                                  int64_t M, int T, void* workspace, void* stream) {
  DMI_REQUIRE(workspace && (qsum || counts), "codebook_usage: null pointer (workspace, or both qsum and counts)");
  DMI_REQUIRE(!qsum || (logits && rowstat), "codebook_usage: null pointer (qsum needs logits and rowstat)");
  DMI_REQUIRE(!counts || index, "codebook_usage: null pointer (counts needs index)");
  DMI_REQUIRE(M > 0, "codebook_usage: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && T % 8 == 0 && T <= KL_MAX_T, "codebook_usage: T must be a multiple of 8 and at most %d (T=%d)", KL_MAX_T, T);
  const int64_t nb = usage_blocks(M);
  const int64_t rpb = cdiv64(M, nb);
  const int64_t nbu = cdiv64(M, rpb);       // slabs that hold a row (<= nb)
  float* qpart = qsum ? (float*)workspace : nullptr;
  int* cpart = counts ? (int*)((float*)workspace + nb * T) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  codebook_usage_part_kernel<<<dim3((unsigned)nbu), dim3(1024), 0, st>>>(logits, rowstat, index, qpart, cpart, M, T, rpb);
  DMI_CHECK_LAUNCH("codebook_usage");
  codebook_usage_sum_kernel<<<dim3((unsigned)((T + 15) / 16)), dim3(1024), 0, st>>>(qpart, cpart, qsum, counts, T, (int)nbu);
  DMI_CHECK_LAUNCH("codebook_usage_sum");
  return DMI_OK;
}

// =====================================================================================
// MSE (src/vae_tf/layers.py:24-25): loss = mean((img - out)^2) over N*Cin values; out bf16 [N, Cp] (Cp >= Cin padded);
// d_out = 2 (out - img) * grad_scale / (N*Cin), pad channels 0.  partial sums -> dmi_sum_f32.
// =====================================================================================
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ img, const bf16_t* __restrict__ outp,
                                                  bf16_t* __restrict__ dout, float* __restrict__ part, int64_t N, int Cin, int Cp,
                                                  float gscale) {
  __shared__ float sm[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N * Cp; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % Cp);
    const int64_t n = i / Cp;
    float d = 0.f;
    if (c < Cin) {
      d = bf2f(outp[i]) - img[n * Cin + c];
      acc += d * d;
    }
    if (dout) dout[i] = f2bf(d * gscale);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
#define MSE_BLOCKS 1024
extern "C" int64_t dmi_mse_workspace_bytes(void) { return MSE_BLOCKS * 4; }
extern "C" int dmi_sum_f32(const float* x, int64_t n, float scale, float* out, void* stream);
extern "C" int dmi_mse_loss(const float* img, const uint16_t* outp, uint16_t* dout, float* loss, int64_t N, int Cin, int Cp,
                            float grad_scale, void* workspace, void* stream) {
  DMI_REQUIRE(img && outp && loss && workspace && N > 0 && Cin <= Cp, "mse: bad args");
  const float gs = 2.f * grad_scale / ((float)N * (float)Cin);
  mse_kernel<<<dim3(MSE_BLOCKS), dim3(256), 0, (hipStream_t)stream>>>(img, outp, dout, (float*)workspace, N, Cin, Cp, gs);
  DMI_CHECK_LAUNCH("mse");
  return dmi_sum_f32((const float*)workspace, MSE_BLOCKS, 1.f / ((float)N * (float)Cin), loss, stream);
}

// dst += src  (fp32; the tied codebook receives gradients from the encoder and the decoder matmul)
__global__ __launch_bounds__(256) void add_f32_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] += src[i];
}
extern "C" int dmi_add_f32(float* dst, const float* src, int64_t n, void* stream) {
  DMI_REQUIRE(dst && src && n > 0, "add_f32: bad args");
  int64_t blocks = cdiv64(n, 256);
  if (blocks > 4096) blocks = 4096;
  add_f32_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(dst, src, n);
  DMI_CHECK_LAUNCH("add_f32");
  return DMI_OK;
}

// bf16 [N, Cp] -> fp32 [N, Cin] (reconstruction image for summaries)
__global__ __launch_bounds__(256) void unpad_channels_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, int64_t N, int Cin, int Cp) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N * Cin; i += (int64_t)gridDim.x * 256)
    out[i] = bf2f(in[(i / Cin) * Cp + (i % Cin)]);
}
extern "C" int dmi_unpad_channels(const uint16_t* in, float* out, int64_t N, int Cin, int Cp, void* stream) {
  DMI_REQUIRE(in && out && N > 0 && Cin <= Cp, "unpad_channels: bad args");
  int64_t blocks = cdiv64(N * Cin, 256);
  if (blocks > 16384) blocks = 16384;
  unpad_channels_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(in, out, N, Cin, Cp);
  DMI_CHECK_LAUNCH("unpad_channels");
  return DMI_OK;
}

// =====================================================================================
// fp32 convolution for the TOKENISING encoder.  Inside dalle_model_fn the reference builds the VAE without use_bf16
// (src/model_fns.py:43-51), so the image tokens fed to DALL-E come from an fp32 encoder and an fp32 `x @ codebook`
// (src/vae_tf/models.py:81-120); argmax over bf16-computed logits flips tokens whose top-2 gap is below bf16 noise.
// This kernel is that path: implicit-im2col convolution on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32, 1/16 of
// the bf16 rate -- forward only, the image is tokenised once per step), weights in the TF layout [(tap, ci)][co] straight
// from the fp32 master buffer.
//   out[(b,oy,ox)][n] = sum_t sum_c x[b, oy*s + dy[t], ox*s + dx[t], c] * Wk[(t*C + c)][n]  + bias[n]  (ReLU) (+ residual)
// Block = 128 output pixels x 64 channels, 4 waves of 32 x 64; the K loop walks (tap, 8-channel chunk): a chunk lies in one
// tap (C % 8 == 0).  LDS: A chunk k-major [8][128] so both MFMA operands are read as 32 consecutive floats.
// The codebook product is the same kernel with one tap on a 1x1 "image".
// =====================================================================================
typedef __attribute__((ext_vector_type(4))) float v4f;
__global__ __launch_bounds__(256) void conv2d_f32_kernel(const float* __restrict__ x, const float* __restrict__ Wk,
                                                         const float* __restrict__ bias, const float* __restrict__ residual,
                                                         float* __restrict__ out, TapList taps, int B, int H, int W, int C,
                                                         int Ho, int Wo, int stride, int N, int relu) {
  __shared__ float As[8][128];
  __shared__ float Ws[8][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t M = (int64_t)B * Ho * Wo;
  const int64_t m0 = (int64_t)blockIdx.x * 128;
  const int n0 = blockIdx.y * 64;
  // loader role: pixel p, channel half
  const int p = tid & 127, half = tid >> 7;
  const int64_t mp = m0 + p;
  const bool pok = mp < M;
  const int ox = (int)(mp % Wo), oy = (int)((mp / Wo) % Ho), b = (int)(mp / ((int64_t)Wo * Ho));
  const int wrow = tid >> 4, wc4 = (tid & 15) * 4;   // W loader (threads 0..127): row of the chunk, 4 columns
  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  const int cchunks = C / 8;
  for (int t = 0; t < taps.n; ++t) {
    const int iy = oy * stride + taps.dy[t], ix = ox * stride + taps.dx[t];
    const bool inside = pok && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const float* xp = x + (((int64_t)b * H + iy) * W + ix) * C + 4 * half;
    for (int cc = 0; cc < cchunks; ++cc) {
      v4f av = {0.f, 0.f, 0.f, 0.f};
      if (inside) av = *(const v4f*)(xp + cc * 8);
      v4f wv = {0.f, 0.f, 0.f, 0.f};
      if (tid < 128 && n0 + wc4 < N) wv = *(const v4f*)(Wk + ((int64_t)(t * C + cc * 8 + wrow)) * N + n0 + wc4);
      __syncthreads();   // previous chunk's fragments have been read
#pragma unroll
      for (int j = 0; j < 4; ++j) As[4 * half + j][p] = av[j];
      if (tid < 128) *(v4f*)&Ws[wrow][wc4] = wv;
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float a = As[2 * kk + (lane >> 5)][wid * 32 + (lane & 31)];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float w = Ws[2 * kk + (lane >> 5)][j * 32 + (lane & 31)];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w, acc[j], 0, 0, 0);   // D[pixel][channel]
        }
      }
    }
  }
  // D layout: lane holds channel (lane & 31) for pixels (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + j * 32 + (lane & 31);
    if (n >= N) continue;
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t m = m0 + wid * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      if (m >= M) continue;
      float v = acc[j][e] + bv;
      if (relu) v = fmaxf(v, 0.f);
      if (residual) v += residual[m * N + n];
      out[m * N + n] = v;
    }
  }
}
extern "C" int dmi_conv2d_f32(const float* x, int B, int H, int W, int C, int Ho, int Wo, int stride, int ntaps, const int* dy,
                              const int* dx, const float* Wk, const float* bias, const float* residual, float* out, int N,
                              int relu, void* stream) {
  DMI_REQUIRE(x && Wk && out && dy && dx, "conv2d_f32: null pointer");
  DMI_REQUIRE(C % 8 == 0 && N % 4 == 0 && ntaps >= 1 && ntaps <= MAX_TAPS && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && stride >= 1,
              "conv2d_f32: need C%%8==0, N%%4==0, 1..16 taps (C=%d N=%d ntaps=%d)", C, N, ntaps);
  DMI_REQUIRE((((uintptr_t)x | (uintptr_t)Wk | (uintptr_t)out) & 15) == 0, "conv2d_f32: operands must be 16-byte aligned");
  TapList t;
  t.n = ntaps;
  for (int i = 0; i < ntaps; ++i) { t.dy[i] = dy[i]; t.dx[i] = dx[i]; }
  const int64_t M = (int64_t)B * Ho * Wo;
  conv2d_f32_kernel<<<dim3((unsigned)cdiv64(M, 128), (unsigned)((N + 63) / 64)), dim3(256), 0, (hipStream_t)stream>>>(
      x, Wk, bias, residual, out, t, B, H, W, C, Ho, Wo, stride, N, relu);
  DMI_CHECK_LAUNCH("conv2d_f32");
  return DMI_OK;
}

// tf.space_to_depth / tf.depth_to_space (NHWC, block size s; src/vae_tf/models.py:85-86,158-161), fp32, with channel
// padding: stacked[b, y, x, (dy*s + dx)*C + c] = img[b, y*s + dy, x*s + dx, c] for c < C; stacked channels [s*s*C, Cp) = 0.
__global__ __launch_bounds__(256) void space_to_depth_kernel(const float* __restrict__ img, float* __restrict__ out, int B, int Hs,
                                                             int Ws_, int C, int s, int Cp) {
  const int64_t total = (int64_t)B * Hs * Ws_ * Cp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cp = (int)(i % Cp);
    const int64_t pix = i / Cp;
    float v = 0.f;
    if (cp < s * s * C) {
      const int c = cp % C, blk = cp / C, dy = blk / s, dx = blk % s;
      const int xx = (int)(pix % Ws_), yy = (int)((pix / Ws_) % Hs), b = (int)(pix / ((int64_t)Ws_ * Hs));
      v = img[(((int64_t)b * Hs * s + yy * s + dy) * (Ws_ * s) + xx * s + dx) * C + c];
    }
    out[i] = v;
  }
}
__global__ __launch_bounds__(256) void depth_to_space_kernel(const float* __restrict__ stacked, float* __restrict__ img, int B,
                                                             int Hs, int Ws_, int C, int s, int Cp) {
  const int64_t total = (int64_t)B * Hs * s * Ws_ * s * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t pix = i / C;
    const int X = (int)(pix % (Ws_ * s)), Y = (int)((pix / (Ws_ * s)) % (Hs * s)), b = (int)(pix / ((int64_t)Ws_ * s * Hs * s));
    const int yy = Y / s, dy = Y % s, xx = X / s, dx = X % s;
    img[i] = stacked[(((int64_t)b * Hs + yy) * Ws_ + xx) * Cp + (dy * s + dx) * C + c];
  }
}
extern "C" int dmi_space_to_depth_f32(const float* img, float* stacked, int B, int Hs, int Ws_, int C, int s, int Cp, void* stream) {
  DMI_REQUIRE(img && stacked && B > 0 && Hs > 0 && Ws_ > 0 && C > 0 && s >= 1 && Cp >= s * s * C, "space_to_depth: bad args");
  int64_t blocks = cdiv64((int64_t)B * Hs * Ws_ * Cp, 256);
  if (blocks > 16384) blocks = 16384;
  space_to_depth_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(img, stacked, B, Hs, Ws_, C, s, Cp);
  DMI_CHECK_LAUNCH("space_to_depth");
  return DMI_OK;
}
extern "C" int dmi_depth_to_space_f32(const float* stacked, float* img, int B, int Hs, int Ws_, int C, int s, int Cp, void* stream) {
  DMI_REQUIRE(img && stacked && B > 0 && Hs > 0 && Ws_ > 0 && C > 0 && s >= 1 && Cp >= s * s * C, "depth_to_space: bad args");
  int64_t blocks = cdiv64((int64_t)B * Hs * s * Ws_ * s * C, 256);
  if (blocks > 16384) blocks = 16384;
  depth_to_space_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(stacked, img, B, Hs, Ws_, C, s, Cp);
  DMI_CHECK_LAUNCH("depth_to_space");
  return DMI_OK;
}

// =====================================================================================
// Vector-quantised bottleneck (project extension; DESIGN.md §4 "VAE: vector quantisation").  X = x_enc bf16 [M, D], Cb the bf16
// codebook, codebook_t [T, D] its transpose (code k = row k), h[k] = 1/2 sum_j Cb[j,k]^2:
//   s[m,k] = sum_j X[m,j] Cb[j,k] - h[k]     idx[m] = lowest k among the maxima of s[m,:]     xq[m,:] = Cb[:, idx[m]]
//   Lq = (1/(M D)) sum_m ||X[m] - xq[m]||^2   dX = bf16(d + (2 beta/(M D)) (X - xq))   dC[:,k] = (2/(M D)) sum_{m: idx[m]=k} (Cb[:,k] - X[m,:])
// Every sum has a fixed order (no float atomics): two runs give equal bits.
// =====================================================================================
#define VQ_MAX_T 4096
#define VQ_MAX_D 512
#define VQ_ROWS 64

// h[k] from the bf16 transpose: one wave per code, a lane squares one 16-byte piece (D <= 512: at most 64 pieces), wave_sum.
__global__ __launch_bounds__(256) void vq_half_norms_bf16_kernel(const bf16_t* __restrict__ cbt, int ldc, float* __restrict__ h, int T, int D) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= T) return;
  float a = 0.f;
  if (lane < D / 8) {
    float f[8];
    unpack8(*(const u32x4*)(cbt + (int64_t)k * ldc + lane * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) a += f[e] * f[e];
  }
  a = wave_sum(a);
  if (lane == 0) h[k] = 0.5f * a;
}
// h[k] from the fp32 masters [D, T]: one thread per code, rows top to bottom
__global__ __launch_bounds__(256) void vq_half_norms_f32_kernel(const float* __restrict__ cb, float* __restrict__ h, int T, int D) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= T) return;
  float a = 0.f;
  for (int j = 0; j < D; ++j) {
    const float v = cb[(int64_t)j * T + k];
    a += v * v;
  }
  h[k] = 0.5f * a;
}
extern "C" int dmi_vq_half_norms(const uint16_t* codebook_t, int ldc, const float* codebook_f32, float* h, int T, int D, void* stream) {
  DMI_REQUIRE(h, "vq_half_norms: null pointer (h)");
  DMI_REQUIRE((codebook_t != nullptr) != (codebook_f32 != nullptr), "vq_half_norms: give exactly one of codebook_t (bf16 [T, ldc]) and codebook_f32 (fp32 [D, T])");
  DMI_REQUIRE(T > 0 && D > 0, "vq_half_norms: T and D must be positive (T=%d D=%d)", T, D);
  if (codebook_t) {
    DMI_REQUIRE(D % 8 == 0 && ldc % 8 == 0 && ldc >= D && (((uintptr_t)codebook_t) & 15) == 0, "vq_half_norms: codebook_t needs D%%8==0, ldc%%8==0, ldc>=D, 16-byte alignment (D=%d ldc=%d)", D, ldc);
    if (D > VQ_MAX_D) {
      dmi_set_error("vq_half_norms: D = %d is above %d (one 16-byte piece per lane)", D, VQ_MAX_D);
      return DMI_ERR_UNSUPPORTED;
    }
    vq_half_norms_bf16_kernel<<<dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(codebook_t, ldc, h, T, D);
  } else {
    vq_half_norms_f32_kernel<<<dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(codebook_f32, h, T, D);
  }
  DMI_CHECK_LAUNCH("vq_half_norms");
  return DMI_OK;
}

// scores[m,k] -= h[k]  (fp32 [M, T]; behind the logits product when DALL-E tokenises)
__global__ __launch_bounds__(256) void vq_scores_bias_kernel(float* __restrict__ s, const float* __restrict__ h, int64_t M, int T) {
  const int t4 = T / 4;
  const int64_t total = M * t4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % t4);
    f32x4 v = *(f32x4*)(s + i * 4);
    const f32x4 hv = *(const f32x4*)(h + c * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] -= hv[e];
    *(f32x4*)(s + i * 4) = v;
  }
}
extern "C" int dmi_vq_scores_bias(float* scores, const float* h, int64_t M, int T, void* stream) {
  DMI_REQUIRE(scores && h, "vq_scores_bias: null pointer");
  DMI_REQUIRE(M > 0, "vq_scores_bias: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && T % 4 == 0, "vq_scores_bias: T must be a positive multiple of 4 (T=%d)", T);
  DMI_REQUIRE(((((uintptr_t)scores) | ((uintptr_t)h)) & 15) == 0, "vq_scores_bias: scores and h must be 16-byte aligned");
  int64_t blocks = cdiv64(M * (T / 4), 256);
  if (blocks > 16384) blocks = 16384;
  vq_scores_bias_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(scores, h, M, T);
  DMI_CHECK_LAUNCH("vq_scores_bias");
  return DMI_OK;
}

// (value descending, index ascending)
__device__ __forceinline__ void vq_take(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

// The assignment: a block owns 64 rows of X, staged once in LDS ([64][D] bf16, 16-byte pieces XOR-swizzled by row & 7), and sweeps
// the codebook in tiles of 256 codes, 64 per wave, read straight from global memory (each wave reads its own codes: no LDS round
// trip, no barrier in the sweep).  MFMA A = codes, B = rows of X, so a lane holds D[code 4g + r][row c] (c = lane & 15,
// g = lane >> 4): four codes of ONE row per accumulator, and the running (best, index) stays per lane.  A 64-wide k-chunk is two
// MFMAs; a load instruction of a wave takes 64 contiguous bytes from each of 16 code rows (lane group g the 16 bytes at 16g).
// The accumulation order of a score depends on D alone, never on the tile: equal columns give equal bits.
// The code fragments of the next k-chunk are fetched under the current chunk's 32 MFMAs.
__global__ __launch_bounds__(256) void vq_assign_kernel(const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ cbt, int ldc,
                                                        const float* __restrict__ h, int* __restrict__ idx, bf16_t* __restrict__ xq,
                                                        int ldq, float* __restrict__ score, int64_t M, int T, int D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vq_smem[];
  u32x4* xs = (u32x4*)vq_smem;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  constexpr int RB = 4, ROWS = VQ_ROWS;      // RB row blocks of 16
  const int64_t m0 = (int64_t)blockIdx.x * ROWS;
  const int cpr = D / 8;       // 16-byte pieces per row (a multiple of 8)
  for (int i = tid; i < ROWS * cpr; i += 256) {
    const int r = i / cpr, p = i % cpr;
    u32x4 v = {0, 0, 0, 0};
    if (m0 + r < M) v = *(const u32x4*)(x + (m0 + r) * ldx + p * 8);
    xs[r * cpr + (p ^ (r & 7))] = v;
  }
  __syncthreads();
  float best[RB];
  int bidx[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    best[rb] = -INFINITY;
    bidx[rb] = 0x7fffffff;
  }
  const int nk = D / 64;
  for (int t0 = wid * 64; t0 < T; t0 += 256) {
    f32x4 acc[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16_t* bp = cbt + (int64_t)(t0 + c) * ldc + g * 8;
    u32x4 bcur[4][2], bnxt[4][2];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      bcur[cb][0] = *(const u32x4*)(bp + (int64_t)cb * 16 * ldc);
      bcur[cb][1] = *(const u32x4*)(bp + (int64_t)cb * 16 * ldc + 32);
    }
    for (int kc = 0; kc < nk; ++kc) {
      if (kc + 1 < nk) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          bnxt[cb][0] = *(const u32x4*)(bp + (int64_t)cb * 16 * ldc + (kc + 1) * 64);
          bnxt[cb][1] = *(const u32x4*)(bp + (int64_t)cb * 16 * ldc + (kc + 1) * 64 + 32);
        }
      }
      u32x4 a[RB][2];
      const int p0 = kc * 8 + g;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int r = rb * 16 + c;
        a[rb][0] = xs[r * cpr + (p0 ^ (r & 7))];
        a[rb][1] = xs[r * cpr + ((p0 + 4) ^ (r & 7))];
      }
      MFMA_PRIO(1);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bcur[cb][j]), __builtin_bit_cast(bf16x8, a[rb][j]),
                                                                  acc[rb][cb], 0, 0, 0);
      MFMA_PRIO(0);
      if (kc + 1 < nk) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          bcur[cb][0] = bnxt[cb][0];
          bcur[cb][1] = bnxt[cb][1];
        }
      }
    }
    // ascending codes within the lane: cb, then the accumulator register; strict > keeps the first maximum
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int k0 = t0 + cb * 16 + g * 4;
      const f32x4 hv = *(const f32x4*)(h + k0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const float sc = acc[rb][cb][e] - hv[e];
          if (sc > best[rb]) {
            best[rb] = sc;
            bidx[rb] = k0 + e;
          }
        }
    }
  }
  // the four lane groups of a row, then the four waves
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ov = __shfl_xor(best[rb], o, 64);
      const int oi = __shfl_xor(bidx[rb], o, 64);
      vq_take(best[rb], bidx[rb], ov, oi);
    }
  __syncthreads();             // every wave has left the X tile: its storage carries the reduction from here on
  float* redv = (float*)vq_smem;          // [4][ROWS]
  int* redi = (int*)(redv + 4 * ROWS);    // [4][ROWS]
  int* sidx = redi + 4 * ROWS;            // [ROWS]   (36 ROWS bytes in all: under the smallest tile, ROWS x 64 x 2)
  if (g == 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      redv[wid * ROWS + rb * 16 + c] = best[rb];
      redi[wid * ROWS + rb * 16 + c] = bidx[rb];
    }
  }
  __syncthreads();
  if (tid < ROWS) {
    float bv = redv[tid];
    int bi = redi[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) vq_take(bv, bi, redv[w * ROWS + tid], redi[w * ROWS + tid]);
    if (bi < 0 || bi >= T) bi = 0;        // no score compared above -inf (NaN rows): a valid code all the same
    sidx[tid] = bi;
    if (m0 + tid < M) {
      idx[m0 + tid] = bi;
      if (score) score[m0 + tid] = bv;
    }
  }
  if (!xq) return;
  __syncthreads();
  for (int i = tid; i < ROWS * cpr; i += 256) {
    const int r = i / cpr, p = i % cpr;
    if (m0 + r < M) *(u32x4*)(xq + (m0 + r) * ldq + p * 8) = *(const u32x4*)(cbt + (int64_t)sidx[r] * ldc + p * 8);
  }
}
extern "C" int dmi_vq_assign(const uint16_t* x, int ldx, const uint16_t* codebook_t, int ldc, const float* h, int32_t* idx, uint16_t* xq,
                             int ldq, float* score, int64_t M, int T, int D, void* stream) {
  DMI_REQUIRE(x && codebook_t && h && idx, "vq_assign: null pointer (x, codebook_t, h or idx)");
  DMI_REQUIRE(M > 0, "vq_assign: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && D > 0, "vq_assign: T and D must be positive (T=%d D=%d)", T, D);
  DMI_REQUIRE(ldx >= D && ldx % 8 == 0, "vq_assign: ldx must be a multiple of 8 and at least D (ldx=%d D=%d)", ldx, D);
  DMI_REQUIRE(ldc >= D && ldc % 8 == 0, "vq_assign: ldc must be a multiple of 8 and at least D (ldc=%d D=%d)", ldc, D);
  DMI_REQUIRE(!xq || (ldq >= D && ldq % 8 == 0), "vq_assign: ldq must be a multiple of 8 and at least D (ldq=%d D=%d)", ldq, D);
  DMI_REQUIRE(((((uintptr_t)x) | ((uintptr_t)codebook_t) | ((uintptr_t)h) | ((uintptr_t)xq)) & 15) == 0,
              "vq_assign: x, codebook_t, h and xq must be 16-byte aligned");
  if (D % 64 != 0 || D > VQ_MAX_D || T % 64 != 0 || T > VQ_MAX_T) {
    dmi_set_error("vq_assign: needs D %% 64 == 0, D <= %d, T %% 64 == 0, T <= %d (D=%d T=%d)", VQ_MAX_D, VQ_MAX_T, D, T);
    return DMI_ERR_UNSUPPORTED;
  }
  vq_assign_kernel<<<dim3((unsigned)cdiv64(M, VQ_ROWS)), dim3(256), VQ_ROWS * D * 2, (hipStream_t)stream>>>(x, ldx, codebook_t, ldc, h, idx,
                                                                                                      xq, ldq, score, M, T, D);
  DMI_CHECK_LAUNCH("vq_assign");
  return DMI_OK;
}

// xq rows by index (decode_tokens); an id outside [0, T) gives a zero row and reads nothing
__global__ __launch_bounds__(256) void vq_gather_kernel(const bf16_t* __restrict__ cbt, int ldc, const int* __restrict__ idx,
                                                        bf16_t* __restrict__ out, int ldo, int64_t M, int T, int D) {
  const int cpr = D / 8;
  const int64_t total = M * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % cpr);
    const int64_t m = i / cpr;
    const int k = idx[m];
    u32x4 v = {0, 0, 0, 0};
    if (k >= 0 && k < T) v = *(const u32x4*)(cbt + (int64_t)k * ldc + p * 8);
    *(u32x4*)(out + m * ldo + p * 8) = v;
  }
}
extern "C" int dmi_vq_gather(const uint16_t* codebook_t, int ldc, const int32_t* idx, uint16_t* out, int ldo, int64_t M, int T, int D,
                             void* stream) {
  DMI_REQUIRE(codebook_t && idx && out, "vq_gather: null pointer");
  DMI_REQUIRE(M > 0, "vq_gather: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && D > 0 && D % 8 == 0, "vq_gather: T must be positive and D a positive multiple of 8 (T=%d D=%d)", T, D);
  DMI_REQUIRE(ldc >= D && ldc % 8 == 0 && ldo >= D && ldo % 8 == 0, "vq_gather: ldc and ldo must be multiples of 8 and at least D (ldc=%d ldo=%d D=%d)", ldc, ldo, D);
  DMI_REQUIRE(((((uintptr_t)codebook_t) | ((uintptr_t)out)) & 15) == 0, "vq_gather: codebook_t and out must be 16-byte aligned");
  int64_t blocks = cdiv64(M * (D / 8), 256);
  if (blocks > 16384) blocks = 16384;
  vq_gather_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(codebook_t, ldc, idx, out, ldo, M, T, D);
  DMI_CHECK_LAUNCH("vq_gather");
  return DMI_OK;
}

// Lq: a thread sums the squares of its 16-byte pieces in order, wave_sum, four waves, then dmi_sum_f32 over the block partials
#define VQ_LOSS_BLOCKS 1024
__global__ __launch_bounds__(256) void vq_loss_kernel(const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ xq, int ldq,
                                                      float* __restrict__ part, int64_t M, int D) {
  __shared__ float sm[4];
  const int cpr = D / 8;
  const int64_t total = M * cpr;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % cpr);
    const int64_t m = i / cpr;
    float a[8], b[8];
    unpack8(*(const u32x4*)(x + m * ldx + p * 8), a);
    unpack8(*(const u32x4*)(xq + m * ldq + p * 8), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = a[e] - b[e];
      acc += d * d;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
extern "C" int64_t dmi_vq_loss_workspace_bytes(void) { return VQ_LOSS_BLOCKS * 4; }
extern "C" int dmi_vq_loss(const uint16_t* x, int ldx, const uint16_t* xq, int ldq, float* loss, int64_t M, int D, void* workspace,
                           void* stream) {
  DMI_REQUIRE(x && xq && loss && workspace, "vq_loss: null pointer");
  DMI_REQUIRE(M > 0, "vq_loss: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(D > 0 && D % 8 == 0, "vq_loss: D must be a positive multiple of 8 (D=%d)", D);
  DMI_REQUIRE(ldx >= D && ldx % 8 == 0 && ldq >= D && ldq % 8 == 0, "vq_loss: ldx and ldq must be multiples of 8 and at least D (ldx=%d ldq=%d D=%d)", ldx, ldq, D);
  DMI_REQUIRE(((((uintptr_t)x) | ((uintptr_t)xq) | ((uintptr_t)workspace)) & 15) == 0, "vq_loss: x, xq and workspace must be 16-byte aligned");
  vq_loss_kernel<<<dim3(VQ_LOSS_BLOCKS), dim3(256), 0, (hipStream_t)stream>>>(x, ldx, xq, ldq, (float*)workspace, M, D);
  DMI_CHECK_LAUNCH("vq_loss");
  return dmi_sum_f32((const float*)workspace, VQ_LOSS_BLOCKS, (float)(1.0 / ((double)M * (double)D)), loss, stream);
}

// dX = bf16(d + a (X - xq)), a = 2 beta / (M D); a == 0 copies d (so that -0 stays -0)
__global__ __launch_bounds__(256) void vq_bwd_x_kernel(const bf16_t* __restrict__ d, int ldd, const bf16_t* __restrict__ x, int ldx,
                                                       const bf16_t* __restrict__ xq, int ldq, bf16_t* __restrict__ dx, int lddx,
                                                       int64_t M, int D, float a) {
  const int cpr = D / 8;
  const int64_t total = M * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % cpr);
    const int64_t m = i / cpr;
    u32x4 dv = *(const u32x4*)(d + m * ldd + p * 8);
    if (a != 0.f) {
      float fd[8], fx[8], fq[8];
      unpack8(dv, fd);
      unpack8(*(const u32x4*)(x + m * ldx + p * 8), fx);
      unpack8(*(const u32x4*)(xq + m * ldq + p * 8), fq);
#pragma unroll
      for (int e = 0; e < 8; ++e) fd[e] = fd[e] + a * (fx[e] - fq[e]);
      dv = pack8(fd);
    }
    *(u32x4*)(dx + m * lddx + p * 8) = dv;
  }
}
extern "C" int dmi_vq_bwd_x(const uint16_t* d, int ldd, const uint16_t* x, int ldx, const uint16_t* xq, int ldq, uint16_t* dx, int lddx,
                            int64_t M, int D, float beta, void* stream) {
  DMI_REQUIRE(d && x && xq && dx, "vq_bwd_x: null pointer");
  DMI_REQUIRE(M > 0, "vq_bwd_x: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(D > 0 && D % 8 == 0, "vq_bwd_x: D must be a positive multiple of 8 (D=%d)", D);
  DMI_REQUIRE(beta >= 0.f && beta <= 3.0e38f, "vq_bwd_x: beta must be finite and >= 0 (beta=%g)", (double)beta);
  DMI_REQUIRE(ldd >= D && ldd % 8 == 0 && ldx >= D && ldx % 8 == 0 && ldq >= D && ldq % 8 == 0 && lddx >= D && lddx % 8 == 0,
              "vq_bwd_x: ldd, ldx, ldq and lddx must be multiples of 8 and at least D (D=%d)", D);
  DMI_REQUIRE(((((uintptr_t)d) | ((uintptr_t)x) | ((uintptr_t)xq) | ((uintptr_t)dx)) & 15) == 0, "vq_bwd_x: operands must be 16-byte aligned");
  const float a = (float)(2.0 * (double)beta / ((double)M * (double)D));
  int64_t blocks = cdiv64(M * (D / 8), 256);
  if (blocks > 16384) blocks = 16384;
  vq_bwd_x_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(d, ldd, x, ldx, xq, ldq, dx, lddx, M, D, a);
  DMI_CHECK_LAUNCH("vq_bwd_x");
  return DMI_OK;
}

// dC: no sort and no workspace.  A block owns eight codes, one per wave; every wave walks idx (512 rows per round, eight per lane,
// the same lines for the eight waves of the block), ballots its code's rows and adds Cb[:,k] - X[m,:] for them in a fixed order
// (element slot 0..7 of the round, then lane): lane p keeps the eight channels of piece p in registers.  A code nobody picked
// keeps its zeros.  The eight columns go through LDS ([code][channel], conflict-free both ways) so that a row of the [D, T] gradient
// is written 32 bytes at a time.
__global__ __launch_bounds__(512) void vq_codebook_grad_kernel(const bf16_t* __restrict__ x, int ldx, const int* __restrict__ idx,
                                                               const bf16_t* __restrict__ cbt, int ldc, float* __restrict__ dC,
                                                               int64_t M, int T, int D, float scale) {
  __shared__ float sm[8][VQ_MAX_D];      // [code of the block][channel]: a lane writes its 32 bytes, a thread reads one float per code
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int k = blockIdx.x * 8 + wid;           // T % 8 == 0
  const bool active = lane < D / 8;
  float cb[8], acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cb[e] = acc[e] = 0.f;
  if (active) unpack8(*(const u32x4*)(cbt + (int64_t)k * ldc + lane * 8), cb);
  for (int64_t base = 0; base < M; base += 512) {
    int v[8];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t m4 = base + q * 256 + lane * 4;
      if (m4 + 3 < M) {
        const u32x4 t = *(const u32x4*)(idx + m4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q * 4 + e] = (int)t[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q * 4 + e] = (m4 + e < M) ? idx[m4 + e] : -1;
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      unsigned long long mask = __ballot(v[s] == k);
      const int64_t row0 = base + (s >> 2) * 256 + (s & 3);
      while (mask) {
        const int b0 = __ffsll(mask) - 1;
        mask &= mask - 1;
        int b1 = -1;
        if (mask) {
          b1 = __ffsll(mask) - 1;
          mask &= mask - 1;
        }
        if (active) {
          float f0[8], f1[8];
          const u32x4 r0 = *(const u32x4*)(x + (row0 + 4 * b0) * ldx + lane * 8);
          u32x4 r1 = {0, 0, 0, 0};
          if (b1 >= 0) r1 = *(const u32x4*)(x + (row0 + 4 * b1) * ldx + lane * 8);
          unpack8(r0, f0);
          unpack8(r1, f1);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += cb[e] - f0[e];
          if (b1 >= 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += cb[e] - f1[e];
          }
        }
      }
    }
  }
  if (active) {
    *(f32x4*)&sm[wid][lane * 8] = f32x4{acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale};
    *(f32x4*)&sm[wid][lane * 8 + 4] = f32x4{acc[4] * scale, acc[5] * scale, acc[6] * scale, acc[7] * scale};
  }
  __syncthreads();
  if (tid < D) {
    float* dst = dC + (int64_t)tid * T + blockIdx.x * 8;
    *(f32x4*)dst = f32x4{sm[0][tid], sm[1][tid], sm[2][tid], sm[3][tid]};
    *(f32x4*)(dst + 4) = f32x4{sm[4][tid], sm[5][tid], sm[6][tid], sm[7][tid]};
  }
}
extern "C" int64_t dmi_vq_codebook_grad_workspace_bytes(int64_t M, int T, int D) {
  (void)M; (void)T; (void)D;
  return 0;       // the ballot walk needs none; the query stays so that another method can have one
}
extern "C" int dmi_vq_codebook_grad(const uint16_t* x, int ldx, const int32_t* idx, const uint16_t* codebook_t, int ldc, float* dC,
                                    int64_t M, int T, int D, void* workspace, void* stream) {
  (void)workspace;
  DMI_REQUIRE(x && idx && codebook_t && dC, "vq_codebook_grad: null pointer (x, idx, codebook_t or dC)");
  DMI_REQUIRE(M > 0, "vq_codebook_grad: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && D > 0, "vq_codebook_grad: T and D must be positive (T=%d D=%d)", T, D);
  DMI_REQUIRE(ldx >= D && ldx % 8 == 0 && ldc >= D && ldc % 8 == 0, "vq_codebook_grad: ldx and ldc must be multiples of 8 and at least D (ldx=%d ldc=%d D=%d)", ldx, ldc, D);
  DMI_REQUIRE(((((uintptr_t)x) | ((uintptr_t)idx) | ((uintptr_t)codebook_t) | ((uintptr_t)dC)) & 15) == 0,
              "vq_codebook_grad: x, idx, codebook_t and dC must be 16-byte aligned");
  if (D % 8 != 0 || D > VQ_MAX_D || T % 8 != 0 || T > VQ_MAX_T) {
    dmi_set_error("vq_codebook_grad: needs D %% 8 == 0, D <= %d, T %% 8 == 0, T <= %d (D=%d T=%d)", VQ_MAX_D, VQ_MAX_T, D, T);
    return DMI_ERR_UNSUPPORTED;
  }
  const float scale = (float)(2.0 / ((double)M * (double)D));
  vq_codebook_grad_kernel<<<dim3((unsigned)(T / 8)), dim3(512), 0, (hipStream_t)stream>>>(x, ldx, idx, codebook_t, ldc, dC, M, T, D, scale);
  DMI_CHECK_LAUNCH("vq_codebook_grad");
  return DMI_OK;
}

// ------------------------------------------------------------------ EMA codebook (DESIGN.md §4 "VAE: EMA codebook and restarts")
// Cluster sums s[k] = sum_{idx[m]=k} X[m] and counts n[k].  The ballot walk of vq_codebook_grad_kernel, cut into row chunks of
// VQ_CS_CHUNK: block (x, y) owns eight codes (one per wave) and the rows [y CHUNK, (y+1) CHUNK); a wave ballots its code's rows in
// row order and adds them in that order, up to four row loads in flight, lane p holding the eight channels of piece p.  The next
// round's idx is loaded before this round's rows.  One chunk: sums / counts are written at once, [T, D] row-major, a row per wave.
// More chunks: partial sums go to the workspace ([chunk][T][D], a code the chunk does not hold is not written) and
// cluster_sums_combine_kernel adds them in chunk order, skipping the chunks whose count is 0.  Fixed order, no float atomics.
#define VQ_CS_CHUNK 4096
#define VQ_CS_MAX_CHUNKS 8
__device__ __forceinline__ void cluster_load_idx(const int* __restrict__ idx, int64_t base, int64_t end, int lane, int* v) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t m4 = base + q * 256 + lane * 4;
    if (m4 + 3 < end) {
      const u32x4 t = *(const u32x4*)(idx + m4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q * 4 + e] = (int)t[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q * 4 + e] = (m4 + e < end) ? idx[m4 + e] : -1;
    }
  }
}
__global__ __launch_bounds__(512) void cluster_sums_walk_kernel(const bf16_t* __restrict__ x, int ldx, const int* __restrict__ idx,
                                                              float* __restrict__ out, int* __restrict__ cnt, int64_t M, int T, int D,
                                                              int64_t rows_per_chunk, int skip_empty) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int k = blockIdx.x * 8 + wid;           // T % 8 == 0
  const bool active = lane < D / 8;
  const int64_t begin = (int64_t)blockIdx.y * rows_per_chunk;       // a multiple of 512: the 16-byte idx loads stay aligned
  const int64_t end = begin + rows_per_chunk < M ? begin + rows_per_chunk : M;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  int n = 0;
  int v[8], nv[8];
  cluster_load_idx(idx, begin, end, lane, v);
  for (int64_t base = begin; base < end; base += 512) {
    if (base + 512 < end) cluster_load_idx(idx, base + 512, end, lane, nv);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      unsigned long long mask = __ballot(v[s] == k);
      n += __popcll(mask);
      const int64_t row0 = base + (s >> 2) * 256 + (s & 3);
      while (mask) {
        int b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          b[j] = -1;
          if (mask) {
            b[j] = __ffsll(mask) - 1;
            mask &= mask - 1;
          }
        }
        if (active) {
          u32x4 r[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            r[j] = u32x4{0, 0, 0, 0};
            if (b[j] >= 0) r[j] = *(const u32x4*)(x + (row0 + 4 * b[j]) * ldx + lane * 8);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (b[j] >= 0) {
              float f[8];
              unpack8(r[j], f);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[e] += f[e];
            }
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) v[s] = nv[s];
  }
  if (lane == 0) cnt[(int64_t)blockIdx.y * T + k] = n;
  if (active && !(skip_empty && n == 0)) {
    float* dst = out + ((int64_t)blockIdx.y * T + k) * D + lane * 8;
    *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(dst + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}
// one wave per code: sums[k] = partial[0][k] + partial[1][k] + ... over the chunks that hold the code, counts[k] = their total
__global__ __launch_bounds__(256) void cluster_sums_combine_kernel(const float* __restrict__ part, const int* __restrict__ pcnt,
                                                                 float* __restrict__ sums, int* __restrict__ counts, int T, int D, int P) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);      // T % 8 == 0
  const bool active = lane < D / 8;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  int n = 0;
  for (int p = 0; p < P; ++p) {
    const int c = pcnt[(int64_t)p * T + k];
    n += c;
    if (c > 0 && active) {
      const float* src = part + ((int64_t)p * T + k) * D + lane * 8;
      const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] += a[e];
        acc[4 + e] += b[e];
      }
    }
  }
  if (lane == 0) counts[k] = n;
  if (active) {
    float* dst = sums + (int64_t)k * D + lane * 8;
    *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(dst + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}
static inline int cluster_chunks(int64_t M) {
  const int64_t p = cdiv64(M, VQ_CS_CHUNK);
  return (int)(p < VQ_CS_MAX_CHUNKS ? p : VQ_CS_MAX_CHUNKS);
}
extern "C" int64_t dmi_vq_cluster_sums_workspace_bytes(int64_t M, int T, int D) {
  if (M <= 0 || T <= 0 || D <= 0) return 0;
  const int P = cluster_chunks(M);
  return P == 1 ? 0 : (int64_t)P * T * ((int64_t)D + 1) * 4;       // [P][T][D] partial sums, then [P][T] partial counts
}
extern "C" int dmi_vq_cluster_sums(const uint16_t* x, int ldx, const int32_t* idx, float* sums, int32_t* counts, int64_t M, int T, int D,
                                   void* workspace, void* stream) {
  DMI_REQUIRE(x && idx && sums && counts, "vq_cluster_sums: null pointer (x, idx, sums or counts)");
  DMI_REQUIRE(M > 0, "vq_cluster_sums: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && D > 0, "vq_cluster_sums: T and D must be positive (T=%d D=%d)", T, D);
  DMI_REQUIRE(ldx >= D && ldx % 8 == 0, "vq_cluster_sums: ldx must be a multiple of 8 and at least D (ldx=%d D=%d)", ldx, D);
  DMI_REQUIRE(((((uintptr_t)x) | ((uintptr_t)idx) | ((uintptr_t)sums) | ((uintptr_t)counts) | ((uintptr_t)workspace)) & 15) == 0,
              "vq_cluster_sums: x, idx, sums, counts and workspace must be 16-byte aligned");
  if (D % 8 != 0 || D > VQ_MAX_D || T % 8 != 0 || T > VQ_MAX_T) {
    dmi_set_error("vq_cluster_sums: needs D %% 8 == 0, D <= %d, T %% 8 == 0, T <= %d (D=%d T=%d)", VQ_MAX_D, VQ_MAX_T, D, T);
    return DMI_ERR_UNSUPPORTED;
  }
  const int P = cluster_chunks(M);
  hipStream_t st = (hipStream_t)stream;
  if (P == 1) {
    cluster_sums_walk_kernel<<<dim3((unsigned)(T / 8), 1), dim3(512), 0, st>>>(x, ldx, idx, sums, counts, M, T, D, M, 0);
    DMI_CHECK_LAUNCH("vq_cluster_sums");
    return DMI_OK;
  }
  DMI_REQUIRE(workspace, "vq_cluster_sums: null pointer (workspace: dmi_vq_cluster_sums_workspace_bytes(M, T, D) bytes at M=%lld)", (long long)M);
  const int64_t rows = cdiv64(cdiv64(M, P), 512) * 512;       // P chunks of whole 512-row rounds cover M; the last may be short
  float* part = (float*)workspace;
  int* pcnt = (int*)(part + (int64_t)P * T * D);
  cluster_sums_walk_kernel<<<dim3((unsigned)(T / 8), (unsigned)P), dim3(512), 0, st>>>(x, ldx, idx, part, pcnt, M, T, D, rows, 1);
  DMI_CHECK_LAUNCH("vq_cluster_sums");
  cluster_sums_combine_kernel<<<dim3((unsigned)(T / 4)), dim3(256), 0, st>>>(part, pcnt, sums, counts, T, D, P);
  DMI_CHECK_LAUNCH("vq_cluster_sums");
  return DMI_OK;
}

// EMA update and dead-code restart of eight codes per block.  Wave w owns code k = 8 blockIdx.x + w: N, idle and the [T, D] row of S
// (lane p the eight channels of piece p); the new code goes through LDS so that thread c rewrites C[c, k0 .. k0 + 8) of the [D, T]
// master (32 bytes) and of its bf16 copy (16 bytes), taking the old bits for the codes that did not change.  Every product is
// rounded on its own (contraction off): a numpy float32 restatement gives the same N and S.
__global__ __launch_bounds__(512) void ema_codebook_step_kernel(float* __restrict__ C, bf16_t* __restrict__ Cb, float* __restrict__ N,
                                                          float* __restrict__ S, int* __restrict__ idle, int* __restrict__ restarts,
                                                          const float* __restrict__ sums, const int* __restrict__ counts,
                                                          const bf16_t* __restrict__ x, int ldx, float g, float w, int restart_after,
                                                          uint64_t seed, int64_t step, const int64_t* __restrict__ step_dev, int64_t M,
                                                          int T, int D) {
#pragma clang fp contract(off)
  __shared__ float sm[8][VQ_MAX_D];
  __shared__ int changed[8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int k = blockIdx.x * 8 + wid;           // T % 8 == 0
  const bool active = lane < D / 8;
  const int n = counts[k];
  float Nk = N[k] * g;
  int id = idle[k];
  if (n > 0) {
    Nk = Nk + w * (float)n;
    id = 0;
  } else {
    id += 1;
  }
  const bool restart = restart_after > 0 && id >= restart_after;
  float c[8], s[8];
  if (active) {
    float* Sk = S + (int64_t)k * D + lane * 8;
    if (restart) {
      if (step_dev) step = *step_dev;
      const uint64_t r = splitmix64(splitmix64(seed) ^ (uint64_t)step);
      const uint64_t m = splitmix64(r + (uint64_t)k) % (uint64_t)M;
      unpack8(*(const u32x4*)(x + (int64_t)m * ldx + lane * 8), c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = c[e];
    } else {
      const f32x4 a = *(const f32x4*)Sk, b = *(const f32x4*)(Sk + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[e] = a[e] * g;
        s[4 + e] = b[e] * g;
      }
      if (n > 0) {
        const float* sk = sums + (int64_t)k * D + lane * 8;
        const f32x4 u = *(const f32x4*)sk, t = *(const f32x4*)(sk + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[e] = s[e] + w * u[e];
          s[4 + e] = s[4 + e] + w * t[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = s[e] / Nk;
      }
    }
    *(f32x4*)Sk = f32x4{s[0], s[1], s[2], s[3]};
    *(f32x4*)(Sk + 4) = f32x4{s[4], s[5], s[6], s[7]};
    if (restart || n > 0) {
      *(f32x4*)&sm[wid][lane * 8] = f32x4{c[0], c[1], c[2], c[3]};
      *(f32x4*)&sm[wid][lane * 8 + 4] = f32x4{c[4], c[5], c[6], c[7]};
    }
  }
  if (lane == 0) {
    N[k] = restart ? 1.f : Nk;
    idle[k] = restart ? 0 : id;
    changed[wid] = (restart || n > 0) ? 1 : 0;
    if (restart) atomicAdd(restarts, 1);       // an integer count: the order of the adds does not show
  }
  __syncthreads();
  if (tid < D) {
    float* dst = C + (int64_t)tid * T + blockIdx.x * 8;
    bf16_t* dstb = Cb + (int64_t)tid * T + blockIdx.x * 8;
    const f32x4 a = *(const f32x4*)dst, b = *(const f32x4*)(dst + 4);
    float o[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    const u32x4 ob = *(const u32x4*)dstb;
    bf16_t q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      q[j] = (bf16_t)((j & 1) ? (ob[j >> 1] >> 16) : (ob[j >> 1] & 0xffffu));
      if (changed[j]) {
        o[j] = sm[j][tid];
        q[j] = f2bf(o[j]);
      }
    }
    *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
    *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
    u32x4 nb;
#pragma unroll
    for (int j = 0; j < 4; ++j) nb[j] = (unsigned)q[2 * j] | ((unsigned)q[2 * j + 1] << 16);
    *(u32x4*)dstb = nb;
  }
}
extern "C" int dmi_vq_ema_step(float* codebook_f32, uint16_t* codebook_bf16, float* N, float* S, int32_t* idle, int32_t* restarts,
                               const float* sums, const int32_t* counts, const uint16_t* x, int ldx, double gamma, int restart_after,
                               uint64_t seed, int64_t step, const int64_t* step_dev, int64_t M, int T, int D, void* stream) {
  DMI_REQUIRE(codebook_f32 && codebook_bf16 && N && S && idle && restarts && sums && counts && x,
              "vq_ema_step: null pointer (codebook_f32, codebook_bf16, N, S, idle, restarts, sums, counts or x)");
  DMI_REQUIRE(M > 0, "vq_ema_step: M must be positive (M=%lld)", (long long)M);
  DMI_REQUIRE(T > 0 && D > 0, "vq_ema_step: T and D must be positive (T=%d D=%d)", T, D);
  DMI_REQUIRE(gamma > 0.0 && gamma < 1.0, "vq_ema_step: gamma must lie strictly between 0 and 1 (gamma=%g)", gamma);
  DMI_REQUIRE(restart_after >= 0, "vq_ema_step: restart_after must be >= 0 (restart_after=%d)", restart_after);
  DMI_REQUIRE(step >= 0, "vq_ema_step: step must be >= 0 (step=%lld)", (long long)step);
  DMI_REQUIRE(ldx >= D && ldx % 8 == 0, "vq_ema_step: ldx must be a multiple of 8 and at least D (ldx=%d D=%d)", ldx, D);
  DMI_REQUIRE(((((uintptr_t)codebook_f32) | ((uintptr_t)codebook_bf16) | ((uintptr_t)S) | ((uintptr_t)sums) | ((uintptr_t)x)) & 15) == 0,
              "vq_ema_step: codebook_f32, codebook_bf16, S, sums and x must be 16-byte aligned");
  DMI_REQUIRE(((((uintptr_t)N) | ((uintptr_t)idle) | ((uintptr_t)restarts) | ((uintptr_t)counts)) & 3) == 0 && (((uintptr_t)step_dev) & 7) == 0,
              "vq_ema_step: N, idle, restarts and counts must be 4-byte aligned, step_dev 8-byte aligned");
  if (D % 8 != 0 || D > VQ_MAX_D || T % 8 != 0 || T > VQ_MAX_T) {
    dmi_set_error("vq_ema_step: needs D %% 8 == 0, D <= %d, T %% 8 == 0, T <= %d (D=%d T=%d)", VQ_MAX_D, VQ_MAX_T, D, T);
    return DMI_ERR_UNSUPPORTED;
  }
  const float g = (float)gamma, w = (float)(1.0 - gamma);
  ema_codebook_step_kernel<<<dim3((unsigned)(T / 8)), dim3(512), 0, (hipStream_t)stream>>>(codebook_f32, codebook_bf16, N, S, idle, restarts, sums, counts,
                                                                                     x, ldx, g, w, restart_after, seed, step, step_dev, M, T, D);
  DMI_CHECK_LAUNCH("vq_ema_step");
  return DMI_OK;
}
