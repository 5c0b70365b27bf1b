// optim.hip -- mtf.optimize.AdafactorOptimizer over the flat parameter buffer (src/optimizers.py:91-97).
//
// One descriptor per REFERENCE variable (q/k/v are column blocks of the fused [d, 3d] matrix, the head's kernel / bias carry pad
// columns past V), DMI_AF_FIELDS int64 each (include/dalle_hip.h).  A step is six launches whatever the layer count; every
// tile launch walks the 64 x 256 tiles of ALL variables:
//   1 af_stats      g, w once: per tile sum g^2 and sum w^2; factored variables also per-tile row sums and column sums of g^2
//   2 af_reduce     per variable: sum of its tile scalars; per 64-entry segment of a factored variable's row / column vector:
//                   the sum of its tile partials (raw sums of g^2, before the clip)
//   3 af_finalize   global sum g^2 -> clip multiplier; vr / vc updated from the raw sums (mean(gc^2 + eps1) = mult^2 * sum / n
//                   + eps1): vr (the shorter vector) with mean(vr) and max(rms(w), eps2) by one block per variable, vc by segments
//   4 af_xsum       per tile sum x^2, x = gc * rsqrt(vr / mean(vr)) * rsqrt(vc)  (or gc * rsqrt(v_new) unfactored)
//   5 af_xfinish    per variable max(1, rms(x))
//   6 af_apply      u = lr * max(rms(w), eps2) * x / max(1, rms(x)); m = b1 m + (1 - b1) u; w -= m (u when b1 = 0); bf16 copy;
//                   v of an unfactored variable written back
// Every reduction runs in a fixed order: no atomics, bit-identical results for identical inputs.  Elements outside the
// variables (pad columns, pad bias entries, alignment gaps) are never read nor written.
#include "common.h"

#define AF_TR 64    // tile rows
#define AF_TC 256   // tile columns: one wave covers a row segment, 4 consecutive columns per lane
#define AF_SEG 64   // entries of a row / column vector per block of af_reduce / af_finalize (a lane each)
#define AF_VS 4     // per-variable scalars in the workspace: sum g^2, sum w^2, mean(vr) or 0, max(rms(w), eps2)

enum {
  F_OFF = 0, F_ROWS, F_COLS, F_LD, F_FACT, F_VR_ROW, F_SLOT_ROW, F_SLOT_COL, F_SLOT_V,   // caller
  F_TILE0, F_NTR, F_NTC, F_SEG0, F_ROWPART, F_COLPART, F_SROW, F_SCOL                   // dmi_adafactor_plan
};
static_assert(F_SCOL + 1 == DMI_AF_FIELDS, "descriptor layout");

struct AfArgs {
  const int64_t* t;   // descriptor table (device)
  int nv;
  float* p;
  const float* g;
  float* m;           // nullable when beta1 == 0
  float* slots;
  bf16_t* pb;         // nullable
  float* ws;
  int64_t ws_tile_g2, ws_tile_w2, ws_tile_x2, ws_var, ws_xden, ws_parts;   // float offsets into ws
  float* gnorm_sq;
  float clip, lr, decay, beta1, eps1, eps2;
  const float* lr_dev;
};

__device__ __forceinline__ const int64_t* af_desc(const AfArgs& a, int v) { return a.t + (int64_t)v * DMI_AF_FIELDS; }

// the variable that owns tile (or segment) index i: last v with t[v][field] <= i
__device__ __forceinline__ int af_find(const AfArgs& a, int64_t i, int field) {
  int lo = 0, hi = a.nv - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.t[(int64_t)mid * DMI_AF_FIELDS + field] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float block_sum_256f(float x, float* sm) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
  __syncthreads();
  const float r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ float af_mult(const AfArgs& a) {
  const float gsq = a.gnorm_sq[0];
  return a.clip > 0.f ? a.clip / fmaxf(sqrtf(gsq), a.clip) : 1.f;
}

// the four columns c0..c0+3 of one row: one 16-byte access where the whole quad is inside the variable and aligned
__device__ __forceinline__ f32x4 af_load4(const float* base, int c0, int C, bool vec) {
  if (vec && c0 + 3 < C) return *(const f32x4*)(base + c0);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c0 + j < C) r[j] = base[c0 + j];
  return r;
}
__device__ __forceinline__ void af_store4(float* base, int c0, int C, bool vec, const f32x4& v) {
  if (vec && c0 + 3 < C) { *(f32x4*)(base + c0) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c0 + j < C) base[c0 + j] = v[j];
}

struct AfTile {
  int v;
  int64_t off, ld, R, C;
  int64_t r0, c0, tr, tc;   // tile origin and index
  bool fact, vec;
};
__device__ __forceinline__ AfTile af_tile(const AfArgs& a, int64_t tile) {
  AfTile T;
  T.v = af_find(a, tile, F_TILE0);
  const int64_t* d = af_desc(a, T.v);
  T.off = d[F_OFF]; T.R = d[F_ROWS]; T.C = d[F_COLS]; T.ld = d[F_LD];
  T.fact = d[F_FACT] != 0;
  const int64_t k = tile - d[F_TILE0];
  T.tr = k / d[F_NTC];
  T.tc = k - T.tr * d[F_NTC];
  T.r0 = T.tr * AF_TR;
  T.c0 = T.tc * AF_TC;
  T.vec = ((T.off | T.ld) & 3) == 0;
  return T;
}

// ---------------------------------------------------------------------------------------------------- 1: statistics
__global__ __launch_bounds__(256) void af_stats_kernel(AfArgs a) {
  __shared__ float sm[4];
  __shared__ f32x4 colsm[4][64];
  const AfTile T = af_tile(a, blockIdx.x);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cl = lane * 4;
  const int C = (int)(T.C - T.c0);
  const int nr = (int)min((int64_t)AF_TR, T.R - T.r0);
  const int64_t* d = af_desc(a, T.v);
  float sg = 0.f, sw = 0.f;
  f32x4 col = {0.f, 0.f, 0.f, 0.f};
  float* rowpart = a.ws + a.ws_parts + d[F_ROWPART] + T.tc * T.R;   // [tc][R]
  for (int r = w; r < nr; r += 4) {
    const int64_t base = T.off + (T.r0 + r) * T.ld + T.c0;
    const f32x4 gv = af_load4(a.g + base, cl, C, T.vec);
    const f32x4 wv = af_load4(a.p + base, cl, C, T.vec);
    const float rg = (gv[0] * gv[0] + gv[1] * gv[1]) + (gv[2] * gv[2] + gv[3] * gv[3]);
    sg += rg;
    sw += (wv[0] * wv[0] + wv[1] * wv[1]) + (wv[2] * wv[2] + wv[3] * wv[3]);
    if (T.fact) {
#pragma unroll
      for (int j = 0; j < 4; ++j) col[j] += gv[j] * gv[j];
      const float rs = wave_sum(rg);
      if (lane == 0) rowpart[T.r0 + r] = rs;
    }
  }
  const float tg = block_sum_256f(sg, sm);
  const float tw = block_sum_256f(sw, sm);
  if (threadIdx.x == 0) {
    a.ws[a.ws_tile_g2 + blockIdx.x] = tg;
    a.ws[a.ws_tile_w2 + blockIdx.x] = tw;
  }
  if (T.fact) {
    colsm[w][lane] = col;
    __syncthreads();
    if (w == 0) {
      f32x4 s;
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = (colsm[0][lane][j] + colsm[1][lane][j]) + (colsm[2][lane][j] + colsm[3][lane][j]);
      float* colpart = a.ws + a.ws_parts + d[F_COLPART] + T.tr * T.C + T.c0;   // [tr][C]
      af_store4(colpart, cl, C, ((T.C | T.c0) & 3) == 0 && ((d[F_COLPART] + a.ws_parts) & 3) == 0, s);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- 2: partial sums
// blocks [0, nv): per-variable scalars; blocks [nv, nv + nseg): 256 entries of a factored variable's row or column vector
__global__ __launch_bounds__(256) void af_reduce_kernel(AfArgs a) {
  __shared__ float sm[4];
  if ((int)blockIdx.x < a.nv) {
    const int v = blockIdx.x;
    const int64_t* d = af_desc(a, v);
    const int64_t t0 = d[F_TILE0], nt = d[F_NTR] * d[F_NTC];
    float sg = 0.f, sw = 0.f;
    for (int64_t i = threadIdx.x; i < nt; i += 256) {
      sg += a.ws[a.ws_tile_g2 + t0 + i];
      sw += a.ws[a.ws_tile_w2 + t0 + i];
    }
    sg = block_sum_256f(sg, sm);
    sw = block_sum_256f(sw, sm);
    if (threadIdx.x == 0) {
      a.ws[a.ws_var + (int64_t)v * AF_VS + 0] = sg;
      a.ws[a.ws_var + (int64_t)v * AF_VS + 1] = sw;
    }
    return;
  }
  // the four waves sum every fourth tile partial of the lane's entry (loads unrolled, adds in order), then combine in fixed order
  __shared__ float part4[4][AF_SEG];
  const int64_t s = (int64_t)blockIdx.x - a.nv;
  const int v = af_find(a, s, F_SEG0);
  const int64_t* d = af_desc(a, v);
  const int64_t R = d[F_ROWS], C = d[F_COLS];
  const int64_t nsr = (R + AF_SEG - 1) / AF_SEG;
  const int64_t k = s - d[F_SEG0];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* parts = a.ws + a.ws_parts;
  const bool row = k < nsr;     // row vector: the column tiles of [tc][R]; column vector: the row tiles of [tr][C]
  const int64_t e = (row ? k : k - nsr) * AF_SEG + lane, len = row ? R : C, nt = row ? d[F_NTC] : d[F_NTR];
  const float* src = parts + (row ? d[F_ROWPART] : d[F_COLPART]) + e;
  float acc = 0.f;
  if (e < len) {
#pragma unroll 8
    for (int64_t t = w; t < nt; t += 4) acc += src[t * len];
  }
  part4[w][lane] = acc;
  __syncthreads();
  if (w == 0 && e < len) parts[(row ? d[F_SROW] : d[F_SCOL]) + e] = (part4[0][lane] + part4[1][lane]) + (part4[2][lane] + part4[3][lane]);
}

// ---------------------------------------------------------------------------------------------------- 3: second moments
// blocks [0, nv): one per variable -- its vr (the vector along d1, the shorter one), mean(vr), max(rms(w), eps2); blocks
// [nv, nv + nseg): the 64-entry segments of the vc vectors (along d0: up to the vocabulary long).  Every block forms the global
// sum g^2 from the per-variable sums in table order, so all of them use the same clip multiplier.
__device__ __forceinline__ float af_vnew(float old, float sum, float n_other, float m2, float keep, float take, float eps1) {
  return keep * old + take * (m2 * (sum / n_other) + eps1);     // mean over the other axis of gc^2 + eps1
}

__global__ __launch_bounds__(256) void af_finalize_kernel(AfArgs a) {
  __shared__ float sm[4];
  const bool scalar = (int)blockIdx.x < a.nv;
  const int64_t s = (int64_t)blockIdx.x - a.nv;
  const int v = scalar ? (int)blockIdx.x : af_find(a, s, F_SEG0);
  const int64_t* d = af_desc(a, v);
  const int64_t R = d[F_ROWS], C = d[F_COLS];
  const bool vr_row = d[F_VR_ROW] != 0;
  const int64_t nsr = (R + AF_SEG - 1) / AF_SEG;
  if (!scalar && ((s - d[F_SEG0] < nsr) == vr_row)) return;   // a vr segment: the variable's own block updates vr
  float gs = 0.f;
  for (int i = threadIdx.x; i < a.nv; i += 256) gs += a.ws[a.ws_var + (int64_t)i * AF_VS];
  gs = block_sum_256f(gs, sm);
  const float mult = a.clip > 0.f ? a.clip / fmaxf(sqrtf(gs), a.clip) : 1.f;
  const float m2 = mult * mult, keep = a.decay, take = 1.f - a.decay;
  const float* parts = a.ws + a.ws_parts;
  if (!scalar) {
    const int64_t k = s - d[F_SEG0];
    const bool row = k < nsr;
    const int64_t e = (row ? k : k - nsr) * AF_SEG + threadIdx.x;
    if (threadIdx.x < AF_SEG && e < (row ? R : C)) {
      float* vec = a.slots + (row ? d[F_SLOT_ROW] : d[F_SLOT_COL]);
      vec[e] = af_vnew(vec[e], parts[(row ? d[F_SROW] : d[F_SCOL]) + e], (float)(row ? C : R), m2, keep, take, a.eps1);
    }
    return;
  }
  if (v == 0 && threadIdx.x == 0) a.gnorm_sq[0] = gs;
  float* var = a.ws + a.ws_var + (int64_t)v * AF_VS;
  float meanvr = 0.f;
  if (d[F_FACT]) {
    const int64_t len = vr_row ? R : C;
    float* vr = a.slots + (vr_row ? d[F_SLOT_ROW] : d[F_SLOT_COL]);
    const float* sum = parts + (vr_row ? d[F_SROW] : d[F_SCOL]);
    const float n_other = (float)(vr_row ? C : R);
    float svr = 0.f;
    for (int64_t e = threadIdx.x; e < len; e += 256) {
      const float x = af_vnew(vr[e], sum[e], n_other, m2, keep, take, a.eps1);
      vr[e] = x;
      svr += x;
    }
    svr = block_sum_256f(svr, sm);
    meanvr = svr / (float)len;
  }
  if (threadIdx.x == 0) {
    var[2] = meanvr;
    var[3] = fmaxf(sqrtf(var[1] / (float)(R * C)), a.eps2);
  }
}

// x of one element (and v_new of an unfactored variable)
struct AfX {
  float mult, keep, take, eps1, meanvr;
  bool fact;
  __device__ __forceinline__ float x(float g, float vrow, float vcol, float vold, float& vnew, bool vr_row) const {
    const float gc = g * mult;
    if (fact) {
      const float vr = vr_row ? vrow : vcol, vc = vr_row ? vcol : vrow;
      return gc * rsqrtf(vr / meanvr) * rsqrtf(vc);
    }
    vnew = keep * vold + take * (gc * gc + eps1);
    return gc * rsqrtf(vnew);
  }
};

__device__ __forceinline__ AfX af_x(const AfArgs& a, int v, bool fact) {
  AfX X;
  X.mult = af_mult(a);
  X.keep = a.decay; X.take = 1.f - a.decay; X.eps1 = a.eps1;
  X.meanvr = a.ws[a.ws_var + (int64_t)v * AF_VS + 2];
  X.fact = fact;
  return X;
}

// ---------------------------------------------------------------------------------------------------- 4 / 6: x, apply
template <bool APPLY>
__global__ __launch_bounds__(256) void af_update_kernel(AfArgs a) {
  __shared__ float sm[4];
  const AfTile T = af_tile(a, blockIdx.x);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cl = lane * 4;
  const int C = (int)(T.C - T.c0);
  const int nr = (int)min((int64_t)AF_TR, T.R - T.r0);
  const int64_t* d = af_desc(a, T.v);
  const AfX X = af_x(a, T.v, T.fact);
  const bool vr_row = d[F_VR_ROW] != 0;
  const float* vrow = a.slots + d[F_SLOT_ROW] + T.r0;
  const float* vcol = a.slots + d[F_SLOT_COL] + T.c0;
  float* vfull = a.slots + d[F_SLOT_V];                 // dense [R, C] for an unfactored variable
  const bool vvec = ((d[F_SLOT_V] | T.C) & 3) == 0;
  f32x4 vc4 = {0.f, 0.f, 0.f, 0.f};
  if (T.fact) vc4 = af_load4(vcol, cl, C, false);
  float ux = 0.f, lr = 0.f;
  if (APPLY) {
    lr = a.lr_dev ? a.lr_dev[0] : a.lr;
    const float* var = a.ws + a.ws_var + (int64_t)T.v * AF_VS;
    ux = (lr * var[3]) / a.ws[a.ws_xden + T.v];   // u = scale * x / max(1, rms(x))  ->  (scale / den) * x
  }
  const float b1 = a.beta1, nb1 = 1.f - a.beta1;
  float sx = 0.f;
  for (int r = w; r < nr; r += 4) {
    const int64_t base = T.off + (T.r0 + r) * T.ld + T.c0;
    const int64_t vbase = (T.r0 + r) * T.C + T.c0;
    const f32x4 gv = af_load4(a.g + base, cl, C, T.vec);
    const float vr = T.fact ? vrow[r] : 0.f;
    f32x4 vo = {0.f, 0.f, 0.f, 0.f}, vn = {0.f, 0.f, 0.f, 0.f};
    if (!T.fact) vo = af_load4(vfull + vbase, cl, C, vvec);
    f32x4 xv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float vj = 0.f;
      xv[j] = X.x(gv[j], vr, vc4[j], vo[j], vj, vr_row);
      vn[j] = vj;
    }
    if (!APPLY) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (cl + j < C) sx += xv[j] * xv[j];
    } else {
      f32x4 pv = af_load4(a.p + base, cl, C, T.vec);
      if (b1 != 0.f) {
        f32x4 mv = af_load4(a.m + base, cl, C, T.vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          mv[j] = b1 * mv[j] + nb1 * (ux * xv[j]);
          pv[j] -= mv[j];
        }
        af_store4(a.m + base, cl, C, T.vec, mv);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) pv[j] -= ux * xv[j];
      }
      af_store4(a.p + base, cl, C, T.vec, pv);
      if (!T.fact) af_store4(vfull + vbase, cl, C, vvec, vn);
      if (a.pb) {
        bf16_t* pb = a.pb + base;
        if (T.vec && cl + 3 < C) {
          *(u32x2*)(pb + cl) = u32x2{pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (cl + j < C) pb[cl + j] = f2bf(pv[j]);
        }
      }
    }
  }
  if (!APPLY) {
    const float t = block_sum_256f(sx, sm);
    if (threadIdx.x == 0) a.ws[a.ws_tile_x2 + blockIdx.x] = t;
  }
}

// ---------------------------------------------------------------------------------------------------- 5: max(1, rms(x))
__global__ __launch_bounds__(256) void af_xfinish_kernel(AfArgs a) {
  __shared__ float sm[4];
  const int v = blockIdx.x;
  const int64_t* d = af_desc(a, v);
  const int64_t t0 = d[F_TILE0], nt = d[F_NTR] * d[F_NTC];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < nt; i += 256) s += a.ws[a.ws_tile_x2 + t0 + i];
  s = block_sum_256f(s, sm);
  if (threadIdx.x == 0) a.ws[a.ws_xden + v] = fmaxf(1.f, sqrtf(s / (float)(d[F_ROWS] * d[F_COLS])) / 1.0f);
}

// ---------------------------------------------------------------------------------------------------- host
static int64_t af_align4(int64_t x) { return (x + 3) & ~(int64_t)3; }

struct AfLayout {
  int64_t ntiles, nseg, tile_g2, tile_w2, tile_x2, var, xden, parts, total;   // floats
};
static AfLayout af_layout(int64_t ntiles, int64_t nseg, int nv, int64_t parts_floats) {
  AfLayout L;
  L.ntiles = ntiles; L.nseg = nseg;
  L.tile_g2 = 0;
  L.tile_w2 = af_align4(ntiles);
  L.tile_x2 = L.tile_w2 + af_align4(ntiles);
  L.var = L.tile_x2 + af_align4(ntiles);
  L.xden = L.var + af_align4((int64_t)nv * AF_VS);
  L.parts = L.xden + af_align4(nv);
  L.total = L.parts + parts_floats;
  return L;
}

extern "C" int dmi_adafactor_plan(int64_t* table, int nvars, int64_t* totals) {
  DMI_REQUIRE(table && totals && nvars > 0, "adafactor_plan: bad args");
  int64_t tile = 0, seg = 0, parts = 0;
  for (int v = 0; v < nvars; ++v) {
    int64_t* d = table + (int64_t)v * DMI_AF_FIELDS;
    const int64_t R = d[F_ROWS], C = d[F_COLS], ld = d[F_LD];
    DMI_REQUIRE(R > 0 && C > 0 && d[F_OFF] >= 0, "adafactor_plan: variable %d: bad extents (%lld x %lld at %lld)", v,
                (long long)R, (long long)C, (long long)d[F_OFF]);
    DMI_REQUIRE(ld >= C && (R == 1 || ld > 0), "adafactor_plan: variable %d: leading dimension %lld < cols %lld", v, (long long)ld,
                (long long)C);
    DMI_REQUIRE(C <= (1 << 30) && R * C < ((int64_t)1 << 40), "adafactor_plan: variable %d too large", v);
    DMI_REQUIRE(d[F_FACT] == 0 || d[F_FACT] == 1, "adafactor_plan: variable %d: factored must be 0 or 1", v);
    DMI_REQUIRE(d[F_SLOT_ROW] >= 0 && d[F_SLOT_COL] >= 0 && d[F_SLOT_V] >= 0, "adafactor_plan: variable %d: negative slot offset", v);
    d[F_TILE0] = tile;
    d[F_NTR] = cdiv64(R, AF_TR);
    d[F_NTC] = cdiv64(C, AF_TC);
    tile += d[F_NTR] * d[F_NTC];
    d[F_SEG0] = seg;
    if (d[F_FACT]) {
      seg += cdiv64(R, AF_SEG) + cdiv64(C, AF_SEG);
      d[F_ROWPART] = parts; parts += af_align4(d[F_NTC] * R);
      d[F_COLPART] = parts; parts += af_align4(d[F_NTR] * C);
      d[F_SROW] = parts; parts += af_align4(R);
      d[F_SCOL] = parts; parts += af_align4(C);
    } else {
      d[F_ROWPART] = d[F_COLPART] = d[F_SROW] = d[F_SCOL] = 0;
    }
  }
  DMI_REQUIRE(tile < ((int64_t)1 << 31) && seg < ((int64_t)1 << 30), "adafactor_plan: too many tiles");
  const AfLayout L = af_layout(tile, seg, nvars, parts);
  totals[0] = tile;
  totals[1] = seg;
  totals[2] = L.total * 4;
  return DMI_OK;
}

extern "C" int dmi_adafactor_step(const int64_t* table_dev, int nvars, const int64_t* totals, float* p, const float* g, float* m,
                                  float* slots, uint16_t* p_bf16, float* gnorm_sq, float clip, float lr, const float* lr_dev,
                                  float decay, float beta1, float eps1, float eps2, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  DMI_REQUIRE(table_dev && totals && nvars > 0 && p && g && slots && gnorm_sq && workspace,
              "adafactor_step: bad args (null pointer or nvars <= 0)");
  DMI_REQUIRE(totals[0] > 0 && totals[1] >= 0 && totals[2] > 0, "adafactor_step: totals do not come from dmi_adafactor_plan");
  DMI_REQUIRE(workspace_bytes >= totals[2], "adafactor_step: workspace of %lld bytes, the plan needs %lld", (long long)workspace_bytes,
              (long long)totals[2]);
  DMI_REQUIRE(beta1 == 0.f || m, "adafactor_step: beta1 != 0 needs the momentum buffer m");
  DMI_REQUIRE(beta1 >= 0.f && beta1 < 1.f && decay >= 0.f && decay < 1.f, "adafactor_step: beta1 and decay must be in [0, 1)");
  DMI_REQUIRE(eps1 >= 0.f && eps2 >= 0.f, "adafactor_step: negative epsilon");
  DMI_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)(m ? m : p) | (uintptr_t)slots | (uintptr_t)workspace) & 15) == 0 &&
                  (((uintptr_t)p_bf16) & 7) == 0,
              "adafactor_step: buffers must be 16-byte aligned");
  // the parts region's size is not needed here: the plan's offsets stay inside what it sized
  const AfLayout L = af_layout(totals[0], totals[1], nvars, 0);
  AfArgs a;
  a.t = table_dev; a.nv = nvars; a.p = p; a.g = g; a.m = m; a.slots = slots; a.pb = p_bf16; a.ws = (float*)workspace;
  a.ws_tile_g2 = L.tile_g2; a.ws_tile_w2 = L.tile_w2; a.ws_tile_x2 = L.tile_x2; a.ws_var = L.var; a.ws_xden = L.xden;
  a.ws_parts = L.parts;
  a.gnorm_sq = gnorm_sq;
  a.clip = clip; a.lr = lr; a.decay = decay; a.beta1 = beta1; a.eps1 = eps1; a.eps2 = eps2; a.lr_dev = lr_dev;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nt = (unsigned)totals[0];
  af_stats_kernel<<<dim3(nt), dim3(256), 0, st>>>(a);
  DMI_CHECK_LAUNCH("adafactor_stats");
  af_reduce_kernel<<<dim3((unsigned)(nvars + totals[1])), dim3(256), 0, st>>>(a);
  DMI_CHECK_LAUNCH("adafactor_reduce");
  af_finalize_kernel<<<dim3((unsigned)(nvars + totals[1])), dim3(256), 0, st>>>(a);
  DMI_CHECK_LAUNCH("adafactor_finalize");
  af_update_kernel<false><<<dim3(nt), dim3(256), 0, st>>>(a);
  DMI_CHECK_LAUNCH("adafactor_xsum");
  af_xfinish_kernel<<<dim3(nvars), dim3(256), 0, st>>>(a);
  DMI_CHECK_LAUNCH("adafactor_xfinish");
  af_update_kernel<true><<<dim3(nt), dim3(256), 0, st>>>(a);
  DMI_CHECK_LAUNCH("adafactor_apply");
  return DMI_OK;
}

// ---------------------------------------------------------------------------------------------------- weight EMA
// tf.train.ExponentialMovingAverage (assign_moving_average): ema -= (ema - p) * one_minus_decay over the flat parameter buffer,
// one streaming pass per optimizer step (DESIGN.md §4 "Weight EMA").  Difference, product and second difference are each rounded
// to fp32 on their own (no fused multiply-add: a numpy float32 restatement gives the same bits); the bf16 copy is rounded from the
// fp32 value that is stored.  16-byte loads and stores (8-byte for the bf16 quad) over the n / 4 whole quads, the n % 4 tail
// element-wise by block 0; 64-bit indices; the grid follows the CU count, not n.  No atomics, no workspace.
__device__ __forceinline__ float ema_update(float e, float p, float omd) {
#pragma clang fp contract(off)
  const float d = e - p;
  const float t = d * omd;
  return e - t;
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, bf16_t* __restrict__ eb, int64_t n,
                                                  float omd) {
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 ev = ((const f32x4*)ema)[i];
    const f32x4 pv = ((const f32x4*)p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[j] = ema_update(ev[j], pv[j], omd);
    ((f32x4*)ema)[i] = ev;
    if (eb) *(u32x2*)(eb + i * 4) = u32x2{pack2bf(ev[0], ev[1]), pack2bf(ev[2], ev[3])};
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    const float e = ema_update(ema[i], p[i], omd);
    ema[i] = e;
    if (eb) eb[i] = f2bf(e);
  }
}

static int ema_num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      n = prop.multiProcessorCount;
    else
      n = 256;
  }
  return n;
}

#define EMA_BLOCKS_PER_CU 8   // 8 blocks of 4 waves: every CU's 32 wave slots hold a stream of 16-byte requests

extern "C" int dmi_ema_step(float* ema, const float* p, uint16_t* ema_bf16, int64_t n, float one_minus_decay, void* stream) {
  DMI_REQUIRE(ema && p, "ema_step: null pointer (ema or p)");
  DMI_REQUIRE(n > 0, "ema_step: n must be positive (n=%lld)", (long long)n);
  DMI_REQUIRE((((uintptr_t)ema | (uintptr_t)p | (uintptr_t)ema_bf16) & 15) == 0, "ema_step: buffers must be 16-byte aligned");
  DMI_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "ema_step: one_minus_decay must lie in [0, 1] (one_minus_decay=%g)",
              (double)one_minus_decay);   // (NaN fails both comparisons)
  int64_t blocks = cdiv64(n / 4 + 1, 256);
  const int64_t cap = (int64_t)ema_num_cus() * EMA_BLOCKS_PER_CU;
  if (blocks > cap) blocks = cap;
  ema_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(ema, p, ema_bf16, n, one_minus_decay);
  DMI_CHECK_LAUNCH("ema_step");
  return DMI_OK;
}
