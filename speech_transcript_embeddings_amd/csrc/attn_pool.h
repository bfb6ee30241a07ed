// The attentive pooling forward's device code, shared by heads.hip (ste_attn_pool_fwd[_f32], the dense
// [B, L] batch of the training and evaluation route) and attn_pool_seg.hip (ste_attn_pool_seg_fwd[_f32],
// overlapping segments of one row buffer), so that both run the same VALU arithmetic in the
// same order: a segment pools to the bits of the dense kernels on a copy of its rows.  Every
// per-thread share below (l = tid, tid + NT, ...; l = w, w + NW, ...) depends on the row's index inside
// its sample / segment alone, and every reduction has a fixed order.
#pragma once
#include "common.h"

constexpr int POOL_NT = 256;       // threads of the score and softmax blocks
constexpr int POOL_SC_ROWS = 16;   // rows per score block
constexpr int POOL_WS_NT = 512;    // threads of a weighted-sum block: 8 waves split the rows
constexpr int POOL_MAX_L = 8192;   // rows of one sample / segment (their weights sit in LDS)

STE_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}
STE_DEV float block_max(float v, float* red) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = -INFINITY;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s = fmaxf(s, red[i]);
  return s;
}

// 4 consecutive elements of a bf16 or fp32 row (the pooling kernels run on the bf16 audio states
// and on the fp32 text states, see ste_attn_pool_fwd_f32)
STE_DEV f32x4 ld4(const bf16* p) { return load_bf16x4(p); }
STE_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
STE_DEV void st4(bf16* p, f32x4 v) { store_bf16x4(p, v); }
STE_DEV void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

template <typename T>
STE_DEV float row_dot(const T* a, const float* b, int n, int lane) {
  float acc = 0.f;
  for (int c = lane * 4; c < n; c += 256) {
    f32x4 x = ld4(a + c);
    f32x4 y = *reinterpret_cast<const f32x4*>(b + c);
    acc += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
  }
  return wave_sum(acc);
}

// score of one row, by one wave: t_l·w2 + b2 (every lane gets it)
template <typename T>
STE_DEV float pool_score(const T* trow, const float* w2, const float* b2, int Hh, int lane) {
  return row_dot(trow, w2, Hh, lane) + b2[0];
}

// the softmax statistics of the L scores r[0 .. L), by a block of POOL_NT threads: mx = max, inv = 1/Σ exp(r - mx)
STE_DEV void pool_softmax_stat(const float* r, int L, float* red, float& mx, float& inv) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int l = tid; l < L; l += POOL_NT) m = fmaxf(m, r[l]);
  mx = block_max(m, red);
  float sum = 0.f;
  for (int l = tid; l < L; l += POOL_NT) sum += __expf(r[l] - mx);
  sum = block_sum(sum, red);
  inv = 1.0f / sum;
}

// a row's pooling weight from its score and the statistics
STE_DEV float pool_weight(float s, float mx, float inv) { return __expf(s - mx) * inv; }

// pooled[c] = Σ_l wl[l] h0[l][c] for the 256 columns of blockIdx.y, by a block of POOL_WS_NT threads: 8 waves
// split the L rows that start at h0, partials summed in wave order.  wl: the L weights, in LDS and complete.
template <typename T>
STE_DEV void pool_wsum_rows(const T* h0, const float* wl, int L, int H, f32x4 (*part)[64], float* pooled,
                            bf16* pooled_bf16) {
  constexpr int NW = POOL_WS_NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.y * 256 + lane * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c < H) {
    const T* hp = h0 + c;
#pragma unroll 4
    for (int l = w; l < L; l += NW) acc += ld4(hp + (int64_t)l * H) * wl[l];
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < H) {
    f32x4 s = part[0][lane];
#pragma unroll
    for (int i = 1; i < NW; ++i) s += part[i][lane];
    *reinterpret_cast<f32x4*>(pooled + c) = s;
    if (pooled_bf16) store_bf16x4(pooled_bf16 + c, s);
  }
}
