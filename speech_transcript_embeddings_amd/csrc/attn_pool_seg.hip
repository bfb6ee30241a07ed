// Segmented attentive pooling: AttentivePooling (ref:training/trainer_unfreeze.py:171-211) of
// G segments of ONE row buffer, each a run of rows seg_row[g] .. seg_row[g] + seg_len[g] - 1.
// Segments may overlap, repeat and come in any order: the overlapping windows of a long recording are views
// of hidden states that are stored once.  Three launches, no atomics, no memset, 64-bit row addresses:
//   pool_seg_score_kernel  score[r] = t_r·w2 + b2, once per row of the buffer   grid ceil(rows/16)
//   pool_seg_stat_kernel   stat[g] = (max, 1/Σ exp) over the segment's scores     grid G
//   pool_seg_wsum_kernel   w_l = exp(score_l - max)·inv into LDS, then            grid (G, ceil(H/256))
//                          pooled[g][c] = Σ_l w_l h_l[c]
// A row's weight differs from segment to segment, so the scores are not normalised in place as the dense
// pool_softmax_kernel does.  The arithmetic is attn_pool.h's, shared with the dense kernels of heads.hip:
// pooled[g] has the bits of ste_attn_pool_fwd[_f32](B = 1, L = seg_len[g], mask = NULL) on a copy of the
// segment's rows, whatever G, the segment's position, its overlaps and the other segments are.
#include "common.h"
#include "attn_pool.h"
#include "../../include/ste.h"

namespace {

// an empty segment pools to zeros and reads no row (the test is uniform over a block)
STE_DEV bool pool_seg_empty(int64_t r0, int len, int64_t rows) {
  return len <= 0 || len > POOL_MAX_L || r0 < 0 || r0 > rows - len;
}

template <typename T>
__global__ __launch_bounds__(POOL_NT) void pool_seg_score_kernel(const T* t, const float* w2, const float* b2,
                                                               int64_t rows, int Hh, float* sc) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * POOL_SC_ROWS;
  const int64_t r1 = min(rows, r0 + POOL_SC_ROWS);
  for (int64_t r = r0 + w; r < r1; r += POOL_NT / 64) {
    const float s = pool_score(t + r * Hh, w2, b2, Hh, lane);
    if (lane == 0) sc[r] = s;
  }
}

__global__ __launch_bounds__(POOL_NT) void pool_seg_stat_kernel(const float* sc, const int64_t* seg_row,
                                                              const int32_t* seg_len, int64_t rows, float* stat) {
  __shared__ float red[8];
  const int g = blockIdx.x;
  const int64_t r0 = seg_row[g];
  const int L = seg_len[g];
  float mx = 0.f, inv = 0.f;
  if (!pool_seg_empty(r0, L, rows)) pool_softmax_stat(sc + r0, L, red, mx, inv);
  if (threadIdx.x == 0) {
    stat[2 * (int64_t)g] = mx;
    stat[2 * (int64_t)g + 1] = inv;
  }
}

template <typename T>
__global__ __launch_bounds__(POOL_WS_NT) void pool_seg_wsum_kernel(const T* h, const float* sc, const float* stat,
                                                                 const int64_t* seg_row, const int32_t* seg_len,
                                                                 int64_t rows, int H, float* pooled,
                                                                 bf16* pooled_bf16) {
  __shared__ float wl[POOL_MAX_L];
  __shared__ f32x4 part[POOL_WS_NT / 64][64];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = seg_row[g];
  const int L = seg_len[g];
  float* out = pooled + (int64_t)g * H;
  bf16* outb = pooled_bf16 ? pooled_bf16 + (int64_t)g * H : nullptr;
  if (pool_seg_empty(r0, L, rows)) {
    const int c = blockIdx.y * 256 + tid * 4;
    if (tid < 64 && c < H) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(out + c) = z;
      if (outb) store_bf16x4(outb + c, z);
    }
    return;
  }
  const float mx = stat[2 * (int64_t)g], inv = stat[2 * (int64_t)g + 1];
  for (int l = tid; l < L; l += POOL_WS_NT) wl[l] = pool_weight(sc[r0 + l], mx, inv);
  __syncthreads();
  pool_wsum_rows(h + r0 * H, wl, L, H, part, out, outb);
}

template <typename T>
int attn_pool_seg_fwd(const T* t, const float* w2, const float* b2, const T* h, int64_t rows, const int64_t* seg_row,
                      const int32_t* seg_len, int G, int Hh, int H, float* score, float* stat, float* pooled,
                      bf16* pooled_bf16, hipStream_t s) {
  if (G < 1 || rows < 1 || Hh < 4 || H < 4 || (Hh & 3) || (H & 3)) return STE_ERR_SHAPE;
  const int64_t sblocks = (rows + POOL_SC_ROWS - 1) / POOL_SC_ROWS;
  if (sblocks > INT32_MAX) return STE_ERR_SHAPE;
  if (!t || !w2 || !b2 || !h || !seg_row || !seg_len || !score || !stat || !pooled) return STE_ERR_ARG;
  hipLaunchKernelGGL(pool_seg_score_kernel<T>, dim3((unsigned)sblocks), dim3(POOL_NT), 0, s, t, w2, b2, rows, Hh,
                     score);
  STE_CHECK_LAUNCH();
  hipLaunchKernelGGL(pool_seg_stat_kernel, dim3(G), dim3(POOL_NT), 0, s, score, seg_row, seg_len, rows, stat);
  STE_CHECK_LAUNCH();
  hipLaunchKernelGGL(pool_seg_wsum_kernel<T>, dim3(G, (H + 255) / 256), dim3(POOL_WS_NT), 0, s, h, score, stat, seg_row,
                     seg_len, rows, H, pooled, pooled_bf16);
  STE_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ste_attn_pool_seg_fwd(const void* t, const float* w2, const float* b2, const void* h, int64_t rows,
                                     const int64_t* seg_row, const int32_t* seg_len, int G, int Hh, int H,
                                     float* score, float* stat, float* pooled, void* pooled_bf16, void* stream) {
  return attn_pool_seg_fwd((const bf16*)t, w2, b2, (const bf16*)h, rows, seg_row, seg_len, G, Hh, H, score, stat,
                           pooled, (bf16*)pooled_bf16, (hipStream_t)stream);
}

extern "C" int ste_attn_pool_seg_fwd_f32(const float* t, const float* w2, const float* b2, const float* h,
                                         int64_t rows, const int64_t* seg_row, const int32_t* seg_len, int G, int Hh,
                                         int H, float* score, float* stat, float* pooled, void* pooled_bf16,
                                         void* stream) {
  return attn_pool_seg_fwd(t, w2, b2, h, rows, seg_row, seg_len, G, Hh, H, score, stat, pooled, (bf16*)pooled_bf16,
                           (hipStream_t)stream);
}
