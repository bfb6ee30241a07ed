// fp32-operand GEMM on the exact-f32 matrix core (v_mfma_f32_16x16x4_f32: an fmaf chain,
// bit for bit) for the projection / cross-attention / fusion heads, whose gradients are
// differences of the positive and corrupted transcripts' nearly identical activations.
//
// Replaces the aten::addmm / aten::mm behind the heads' nn.Linear layers in
//   /root/reference/training/trainer_unfreeze.py:66-99   EnhancedProjection
//                                                   :125-168 CrossModalAttention q / out_proj
//                                                   :171-211 AttentivePooling scorer (text side)
//                                                   :470-477 text_fusion / audio_fusion
// The reference computes these in fp32 (run_embedding_trainer_unfreeze.sh:27 --no_fp16).  With
// bf16 operands the loss gradient ds·(t_neg - t_pos) — a difference of two embeddings that
// share 80 % of their tokens — turns 2^-9 operand rounding into 4-18 % gradient errors (DESIGN
// §4); these GEMMs are tiny (M = batch rows, or 2·b·L text rows for the pooling scorer), so
// they run in fp32 at the f32 matrix rate (1/16 of bf16, MI355X_MICROARCH.md matrix table).
//
// Same argument block and epilogue order as ste_gemm (include/ste.h), with A, B, C2 and Z fp32.
// Tile 64x64, 256 threads = 4 waves of 32x32 (2x2 16x16 accumulators); k staged through LDS in
// chunks of 16 as [k][m] images (row stride 80 floats: the four k rows a fragment read touches
// land on disjoint 16-bank groups); launches with few such tiles and no column sums run on 32x32
// tiles (4 waves of 16x16, chunks of 32) with bit-identical results.  The K loop is
// software-pipelined over two LDS images: chunk
// k+1 is loaded into registers before the MFMA block of chunk k and written to the other image
// after it, one barrier per chunk.
//
// Two split-K plans, both deterministic (slabs of ws summed in slab order):
//  - few output tiles (<= ste_gemm_f32_plan_max_tiles, 0 = off by default) and K >= 512, any epilogue: the heads'
//    M = batch-rows launches, 12-48 tiles on 256 CUs with 48-96 serial chunks each.  S slabs write
//    raw accumulators to ws[z][M][N]; gemm_f32_reduce_kernel (same tiling and element mapping)
//    rebuilds each accumulator and runs the one epilogue.
//  - plain weight gradients with K >= 1024 and a caller's workspace: the older plan, slabs summed
//    by f32_slab_reduce_kernel (kept as it is: its rounding differs from the epilogue's).
#include <atomic>

#include "common.h"
#include "../../include/ste.h"

namespace {

constexpr int BM = 64, BN = 64, BKC = 16, NT = 256;   // the 64x64 tiling (plans, slabs); Geo has both

STE_DEV float act_fwd(float v, int act) {
  switch (act) {
    case STE_ACT_SWISH: return swish_f(v);
    case STE_ACT_GELU: return gelu_f(v);
    case STE_ACT_TANH: return tanhf(v);
    case STE_ACT_RELU: return fmaxf(v, 0.0f);
    default: return v;
  }
}
STE_DEV float act_bwd(float z, int act) {
  switch (act) {
    case STE_ACT_SWISH_BWD: return swish_d(z);
    case STE_ACT_GELU_BWD: return gelu_d(z);
    case STE_ACT_TANH_BWD_OUT: return 1.0f - z * z;
    case STE_ACT_RELU_BWD: return z > 0.0f ? 1.0f : 0.0f;
    default: return 1.0f;
  }
}

// Tile geometry by NI, the accumulators per wave and dimension (4 waves as 2 x 2):
//   NI = 2: 64x64 tile, chunks of 16 k, LDS row stride 80;  NI = 1: 32x32 tile, chunks of 32 k, stride 48
// (either stride puts the four k rows of a fragment read on disjoint 16-bank groups).  Both stage
// 256 float4 per operand and chunk, one per thread, and issue the same MFMAs in the same k order
// for an output element, so its value does not depend on NI.
template <int NI> struct Geo {
  static constexpr int TB = 32 * NI, KB = NI == 2 ? 16 : 32, LW = NI == 2 ? 80 : 48;
};

// This thread's 4 floats of a [TB rows x KB k] operand chunk (zero outside the matrix).
// KC: X[r*ld + k] (one float4 of 4 consecutive k per thread); KM: X[k*ld + r] (4 consecutive rows).
template <bool KC, int NI>
STE_DEV f32x4 stage_load(const float* X, int64_t ld, int rows, int K, int r0, int k0, int tid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (KC) {
    const int r = tid / (Geo<NI>::KB / 4), kq = (tid % (Geo<NI>::KB / 4)) * 4;
    const int gr = r0 + r, gk = k0 + kq;
    if (gr < rows) {
      const float* src = X + (int64_t)gr * ld + gk;
      if (gk + 3 < K) v = *reinterpret_cast<const f32x4*>(src);
      else
        for (int e = 0; e < 4; ++e) v[e] = gk + e < K ? src[e] : 0.f;
    }
  } else {
    const int k = tid / (Geo<NI>::TB / 4), rq = (tid % (Geo<NI>::TB / 4)) * 4;
    const int gk = k0 + k, gr = r0 + rq;
    if (gk < K) {
      const float* src = X + (int64_t)gk * ld + gr;
      if (gr + 3 < rows) v = *reinterpret_cast<const f32x4*>(src);
      else
        for (int e = 0; e < 4; ++e) v[e] = gr + e < rows ? src[e] : 0.f;
    }
  }
  return v;
}

// ... and their place in the chunk's LDS image img[k][row].
template <bool KC, int NI>
STE_DEV void stage_store(float* img, f32x4 v, int tid) {
  if constexpr (KC) {
    const int r = tid / (Geo<NI>::KB / 4), kq = (tid % (Geo<NI>::KB / 4)) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) img[(kq + e) * Geo<NI>::LW + r] = v[e];
  } else {
    const int k = tid / (Geo<NI>::TB / 4), rq = (tid % (Geo<NI>::TB / 4)) * 4;
    *reinterpret_cast<f32x4*>(img + k * Geo<NI>::LW + rq) = v;
  }
}

// The epilogue of one wave's NI x NI accumulators, shared by the unsplit kernels and the slab reduction.
// Accumulator (i, j) element e: row m0+wm+16i+4g+e, column n0+wn+16j+r (wave w: wm = 16·NI·(w&1),
// wn = 16·NI·(w>>1); lane: r = lane&15, g = lane>>4).  cs_part: the ordered column-sum partial rows
// (one per (tile row, wave row), summed by ste_rowsum_ordered) or null: one atomic per column.
template <int NI>
STE_DEV void epilogue(const ste_gemm_args& p, const f32x4 (&acc)[NI][NI], int m0, int n0, int w, int lane,
                      float* cs_part) {
  const int wm = (w & 1) * 16 * NI, wn = (w >> 1) * 16 * NI;
  const int r = lane & 15, g = lane >> 4;
  const uint32_t thresh = (uint32_t)(p.drop_p * 4294967296.0);
  const float inv_keep = p.drop_p > 0.f ? 1.0f / (1.0f - p.drop_p) : 1.0f;
  const bool fwd_act = p.act >= STE_ACT_SWISH && p.act <= STE_ACT_RELU;
  const bool bwd_act = p.act >= STE_ACT_SWISH_BWD;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = n0 + wn + 16 * j + r;
    const bool cv = col < p.N;
    const float bias = (p.bias && cv) ? p.bias[col] : 0.f;
    float cs = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = m0 + wm + 16 * i + 4 * g + e;
        if (!cv || row >= p.M) continue;
        float v = (acc[i][j][e] + bias) * p.alpha;
        if (fwd_act) {
          if (p.C2) ((float*)p.C2)[(int64_t)row * p.ldc2 + col] = v;
          v = act_fwd(v, p.act);
        } else if (bwd_act) {
          v *= act_bwd(((const float*)p.Z)[(int64_t)row * p.ldz + col], p.act);
        }
        if (p.drop_p > 0.f) v *= drop_scale(p.seed, (uint64_t)row * (uint64_t)p.drop_ld + (uint64_t)col, thresh, inv_keep);
        if (p.row_scale) v *= p.row_scale[row];
        cs += v;
        if (p.R) {
          const int64_t ro = (int64_t)row * p.ldr + col;
          v += p.r_bf16 ? (float)((const bf16*)p.R)[ro] : ((const float*)p.R)[ro];
        }
        const int64_t co = (int64_t)row * p.ldc + col;
        if (p.beta != 0.f) v += p.beta * (p.c_bf16 ? (float)((const bf16*)p.C)[co] : ((const float*)p.C)[co]);
        if (p.C) {
          if (p.c_bf16) ((bf16*)p.C)[co] = (bf16)v;
          else ((float*)p.C)[co] = v;
        }
        if (p.C3) ((bf16*)p.C3)[(int64_t)row * p.ldc3 + col] = (bf16)(p.c3_lo ? v - (float)(bf16)v : v);
      }
    if (p.colsum) {  // the column's 4 lane groups hold disjoint rows: sum them
      cs += __shfl_xor(cs, 16, 64);
      cs += __shfl_xor(cs, 32, 64);
      if (g == 0 && cv) {
        if (cs_part) cs_part[((int64_t)blockIdx.x * 2 + (w & 1)) * p.N + col] = cs;
        else atomicAdd(p.colsum + col, cs);
      }
    }
  }
}

// SPLIT: write the raw accumulators of K range [z*kc, (z+1)*kc) to ws[z][M][N] (no epilogue).
// (NI = 2 only.)
template <bool A_KC, bool B_KC, bool SPLIT, int NI>
__global__ __launch_bounds__(NT) void gemm_f32_kernel(ste_gemm_args p, int kc) {
  constexpr int TB = Geo<NI>::TB, KB = Geo<NI>::KB, LW = Geo<NI>::LW;
  static_assert(NI == 2 || !SPLIT, "slabs are written and reduced in the 64x64 mapping");
  __shared__ __attribute__((aligned(16))) float sa[2][KB * LW];
  __shared__ __attribute__((aligned(16))) float sb[2][KB * LW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m0 = blockIdx.x * TB, n0 = blockIdx.y * TB;
  const int wm = (w & 1) * 16 * NI, wn = (w >> 1) * 16 * NI;
  const int r = lane & 15, g = lane >> 4;
  const float* A = (const float*)p.A;
  const float* B = (const float*)p.B;
  const int kb = SPLIT ? blockIdx.z * kc : 0;
  const int ke = SPLIT ? min(p.K, kb + kc) : p.K;
  f32x4 acc[NI][NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the K range end acts as the matrix edge for this slab
  f32x4 va = stage_load<A_KC, NI>(A, p.lda, p.M, ke, m0, kb, tid);
  f32x4 vb = stage_load<B_KC, NI>(B, p.ldb, p.N, ke, n0, kb, tid);
  stage_store<A_KC, NI>(sa[0], va, tid);
  stage_store<B_KC, NI>(sb[0], vb, tid);
  __syncthreads();
  int cur = 0;
  for (int k0 = kb; k0 < ke; k0 += KB, cur ^= 1) {
    const bool more = k0 + KB < ke;
    if (more) {   // chunk k+1 travels while chunk k multiplies
      va = stage_load<A_KC, NI>(A, p.lda, p.M, ke, m0, k0 + KB, tid);
      vb = stage_load<B_KC, NI>(B, p.ldb, p.N, ke, n0, k0 + KB, tid);
    }
    const float* ia = sa[cur];
    const float* ib = sb[cur];
#pragma unroll
    for (int kk = 0; kk < KB; kk += 4) {
      float a[NI], b[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        a[i] = ia[(kk + g) * LW + wm + 16 * i + r];
        b[i] = ib[(kk + g) * LW + wn + 16 * i + r];
      }
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      // the other image: every wave finished reading it before the previous barrier
      stage_store<A_KC, NI>(sa[cur ^ 1], va, tid);
      stage_store<B_KC, NI>(sb[cur ^ 1], vb, tid);
    }
    __syncthreads();
  }
  // accumulator (i, j) element e: row m0+wm+16i+4g+e, column n0+wn+16j+r
  if constexpr (SPLIT) {
    float* slab = p.ws + (int64_t)blockIdx.z * p.M * p.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn + 16 * j + r;
        if (col >= p.N) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = m0 + wm + 16 * i + 4 * g + e;
          if (row < p.M) slab[(int64_t)row * p.N + col] = acc[i][j][e];
        }
      }
    return;
  } else {
    // ordered column sums: p.ws holds this launch's partial rows (the host leaves it null otherwise)
    epilogue<NI>(p, acc, m0, n0, w, lane, p.ws);
  }
}

// Second pass of the few-tile split: accumulator = Σ_z ws[z] in increasing z, in the tiling and
// element mapping of gemm_f32_kernel, then its epilogue.  The column-sum partial rows follow the
// S slabs in ws.  Out-of-range elements read a clamped (valid) address; the epilogue drops them.
__global__ __launch_bounds__(NT) void gemm_f32_reduce_kernel(ste_gemm_args p, int S) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
  const int r = lane & 15, g = lane >> 4;
  const int64_t slab = (int64_t)p.M * p.N;
  const float* src[2][2][4];
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int col = min(n0 + wn + 16 * j + r, p.N - 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = min(m0 + wm + 16 * i + 4 * g + e, p.M - 1);
        src[i][j][e] = p.ws + (int64_t)row * p.N + col;
      }
    }
#pragma unroll 4
  for (int z = 0; z < S; ++z)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] += src[i][j][e][(int64_t)z * slab];
  epilogue<2>(p, acc, m0, n0, w, lane, p.colsum ? p.ws + (int64_t)S * slab : nullptr);
}

// C = beta·C + alpha·Σ_z ws[z] (slab order), 4 columns per thread
__global__ __launch_bounds__(256) void f32_slab_reduce_kernel(float* C, int64_t ldc, const float* ws, int M, int N,
                                                              int S, float alpha, float beta) {
  const int64_t per_row = (N + 3) / 4;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)M * per_row; t += (int64_t)gridDim.x * 256) {
    const int row = (int)(t / per_row), c = (int)(t - (int64_t)row * per_row) * 4;
    for (int e = 0; e < 4 && c + e < N; ++e) {
      float s = 0.f;
      for (int z = 0; z < S; ++z) s += ws[((int64_t)z * M + row) * N + c + e];
      float* o = C + (int64_t)row * ldc + c + e;
      *o = (beta != 0.f ? beta * *o : 0.f) + alpha * s;
    }
  }
}

template <bool SPLIT, int NI>
void launch(const ste_gemm_args& a, int S, int kc, hipStream_t s) {
  constexpr int TB = Geo<NI>::TB;
  const dim3 grid((a.M + TB - 1) / TB, (a.N + TB - 1) / TB, S);
  if (a.a_kc && a.b_kc) hipLaunchKernelGGL((gemm_f32_kernel<true, true, SPLIT, NI>), grid, dim3(NT), 0, s, a, kc);
  else if (a.a_kc) hipLaunchKernelGGL((gemm_f32_kernel<true, false, SPLIT, NI>), grid, dim3(NT), 0, s, a, kc);
  else if (a.b_kc) hipLaunchKernelGGL((gemm_f32_kernel<false, true, SPLIT, NI>), grid, dim3(NT), 0, s, a, kc);
  else hipLaunchKernelGGL((gemm_f32_kernel<false, false, SPLIT, NI>), grid, dim3(NT), 0, s, a, kc);
}

// ---- the plan: host arithmetic only (no device query), shared by ste_gemm_f32 and its queries.
// Few 64x64 tiles (at most g_small_tiles, default 64: a quarter of the 256 CUs; the heads' launches
// have 6-48) and no column sums: the 32x32 tiling, four times the workgroups, a quarter of the MFMAs
// per wave and chunk, half the barriers, and the same value for every output element.  Column sums
// stay on the 64x64 tiling: their partial rows are sums over a wave's 32 rows in a fixed order.
// The few-tile split (DESIGN §16 has the isolated timings behind its constants) is off by default
// (g_max_tiles = 0): it changes the fp32 summation order.  When on, it splits when the 64x64
// tiles number at most g_max_tiles and K >= SPLIT_MIN_K; it aims
// at SPLIT_WGS workgroups (LDS and registers let several share a CU, which is what hides the
// chunk round trips) with slabs of at least SLAB_MIN_K.  The A/B build reads the STE_F32_* variables.
constexpr int SPLIT_MIN_K = 512;
std::atomic<int> g_max_tiles{-1};
int max_tiles() {
  int v = g_max_tiles.load();
  if (v < 0) {   // first use: the default, unless a concurrent ste_gemm_f32_plan_max_tiles set one
    const char* e = STE_AB_ENV("STE_F32_MAX_TILES");
    const int dflt = e ? atoi(e) : 0;
    if (g_max_tiles.compare_exchange_strong(v, dflt)) v = dflt;
  }
  return v;
}
std::atomic<int> g_small_tiles{-1};
int small_tiles() {
  int v = g_small_tiles.load();
  if (v < 0) {
    const char* e = STE_AB_ENV("STE_F32_SMALL_TILES");
    const int dflt = e ? atoi(e) : 64;
    if (g_small_tiles.compare_exchange_strong(v, dflt)) v = dflt;
  }
  return v;
}
int split_wgs() {
  static const char* e = STE_AB_ENV("STE_F32_SPLIT_WGS");
  static const int v = e ? atoi(e) : 512;
  return v;
}
int slab_min_k() {
  static const char* e = STE_AB_ENV("STE_F32_SLAB_MIN_K");
  static const int v = e ? atoi(e) : 128;
  return v;
}

int tiles_of(const ste_gemm_args& a) { return ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN); }
int64_t colsum_rows(const ste_gemm_args& a) { return a.colsum ? 2 * (int64_t)((a.M + BM - 1) / BM) : 0; }

// S slabs of whole chunks, as even as whole chunks allow: slab z is [z*kc, min(K, (z+1)*kc)).
void even_slabs(int K, int& S, int& kc) {
  const int chunks = (K + BKC - 1) / BKC;
  kc = (chunks + S - 1) / S * BKC;
  S = (K + kc - 1) / kc;
}

// Slabs the few-tile plan wants for this shape, whatever the workspace (1: no split).
int few_tile_slabs(const ste_gemm_args& a) {
  const int tiles = tiles_of(a), mt = max_tiles();
  if (mt <= 0 || tiles > mt || a.K < SPLIT_MIN_K) return 1;
  int S = (split_wgs() + tiles - 1) / tiles;
  S = S < a.K / slab_min_k() ? S : a.K / slab_min_k();
  if (S < 2) return 1;
  int kc;
  even_slabs(a.K, S, kc);
  return S;
}

struct F32Plan {
  int S, kc;         // slabs (1: one launch) of kc k each
  bool wgrad;        // the plain weight-gradient plan (f32_slab_reduce_kernel)
  bool small;        // one launch on the 32x32 tiling
  int64_t cs_rows;   // ordered column-sum partial rows in ws (0: atomics, or no column sums)
};

F32Plan plan_of(const ste_gemm_args& a) {
  F32Plan pl{1, 0, false, false, 0};
  const int tiles = tiles_of(a);
  const int64_t mn = (int64_t)a.M * a.N;
  // weight gradient over a long reduction: split K into slabs when the tiles cannot fill the chip
  const bool plain = !a.bias && a.act == STE_ACT_NONE && a.drop_p == 0.f && !a.row_scale && !a.colsum && !a.R &&
                     !a.C2 && !a.C3 && a.C && !a.c_bf16;
  if (plain && a.ws && tiles < 256 && a.K >= 1024) {
    int S = (512 + tiles - 1) / tiles;
    S = S < a.K / 256 ? S : a.K / 256;
    while (S > 1 && S * mn * 4 > a.ws_bytes) --S;
    if (S > 1) {
      int kc = (a.K + S - 1) / S;
      kc = (kc + BKC - 1) / BKC * BKC;
      pl.S = (a.K + kc - 1) / kc;
      pl.kc = kc;
      pl.wgrad = true;
      return pl;
    }
  }
  const int64_t rows = colsum_rows(a);
  if (a.ws) {
    // few tiles: the largest S <= the wanted one whose slabs (and partial rows) fit the workspace
    int S = few_tile_slabs(a);
    while (S > 1 && (S * mn + rows * a.N) * 4 > a.ws_bytes) --S;
    if (S > 1) {
      even_slabs(a.K, S, pl.kc);
      pl.S = S;
      pl.cs_rows = rows;
      return pl;
    }
    // column sums: ordered partial rows in ws when it is large enough (deterministic), else atomics
    if (rows && a.ws_bytes >= rows * a.N * 4) pl.cs_rows = rows;
  }
  pl.small = !a.colsum && tiles <= small_tiles();
  return pl;
}

}  // namespace

extern "C" int ste_gemm_f32_plan(const ste_gemm_args* args) {
  if (!args || args->M <= 0 || args->N <= 0 || args->K <= 0) return 0;
  return plan_of(*args).S;
}

extern "C" int ste_gemm_f32_plan_slab(const ste_gemm_args* args) {
  if (!args || args->M <= 0 || args->N <= 0 || args->K <= 0) return 0;
  const F32Plan pl = plan_of(*args);
  return pl.S > 1 ? pl.kc : args->K;
}

extern "C" int64_t ste_gemm_f32_ws_floats(const ste_gemm_args* args) {
  if (!args || args->M <= 0 || args->N <= 0 || args->K <= 0) return 0;
  const int S = few_tile_slabs(*args);
  return (S > 1 ? (int64_t)S * args->M * args->N : 0) + colsum_rows(*args) * args->N;
}

extern "C" int ste_gemm_f32_plan_tile(const ste_gemm_args* args) {
  if (!args || args->M <= 0 || args->N <= 0 || args->K <= 0) return 0;
  return plan_of(*args).small ? 32 : 64;
}

extern "C" int ste_gemm_f32_plan_small_tiles(int tiles) {
  const int prev = small_tiles();
  g_small_tiles.store(tiles < 0 ? 0 : tiles);
  return prev;
}

extern "C" int ste_gemm_f32_plan_max_tiles(int tiles) {
  const int prev = max_tiles();
  g_max_tiles.store(tiles < 0 ? 0 : tiles);
  return prev;
}

extern "C" int ste_gemm_f32(const ste_gemm_args* args, void* stream) {
  if (!args) return STE_ERR_ARG;
  ste_gemm_args a = *args;
  if (a.batch > 1) return STE_ERR_SHAPE;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || !a.A || !a.B) return STE_ERR_ARG;
  // 16-B operand loads: KC operands need K % 4 == 0 and ld % 4 == 0, KM operands rows % 4 == 0
  if (a.a_kc ? (a.K & 3) || (a.lda & 3) : (a.M & 3) || (a.lda & 3)) return STE_ERR_SHAPE;
  if (a.b_kc ? (a.K & 3) || (a.ldb & 3) : (a.N & 3) || (a.ldb & 3)) return STE_ERR_SHAPE;
  if ((((uintptr_t)a.A) & 15) || (((uintptr_t)a.B) & 15)) return STE_ERR_SHAPE;
  if (a.act >= STE_ACT_SWISH_BWD && !a.Z) return STE_ERR_ARG;
  if (!a.C && !a.C3) return STE_ERR_ARG;
  if (a.drop_ld == 0) a.drop_ld = a.N;
  hipStream_t s = (hipStream_t)stream;
  const F32Plan pl = plan_of(a);
  if (pl.S > 1) {
    launch<true, 2>(a, pl.S, pl.kc, s);
    STE_CHECK_LAUNCH();
    if (pl.wgrad) {
      const int64_t work = (int64_t)a.M * ((a.N + 3) / 4);
      const int blocks = (int)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
      hipLaunchKernelGGL(f32_slab_reduce_kernel, dim3(blocks), dim3(256), 0, s, (float*)a.C, a.ldc, a.ws, a.M, a.N,
                         pl.S, a.alpha, a.beta);
      STE_CHECK_LAUNCH();
      return 0;
    }
    const dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN);
    hipLaunchKernelGGL(gemm_f32_reduce_kernel, grid, dim3(NT), 0, s, a, pl.S);
    STE_CHECK_LAUNCH();
    if (pl.cs_rows)
      return ste_rowsum_ordered(a.ws + (int64_t)pl.S * a.M * a.N, pl.cs_rows, a.N, 1, a.colsum, stream);
    return 0;
  }
  if (!pl.cs_rows) a.ws = nullptr;
  if (pl.small) launch<false, 1>(a, 1, 0, s);
  else launch<false, 2>(a, 1, 0, s);
  STE_CHECK_LAUNCH();
  if (pl.cs_rows) return ste_rowsum_ordered(a.ws, pl.cs_rows, a.N, 1, a.colsum, stream);
  return 0;
}
