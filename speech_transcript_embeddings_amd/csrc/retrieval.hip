// Corpus retrieval: fused similarity + top-k selection, the merge of candidate
// lists, and the 0-based rank of a target row.  The score matrix S = Q·Cᵀ is never written.
//
//   ste_topk_sim_plan     host-only: split count and workspace bytes
//   ste_topk_sim          k best corpus rows per query (+ rank of a target row)
//   ste_topk_target_score the target rows' scores, by the same MFMA chain as the scan
//   ste_topk_merge        L candidate lists per query -> one list; rank counts summed
//
// Scores run on v_mfma_f32_16x16x4_f32 like similarity_kernel (heads.hip): a score is an fmaf
// chain over k = 0, 1, 2, ... starting from +0, so it depends on its two rows only (zero-filled
// k tails add fma(0, 0, acc) = acc) and is bit-identical in every tile, split, chunk and kernel
// of this file.  The order is total: value descending, then index ascending.
#include "common.h"
#include "ste.h"

namespace rtv {
constexpr int NT = 256;             // 4 waves
constexpr int QT = 32;              // queries held in LDS per block
constexpr int CT = 64;              // corpus rows per tile
constexpr int KC = 32;              // k per staged chunk
constexpr int SLD = KC + 2;         // staged row stride: ld % 32 == 2 -> the 16 rows x 2 k of a
                                    // 32-lane half of ds_read_b32 fall on 32 distinct banks
constexpr int SCLD = CT + 1;        // score tile row stride
constexpr int RPW = QT / 4;         // query rows whose lists one wave owns
constexpr int KMAX = 128, PMAX = 1024;
constexpr int IDX_NONE = 0x7fffffff;  // index of an empty list entry (orders last); -1 on output
constexpr int MERGE_TILE = 1024;
constexpr int CUS = 256;

STE_HD int kpad(int P) { return (P + KC - 1) / KC * KC; }
STE_HD int ldq(int P) { return kpad(P) + 2; }
STE_HD int64_t lds_floats(int P) { return (int64_t)QT * ldq(P) + 2 * CT * SLD + QT * SCLD; }

STE_DEV float readlane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// (va, ia) orders before (vb, ib)
STE_DEV bool before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// 8 corpus elements [k0, k0 + 8) of one row as fp32 (bf16 widens exactly); zero past P
template <bool BF>
STE_DEV void load8(const void* corpus, int64_t row, int P, int k0, bool vec, float (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = 0.f;
  if (k0 >= P) return;
  if constexpr (BF) {
    const bf16* p = (const bf16*)corpus + row * P + k0;
    if (vec) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = (float)v[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (k0 + i < P) r[i] = (float)p[i];
    }
  } else {
    const float* p = (const float*)corpus + row * P + k0;
    if (vec) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { r[i] = a[i]; r[4 + i] = b[i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (k0 + i < P) r[i] = p[i];
    }
  }
}

// Sorted list of up to 128 (value, index) per query row, held by one wave: entry e lives in
// lane e & 63 of register e >> 6.  Insert (cv, ci) at its place; entries behind it move down one.
STE_DEV void list_insert(float& v0, int& i0, float& v1, int& i1, float cv, int ci, int lane) {
  const int p = __popcll(__ballot(before(v0, i0, cv, ci))) + __popcll(__ballot(before(v1, i1, cv, ci)));
  const float cv63 = readlane_f(v0, 63);
  const int ci63 = __builtin_amdgcn_readlane(i0, 63);
  float u0 = __shfl_up(v0, 1, 64), u1 = __shfl_up(v1, 1, 64);
  int j0 = __shfl_up(i0, 1, 64), j1 = __shfl_up(i1, 1, 64);
  if (lane == 0) { u1 = cv63; j1 = ci63; }
  const int e0 = lane, e1 = lane + 64;
  v0 = e0 < p ? v0 : (e0 == p ? cv : u0);
  i0 = e0 < p ? i0 : (e0 == p ? ci : j0);
  v1 = e1 < p ? v1 : (e1 == p ? cv : u1);
  i1 = e1 < p ? i1 : (e1 == p ? ci : j1);
}

// One block: QT queries x one slice of the corpus (blockIdx.y of S slices, whole tiles of CT
// rows).  Waves (mt, ch) = (wave & 1, wave >> 1) compute the 16-query x 32-row quarter of each
// 32 x 64 score tile; the tile goes through LDS and wave w then selects for query rows 8w..8w+7
// with lane = corpus column.
template <bool BF>
__global__ __launch_bounds__(NT) void topk_sim_kernel(const float* __restrict__ q, const void* __restrict__ corpus,
                                                     int Q, int N, int P, int k, int index_base,
                                                     const int* __restrict__ target, const float* __restrict__ tscore,
                                                     int S, int tiles_per_split, int vec, float* __restrict__ out_v,
                                                     int* __restrict__ out_i, int* __restrict__ out_c) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KP = kpad(P), LDQ = KP + 2, nkc = KP / KC;
  float* sQ = sm;                      // [QT][LDQ]
  float* sB = sQ + QT * LDQ;           // [2][CT][SLD]
  float* sS = sB + 2 * CT * SLD;       // [QT][SCLD]
  const int q0 = blockIdx.x * QT, split = blockIdx.y;
  const int ntiles = (N + CT - 1) / CT;
  const int t_begin = min(ntiles, split * tiles_per_split), t_end = min(ntiles, t_begin + tiles_per_split);
  const int total = (t_end - t_begin) * nkc;

  for (int i = tid; i < QT * KP; i += NT) {
    const int r = i / KP, c = i - r * KP;
    sQ[r * LDQ + c] = (q0 + r < Q && c < P) ? q[(int64_t)(q0 + r) * P + c] : 0.f;
  }

  // per-wave selection state (static indices only: these stay in registers)
  float lv0[RPW], lv1[RPW], thr[RPW], ts[RPW];
  int li0[RPW], li1[RPW], cnt[RPW], tg[RPW];
  const int kth = k - 1;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    lv0[r] = lv1[r] = thr[r] = -INFINITY;
    li0[r] = li1[r] = IDX_NONE;
    cnt[r] = 0;
    const int qi = q0 + wave * RPW + r;
    tg[r] = (target && qi < Q) ? target[qi] : -1;
    ts[r] = tg[r] >= 0 ? tscore[qi] : 0.f;
  }

  const int srow = tid >> 2, sseg = (tid & 3) * 8;   // staging: 4 threads per corpus row
  const int mt = wave & 1, ch = wave >> 1;
  float stage[8];
  if (total > 0) {
    const int n = t_begin * CT + srow;
    if (n < N) load8<BF>(corpus, n, P, sseg, vec, stage);
    else {
#pragma unroll
      for (int i = 0; i < 8; ++i) stage[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) sB[srow * SLD + sseg + i] = stage[i];
  }
  __syncthreads();

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int tile = t_begin, kc = 0;
  for (int c = 0; c < total; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < total;
    if (more) {   // next chunk's global loads fly over this chunk's MFMAs
      const int ntile = kc + 1 == nkc ? tile + 1 : tile, nk = kc + 1 == nkc ? 0 : kc + 1;
      const int n = ntile * CT + srow;
      if (n < N) load8<BF>(corpus, n, P, nk * KC + sseg, vec, stage);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) stage[i] = 0.f;
      }
    }
    const float* ap = sQ + (mt * 16 + (lane & 15)) * LDQ + kc * KC + (lane >> 4);
    const float* bp = sB + buf * CT * SLD + (ch * 32 + (lane & 15)) * SLD + (lane >> 4);
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      const float a = ap[4 * s], b0 = bp[4 * s], b1 = bp[16 * SLD + 4 * s];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
    }
    if (kc + 1 == nkc) {   // tile done: scores -> LDS, then row-per-wave selection
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* d = sS + (mt * 16 + (lane >> 4) * 4 + r) * SCLD + ch * 32 + (lane & 15);
        d[0] = acc0[r];
        d[16] = acc1[r];
      }
      acc0 = f32x4{0.f, 0.f, 0.f, 0.f};
      acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
      __syncthreads();
      const int n = tile * CT + lane;
      const bool valid = n < N;
      const int gi = index_base + n;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int row = wave * RPW + r;
        if (q0 + row < Q) {
          const float v = sS[row * SCLD + lane];
          if (tg[r] >= 0) cnt[r] += (valid && before(v, gi, ts[r], tg[r])) ? 1 : 0;
          // indices arrive ascending, so a tie with the k-th entry loses: strict >
          unsigned long long m = __ballot(valid && v > thr[r]);
          while (m) {
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
            m &= m - 1;
            const float cv = readlane_f(v, l);
            if (cv > thr[r]) {
              list_insert(lv0[r], li0[r], lv1[r], li1[r], cv, index_base + tile * CT + l, lane);
              thr[r] = kth < 64 ? readlane_f(lv0[r], kth) : readlane_f(lv1[r], kth - 64);
            }
          }
        }
      }
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sB[(buf ^ 1) * CT * SLD + srow * SLD + sseg + i] = stage[i];
    }
    __syncthreads();
    if (++kc == nkc) { kc = 0; ++tile; }
  }

#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int qi = q0 + wave * RPW + r;
    if (qi >= Q) continue;
    const int64_t o = ((int64_t)qi * S + split) * k;
    if (lane < k) { out_v[o + lane] = lv0[r]; out_i[o + lane] = li0[r] == IDX_NONE ? -1 : li0[r]; }
    if (lane + 64 < k) { out_v[o + lane + 64] = lv1[r]; out_i[o + lane + 64] = li1[r] == IDX_NONE ? -1 : li1[r]; }
    if (out_c) {
      int s = cnt[r];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
      if (lane == 0) out_c[(int64_t)qi * S + split] = tg[r] >= 0 ? s : -1;
    }
  }
}

// Score of each query against its target row, 16 queries per wave: the diagonal of the 16x16
// MFMA tile whose B rows are the targets.  Writes only where the target lies in
// [index_base, index_base + N); tgt_eff (optional) gets the target there and -1 elsewhere.
template <bool BF>
__global__ __launch_bounds__(64) void topk_tscore_kernel(const float* __restrict__ q, const void* __restrict__ corpus,
                                                       int Q, int N, int P, int index_base,
                                                       const int* __restrict__ target, float* __restrict__ tscore,
                                                       int* __restrict__ tgt_eff) {
  const int lane = threadIdx.x, qi = blockIdx.x * 16 + (lane & 15), kk = lane >> 4;
  const int t = qi < Q ? target[qi] : -1;
  const int64_t loc = (int64_t)t - index_base;
  const bool in = t >= 0 && loc >= 0 && loc < N;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < P; k += 4) {
    const bool kin = k + kk < P;
    const float a = (qi < Q && kin) ? q[(int64_t)qi * P + k + kk] : 0.f;
    float b = 0.f;
    if (in && kin) {
      if constexpr (BF) b = (float)((const bf16*)corpus)[loc * P + k + kk];
      else b = ((const float*)corpus)[loc * P + k + kk];
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const int r = (lane & 15) - (lane >> 4) * 4;   // D[row = (lane>>4)*4 + r][col = lane&15]: the diagonal
  if (r >= 0 && r < 4 && qi < Q) {
    const float d = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    if (in) tscore[qi] = d;
    if (tgt_eff) tgt_eff[qi] = in ? t : -1;
  }
}

// One block per query: each candidate's output position is the number of candidates that order
// before it (value desc, index asc, then position in the input), so the result does not depend
// on the order the lists come in and needs no atomics.
__global__ __launch_bounds__(NT) void topk_merge_kernel(const float* __restrict__ v, const int* __restrict__ idx, int C,
                                                      int k, const int* __restrict__ counts, int L,
                                                      float* __restrict__ ov, int* __restrict__ oi,
                                                      int* __restrict__ orank) {
  __shared__ float sv[MERGE_TILE];
  __shared__ int si[MERGE_TILE];
  const int qi = blockIdx.x, tid = threadIdx.x;
  const float* vq = v + (int64_t)qi * C;
  const int* iq = idx + (int64_t)qi * C;
  for (int cb = 0; cb < C; cb += NT) {
    const int c = cb + tid;
    const bool have = c < C;
    const float mv = have ? vq[c] : 0.f;
    int mi = have ? iq[c] : 0;
    if (mi < 0) mi = IDX_NONE;
    int pos = 0;
    for (int t0 = 0; t0 < C; t0 += MERGE_TILE) {
      const int tn = min(MERGE_TILE, C - t0);
      __syncthreads();
      for (int j = tid; j < tn; j += NT) {
        sv[j] = vq[t0 + j];
        const int x = iq[t0 + j];
        si[j] = x < 0 ? IDX_NONE : x;
      }
      __syncthreads();
      if (have)
        for (int j = 0; j < tn; ++j) {
          const float a = sv[j];
          const int ai = si[j];
          pos += (a > mv || (a == mv && (ai < mi || (ai == mi && t0 + j < c)))) ? 1 : 0;
        }
    }
    if (have && pos < k) {
      ov[(int64_t)qi * k + pos] = mv;
      oi[(int64_t)qi * k + pos] = mi == IDX_NONE ? -1 : mi;
    }
  }
  for (int e = C + tid; e < k; e += NT) {
    ov[(int64_t)qi * k + e] = -INFINITY;
    oi[(int64_t)qi * k + e] = -1;
  }
  if (orank && tid == 0) {
    int s = 0;
    bool none = false;
    for (int l = 0; l < L; ++l) {
      const int x = counts[(int64_t)qi * L + l];
      none |= x < 0;
      s += x;
    }
    orank[qi] = none ? -1 : s;
  }
}

struct Plan {
  int S, tiles_per_split;
  int64_t ws_bytes;
};

static int make_plan(int Q, int N, int P, int k, int splits, Plan* pl) {
  if (Q <= 0 || N <= 0 || P <= 0 || splits < 0) return STE_ERR_ARG;
  if (k < 1 || k > KMAX) return STE_ERR_ARG;
  if (P > PMAX) return STE_ERR_SHAPE;
  const int qtiles = (Q + QT - 1) / QT, ntiles = (N + CT - 1) / CT;
  int S;
  if (splits > 0) S = splits < ntiles ? splits : ntiles;
  else {
    // two blocks per CU when the queries alone cannot give them, at least 8 tiles per slice so
    // that a block's query-tile load and list warm-up stay small beside its scan
    S = (2 * CUS + qtiles - 1) / qtiles;
    const int cap = ntiles / 8 > 1 ? ntiles / 8 : 1;
    S = S < cap ? S : cap;
  }
  if (S > 65535) S = 65535;
  pl->S = S;
  pl->tiles_per_split = (ntiles + S - 1) / S;
  pl->ws_bytes = (int64_t)Q * 8 + (S > 1 ? (int64_t)Q * S * (8 * k + 4) : 0);
  return STE_OK;
}
}  // namespace rtv

extern "C" int ste_topk_sim_plan(int Q, int N, int P, int k, int splits, int* splits_out, int64_t* ws_bytes) {
  rtv::Plan pl;
  const int rc = rtv::make_plan(Q, N, P, k, splits, &pl);
  if (rc != STE_OK) return rc;
  if (splits_out) *splits_out = pl.S;
  if (ws_bytes) *ws_bytes = pl.ws_bytes;
  return STE_OK;
}

extern "C" int ste_topk_target_score(const float* q, const void* corpus, int corpus_bf16, int Q, int N, int P,
                                     int index_base, const int32_t* target, float* tscore, void* stream) {
  if (Q <= 0 || N <= 0 || P <= 0 || index_base < 0 || (int64_t)index_base + N > 0x7fffffffll) return STE_ERR_ARG;
  if (!q || !corpus || !target || !tscore) return STE_ERR_ARG;
  const dim3 grid((Q + 15) / 16);
  if (corpus_bf16)
    hipLaunchKernelGGL(rtv::topk_tscore_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, q, corpus, Q, N, P,
                       index_base, target, tscore, (int*)nullptr);
  else
    hipLaunchKernelGGL(rtv::topk_tscore_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, q, corpus, Q, N, P,
                       index_base, target, tscore, (int*)nullptr);
  STE_CHECK_LAUNCH();
  return STE_OK;
}

extern "C" int ste_topk_merge(const float* vals, const int32_t* idx, int Q, int C, int k, const int32_t* counts,
                              int L, float* out_v, int32_t* out_i, int32_t* out_rank, void* stream) {
  if (Q <= 0 || C <= 0 || k < 1 || k > rtv::KMAX) return STE_ERR_ARG;
  if (!vals || !idx || !out_v || !out_i) return STE_ERR_ARG;
  if ((counts != nullptr) != (out_rank != nullptr) || (counts && L <= 0)) return STE_ERR_ARG;
  hipLaunchKernelGGL(rtv::topk_merge_kernel, dim3(Q), dim3(rtv::NT), 0, (hipStream_t)stream, vals, idx, C, k, counts,
                     L, out_v, out_i, out_rank);
  STE_CHECK_LAUNCH();
  return STE_OK;
}

extern "C" int ste_topk_sim(const float* q, const void* corpus, int corpus_bf16, int Q, int N, int P, int k,
                            int index_base, const int32_t* target, const float* tscore, int splits, float* values,
                            int32_t* indices, int32_t* rank, void* ws, int64_t ws_bytes, void* stream) {
  using namespace rtv;
  Plan pl;
  const int rc = make_plan(Q, N, P, k, splits, &pl);
  if (rc != STE_OK) return rc;
  if (index_base < 0 || (int64_t)index_base + N > 0x7fffffffll) return STE_ERR_ARG;
  if (!q || !corpus || !values || !indices) return STE_ERR_ARG;
  if ((target != nullptr) != (rank != nullptr) || (tscore && !target)) return STE_ERR_ARG;
  if (!ws || ws_bytes < pl.ws_bytes) return STE_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // workspace: target scores [Q] f32, effective targets [Q] i32, then the partial lists
  float* ts_ws = (float*)ws;
  int* tg_ws = (int*)(ts_ws + Q);
  float* pv = (float*)(tg_ws + Q);
  int* pi = (int*)(pv + (int64_t)Q * pl.S * k);
  int* pc = pi + (int64_t)Q * pl.S * k;
  const int* tg = target;
  const float* ts = tscore;
  if (target && !tscore) {   // targets of this corpus: their scores by the same chain; others count as none
    const dim3 g((Q + 15) / 16);
    if (corpus_bf16)
      hipLaunchKernelGGL(topk_tscore_kernel<true>, g, dim3(64), 0, s, q, corpus, Q, N, P, index_base, target, ts_ws,
                         tg_ws);
    else
      hipLaunchKernelGGL(topk_tscore_kernel<false>, g, dim3(64), 0, s, q, corpus, Q, N, P, index_base, target, ts_ws,
                         tg_ws);
    STE_CHECK_LAUNCH();
    tg = tg_ws;
    ts = ts_ws;
  }
  const bool direct = pl.S == 1;
  float* ov = direct ? values : pv;
  int* oi = direct ? indices : pi;
  int* oc = target ? (direct ? rank : pc) : nullptr;
  const int vec = (P % 8 == 0) && ((uintptr_t)corpus % 16 == 0);
  const dim3 grid((Q + QT - 1) / QT, pl.S);
  const size_t lds = (size_t)lds_floats(P) * sizeof(float);
  if (corpus_bf16)
    hipLaunchKernelGGL(topk_sim_kernel<true>, grid, dim3(NT), lds, s, q, corpus, Q, N, P, k, index_base, tg, ts, pl.S,
                       pl.tiles_per_split, vec, ov, oi, oc);
  else
    hipLaunchKernelGGL(topk_sim_kernel<false>, grid, dim3(NT), lds, s, q, corpus, Q, N, P, k, index_base, tg, ts, pl.S,
                       pl.tiles_per_split, vec, ov, oi, oc);
  STE_CHECK_LAUNCH();
  if (!direct) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3(Q), dim3(NT), 0, s, (const float*)pv, (const int*)pi, pl.S * k, k,
                       (const int*)(target ? pc : nullptr), pl.S, values, indices, target ? rank : (int*)nullptr);
    STE_CHECK_LAUNCH();
  }
  return STE_OK;
}
