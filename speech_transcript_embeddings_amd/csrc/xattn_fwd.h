// The single-query cross attention forward kernel, shared by heads.hip (ste_xattn_fwd, the training
// and evaluation route) and xattn_mq.hip (ste_xattn_gather_fwd, the rerank route), so that both
// run the same VALU arithmetic in the same order.
#pragma once
#include "common.h"

constexpr int XATTN_NT = 256;  // threads of a block: 4 waves

// ---------------------------------------------------- single-query cross attention
// scores/probs layout: [B][nh][S]
// CrossModalAttention with NQ single-vector queries per sample sharing the same keys/values
// (the positive and the corrupted transcript's text->audio calls, ref:525-542, read one audio
// K/V): one block per (sample, head), so B*nh blocks fill the chip.  Query qi of sample b is
// row qi*B + b of q / out / dout / dq and of the probs ((qi*B + b)*nh + head)*S; its dropout
// uses seed qi and the index (b*nh + head)*S + s (the per-call layout of one query set).
// Rows of K/V are read with 16-B (8 x bf16) loads; the PV / dK / dV passes put 4 columns on a
// lane and spread the key rows over the block's row groups.
//
// GATHER (NQ = 1, drop_p = 0, probs unused): block b is pair b, whose query is row qrow[b] of q and
// whose keys/values/mask are block kvblk[b] (rows kvblk[b]*S + s); out row b.  A negative qrow or
// kvblk entry writes a zero row.  Only the addresses differ from the plain form.
template <int NQ, bool GATHER>
__global__ __launch_bounds__(XATTN_NT) void xattn_fwd_kernel(const float* q, const bf16* k, const bf16* v,
                                                           int64_t ldkv, const int32_t* mask, int B, int S, int P,
                                                           int nh, float scale, float drop_p, uint64_t seed0,
                                                           uint64_t seed1, float* probs, float* out,
                                                           const int32_t* qrow, const int32_t* kvblk) {
  constexpr int NT = XATTN_NT;
  static_assert(!GATHER || NQ == 1, "the gather form takes one query per pair");
  extern __shared__ float sp[];  // NQ * S
  __shared__ float sq[NQ][256];
  __shared__ float red[NQ][NT / 64];
  __shared__ f32x4 racc[NT];
  const int b = blockIdx.x, hh = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int dh = P / nh, c0 = hh * dh;
  const int qb = GATHER ? qrow[b] : b;   // row of q (query set 0)
  const int kb = GATHER ? kvblk[b] : b;  // block of S rows of k / v / mask
  if (GATHER && (qb < 0 || kb < 0)) {    // empty pair (uniform over the block)
    for (int c = tid; c < dh; c += NT) out[(int64_t)b * P + c0 + c] = 0.f;
    return;
  }
  for (int c = tid; c < NQ * dh; c += NT)
    sq[c / dh][c % dh] = q[(int64_t)(GATHER ? qb : (c / dh) * B + b) * P + c0 + c % dh];
  __syncthreads();
  // scores
  for (int s = tid; s < S; s += NT) {
    const bf16* kr = k + (int64_t)(kb * S + s) * ldkv + c0;
    float acc[NQ];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) acc[qi] = 0.f;
    for (int d = 0; d < dh; d += 8) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(kr + d);
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) acc[qi] += (float)x[e] * sq[qi][d + e];
    }
    const bool masked = mask && mask[kb * S + s] == 0;
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) sp[qi * S + s] = masked ? -1e9f : acc[qi] * scale;
  }
  __syncthreads();
  // softmax per query over the block
  float mx[NQ], sm[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    float m = -INFINITY;
    for (int s = tid; s < S; s += NT) m = fmaxf(m, sp[qi * S + s]);
    m = wave_max(m);
    if (lane == 0) red[qi][w] = m;
  }
  __syncthreads();
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    mx[qi] = fmaxf(fmaxf(red[qi][0], red[qi][1]), fmaxf(red[qi][2], red[qi][3]));
    float t = 0.f;
    for (int s = tid; s < S; s += NT) t += __expf(sp[qi * S + s] - mx[qi]);
    sm[qi] = wave_sum(t);
  }
  __syncthreads();
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi)
    if (lane == 0) red[qi][w] = sm[qi];
  __syncthreads();
  const uint32_t thresh = (uint32_t)(drop_p * 4294967296.0);
  const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const float inv = 1.f / (red[qi][0] + red[qi][1] + red[qi][2] + red[qi][3]);
    const uint64_t sd = qi ? seed1 : seed0;
    float* pr = probs + ((int64_t)(qi * B + b) * nh + hh) * S;
    for (int s = tid; s < S; s += NT) {
      float pv = __expf(sp[qi * S + s] - mx[qi]) * inv;
      if (!GATHER) pr[s] = pv;
      if (drop_p > 0.f) pv *= drop_scale(sd, ((uint64_t)b * nh + hh) * S + s, thresh, inv_keep);
      sp[qi * S + s] = pv;
    }
  }
  __syncthreads();
  // out = P·V: lane (row group rg, column quad cq)
  const int nq4 = dh >> 2, RG = NT / nq4;
  const int cq = tid % nq4, rg = tid / nq4;
  f32x4 acc[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) acc[qi] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (rg < RG)
    for (int s = rg; s < S; s += RG) {
      const f32x4 vv = load_bf16x4(v + (int64_t)(kb * S + s) * ldkv + c0 + 4 * cq);
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) acc[qi] += vv * sp[qi * S + s];
    }
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    racc[tid] = acc[qi];
    __syncthreads();
    if (tid < nq4) {
      f32x4 t = racc[tid];
      for (int r = 1; r < RG; ++r) t += racc[r * nq4 + tid];
      *reinterpret_cast<f32x4*>(out + (int64_t)(qi * B + b) * P + c0 + 4 * tid) = t;
    }
    __syncthreads();
  }
}
