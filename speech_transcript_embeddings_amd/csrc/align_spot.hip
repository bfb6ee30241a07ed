// Free-endpoint phrase spotting, forward only:
//   ste_align_spot   where inside a clip the phrase's tokens explain the audio better than a per-pair
//                    background: the monotone decode of csrc/align_infer.hip with both ends free, on
//                    the same frame-major emissions, one wave per pair.
#include "common.h"
#include "../../include/ste.h"

#include <float.h>

namespace {

constexpr int TMAX = 2048, LMAX = 256, PF = 8;   // the limits of ste_align_decode; emission rows in flight per lane

// Lane i of the wave owns phrase tokens TPL*i .. TPL*i + TPL - 1, i.e. columns lead + TPL*i + k: the
// columns are RELATIVE to lead, so that what enters token 0 is the `old` operand of the DPP shift and
// costs the dependent chain nothing.
// Branch-free (a branch around a load would make the compiler drain the rows in flight): a column
// >= L reads column 0 instead.  Its value is never used by a token below it, and only those count.
// VEC (lde % 4 == 0, lead % 4 == 0, 16-byte aligned rows): one 16-byte load, which for a lane
// straddling L reads up to 3 padding columns inside the row.
template <int TPL, bool VEC>
STE_DEV void load_row(const float* row, int c0, int L, float (&r)[TPL]) {
  if constexpr (VEC) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + (c0 < L ? c0 : 0));
#pragma unroll
    for (int k = 0; k < TPL; ++k) r[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < TPL; ++k) r[k] = row[c0 + k < L ? c0 + k : 0];
  }
}

// the value of lane - 1 (DPP wave_shr:1), +0.0 in lane 0: a hit may start at any frame for free
STE_DEV float from_lane_below_or_zero(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, false));
}

// One frame.  The dependent chain is align_decode's: DPP -> compare -> select -> add.  Beside it: the
// subtract of bg (on the loaded row) and the tracker of the best end (on the new D, read by nothing
// in the next frame); every lane tracks its own slot `last` (= (m - 1) % TPL, uniform), the lane that
// owns token m - 1 is read at the end.
template <int TPL>
STE_DEV void spot_step(float (&D)[TPL], const float (&e)[TPL], float bg, unsigned long long* advrow, int lane, int t,
                       int last, float& best, int& t_best) {
  const float up = from_lane_below_or_zero(D[TPL - 1]);
  unsigned long long wd[TPL];
#pragma unroll
  for (int k = TPL - 1; k >= 0; --k) {  // downwards: D[k - 1] is still step t - 1's
    const float left = k ? D[k - 1] : up;
    const bool adv = left > D[k];       // strict: a tie stays
    wd[k] = __ballot(adv);
    D[k] = (adv ? left : D[k]) + (e[k] - bg);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < TPL; ++k) advrow[k] = wd[k];
  }
  float v = D[0];
#pragma unroll
  for (int k = 1; k < TPL; ++k) v = last == k ? D[k] : v;
  const bool better = v > best;         // strict: the earliest frame that attains the maximum
  best = better ? v : best;
  t_best = better ? t : t_best;
}

template <int TPL, bool VEC>
__global__ __launch_bounds__(64) void align_spot_kernel(const float* emit, int64_t lde, const int32_t* ntok,
                                                      const int32_t* nfrm, const float* bgs, int lead, int L, int T,
                                                      int32_t* spans, int32_t* hit, float* score) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sadv[];  // [T][TPL]: bit i of word k = token TPL*i + k
  __shared__ int s_start[LMAX + 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int m = __builtin_amdgcn_readfirstlane(ntok[b]), F = __builtin_amdgcn_readfirstlane(nfrm[b]);
  int32_t* sp = spans + (int64_t)b * L * 2;
  bool found = !(m < 1 || m > L - lead || F < m || F > T);  // else an infeasible pair (uniform)
  float best = -INFINITY;
  int t_best = -1;
  if (found) {
    const float bg = bgs[b];
    const float* e = emit + (int64_t)b * T * lde;
    const int c0 = lead + lane * TPL, last = (m - 1) % TPL;
    float D[TPL], buf[PF][TPL];
#pragma unroll
    for (int k = 0; k < TPL; ++k) D[k] = -INFINITY;
#pragma unroll
    for (int j = 0; j < PF; ++j) load_row<TPL, VEC>(e + (int64_t)min(j, F - 1) * lde, c0, L, buf[j]);
    int t0 = 0;
    for (; t0 + PF <= F; t0 += PF) {  // buf[j] holds row t0 + j; its slot is refilled with row t0 + j + PF
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        spot_step<TPL>(D, buf[j], bg, sadv + (t0 + j) * TPL, lane, t0 + j, last, best, t_best);
        load_row<TPL, VEC>(e + (int64_t)min(t0 + j + PF, F - 1) * lde, c0, L, buf[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < PF - 1; ++j)
      if (t0 + j < F) spot_step<TPL>(D, buf[j], bg, sadv + (t0 + j) * TPL, lane, t0 + j, last, best, t_best);
    const int owner = (m - 1) / TPL;    // uniform: the lane of token m - 1
    best = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), owner));
    t_best = __builtin_amdgcn_readlane(t_best, owner);
    found = t_best >= 0;                // no D_t[m-1] above -inf: no hit
  }
  if (!found) {
    for (int l = lane; l < L; l += 64) { sp[2 * l] = -1; sp[2 * l + 1] = -1; }
    if (lane == 0) { hit[2 * b] = -1; hit[2 * b + 1] = -1; score[b] = best; }
    return;
  }
  if (lane == 0) {  // the walk back from (t_best, m - 1): s_start[j] = t for t downwards leaves each token's first frame
    int j = m - 1;
    s_start[m] = t_best + 1;
#pragma unroll 4  // the rows' addresses do not depend on j: their reads run ahead of the chain
    for (int t = t_best; t >= 0; --t) {
      s_start[j] = t;
      const unsigned long long* r = sadv + t * TPL;
      unsigned long long wd = r[0];
      if constexpr (TPL == 4) {
        const unsigned long long w1 = r[1], w2 = r[2], w3 = r[3];
        const int k = j & 3;
        wd = (k & 2) ? ((k & 1) ? w3 : w2) : ((k & 1) ? w1 : wd);
      }
      j -= (int)((wd >> (j / TPL)) & 1ull);
      if (j < 0) break;                 // token 0 advanced: the hit starts at t
    }
    for (; j >= 0; --j) s_start[j] = 0;  // only with emissions outside the contract: the walk ran out of frames
    hit[2 * b] = s_start[0];
    hit[2 * b + 1] = t_best + 1;
    score[b] = best;
  }
  __syncthreads();
  for (int l = lane; l < L; l += 64) {
    const int j = l - lead;
    const bool live = j >= 0 && j < m;
    sp[2 * l] = live ? s_start[j] : -1;
    sp[2 * l + 1] = live ? s_start[j + 1] : -1;
  }
}

}  // namespace

extern "C" int ste_align_spot(const float* emit, int64_t lde, const int32_t* ntok, const int32_t* nfrm, const float* bg,
                              int lead, int B, int L, int T, int32_t* spans, int32_t* hit, float* score, void* stream) {
  if (emit == nullptr || ntok == nullptr || nfrm == nullptr || bg == nullptr || spans == nullptr || hit == nullptr ||
      score == nullptr)
    return STE_ERR_ARG;
  if (B <= 0 || L <= 0 || T <= 0 || L > LMAX || T > TMAX || lde < L || lead < 0 || lead >= L) return STE_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (L <= 64) {
    hipLaunchKernelGGL((align_spot_kernel<1, false>), dim3(B), dim3(64), (size_t)T * 8, s, emit, lde, ntok, nfrm, bg,
                       lead, L, T, spans, hit, score);
  } else if (lde % 4 == 0 && lead % 4 == 0 && (uintptr_t)emit % 16 == 0) {
    hipLaunchKernelGGL((align_spot_kernel<4, true>), dim3(B), dim3(64), (size_t)T * 32, s, emit, lde, ntok, nfrm, bg,
                       lead, L, T, spans, hit, score);
  } else {
    hipLaunchKernelGGL((align_spot_kernel<4, false>), dim3(B), dim3(64), (size_t)T * 32, s, emit, lde, ntok, nfrm, bg,
                       lead, L, T, spans, hit, score);
  }
  STE_CHECK_LAUNCH();
  return 0;
}
