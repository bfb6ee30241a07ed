// Word timestamps from the alignment head, forward only:
//   ste_align_matrix_fwd  the head-averaged text->audio attention matrix of
//                         WordLevelAlignmentModule (ref:training/trainer_unfreeze.py:295,
//                         alignment_weights.mean(dim=1)), its frame-major log and the attention
//                         output, one block per query group looping over all heads so that
//                         per-head probabilities stay in LDS;
//   ste_align_matrix_seg_fwd  the same block for (query, segment) pairs over runs of rows of one K/V
//                         buffer, an AudioStateStore's alignment rows read in place;
//   ste_align_decode     the monotone (Viterbi) path through that log matrix, one wave per pair.
#include "common.h"
#include "../../include/ste.h"

#include <float.h>

namespace {

// QB, DMAX and each thread's arithmetic are csrc/align.hip's forward's.  The block is 16 waves, not
// its 4: a block here runs the heads one after the other, so there are nh times fewer blocks, and
// these latency-bound loops need the waves (B = 64, L = 64, P = 768: 3.30 -> 1.89 ms at T = 500,
// 18.7 -> 7.25 ms at T = 1500), and the output loop keeps VU value rows in flight where that
// kernel waits for each row in turn (-> 0.49 / 1.70 ms).  A thread's sums, and their
// order, depend on neither.
constexpr int NT = 1024, QB = 8, DMAX = 256, VU = 8;
constexpr int TMAX = 2048, DEC_LMAX = 256, PF = 8;   // decode: emission rows in flight per lane

// One block's work, shared by the dense and the segmented kernel: QB query rows from l0 of one query
// block against T consecutive K/V rows.  The arithmetic is one text; SEG selects how the seven
// addresses are formed.
//   SEG = false  the dense kernel's own expressions on the whole-batch pointers, clip / transcript b:
//                row b*L + l of q and out, row b*T + t of kv and kmask, matrix [B][L][T], emit [B][T][lde].
//   SEG = true   every pointer is already that of the block's pair (b = 0, no mask): row l of the query
//                block at q + l*ldq, row t of the segment at kv + t*ldkv, matrix [L][ldm], emit [T][lde],
//                out [L][ldo].  Inside the segment an element of kv is addressed by a 32-bit offset from
//                the (scalar) row pointer: the entry point refuses Tmax*ldkv + 2P >= 2^31.
// ss holds QB * T score rows, then QB * T running head sums: the layout depends on T alone.
template <bool SEG>
STE_DEV void align_matrix_block(const bf16* q, int64_t ldq, const bf16* kv, int64_t ldkv, const int32_t* kmask, int l0,
                                int b, int L, int T, int P, int nh, float scale, float inv_nh, float* matrix,
                                int64_t ldm, float* emit, int64_t lde, bf16* out, int64_t ldo, float* ss,
                                float (&sq)[QB][DMAX]) {
  float* sacc = ss + QB * T;
  const int ldk = (int)ldkv;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int d = P / nh;
  const int nq = min(QB, L - l0);
  for (int h = 0; h < nh; ++h) {
    __syncthreads();  // the previous head's readers of sq / ss
    for (int i = tid; i < QB * d; i += NT) {
      const int qi = i / d, c = i % d;
      sq[qi][c] = qi < nq ? (float)q[(int64_t)(b * L + l0 + qi) * ldq + h * d + c] * scale : 0.f;
    }
    __syncthreads();
    for (int t = tid; t < T; t += NT) {
      const bf16* kr = SEG ? kv + (t * ldk + h * d) : kv + (int64_t)(b * T + t) * ldkv + h * d;
      float acc[QB];
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) acc[qi] = 0.f;
      for (int c = 0; c < d; c += 8) {
        const bf16x8 kk = *reinterpret_cast<const bf16x8*>(kr + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float kf = (float)kk[e];
#pragma unroll
          for (int qi = 0; qi < QB; ++qi) acc[qi] += kf * sq[qi][c + e];
        }
      }
      const bool valid = SEG || kmask == nullptr || kmask[b * T + t] != 0;
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) ss[qi * T + t] = valid ? acc[qi] : -INFINITY;
    }
    __syncthreads();
    for (int qi = w; qi < nq; qi += NT / 64) {
      float* row = ss + qi * T;
      float* arow = sacc + qi * T;
      float mx = -INFINITY;
      for (int t = lane; t < T; t += 64) mx = fmaxf(mx, row[t]);
      mx = wave_max(mx);
      float sum = 0.f;
      for (int t = lane; t < T; t += 64) { const float e = __expf(row[t] - mx); row[t] = e; sum += e; }
      sum = wave_sum(sum);
      const float inv = 1.f / sum;
      for (int t = lane; t < T; t += 64) {
        const float p = row[t] * inv;
        row[t] = p;
        arow[t] = h == 0 ? p : arow[t] + p;  // heads in the order 0..nh-1
      }
    }
    __syncthreads();
    if (out != nullptr) {
      for (int i = tid; i < nq * d; i += NT) {
        const int qi = i / d, c = i % d;
        const float* pr = ss + qi * T;
        const bf16* vc = SEG ? kv + (P + h * d + c) : kv + (int64_t)(b * T) * ldkv + P + h * d + c;
        float acc = 0.f;
        int t = 0;
        for (; t + VU <= T; t += VU) {  // VU value rows in flight, then the same sums in the same order
          float v[VU];
#pragma unroll
          for (int u = 0; u < VU; ++u) v[u] = (float)(SEG ? vc[(t + u) * ldk] : vc[(int64_t)(t + u) * ldkv]);
#pragma unroll
          for (int u = 0; u < VU; ++u) acc += pr[t + u] * v[u];
        }
        for (; t < T; ++t) acc += pr[t] * (float)(SEG ? vc[t * ldk] : vc[(int64_t)t * ldkv]);
        out[(int64_t)(b * L + l0 + qi) * ldo + h * d + c] = (bf16)acc;
      }
    }
  }
  // sacc was last written before the barrier that precedes the out loop
  if (matrix != nullptr) {
    for (int i = tid; i < nq * T; i += NT) {
      const int qi = i / T, t = i % T;
      matrix[((int64_t)b * L + l0 + qi) * (SEG ? ldm : (int64_t)T) + t] = sacc[qi * T + t] * inv_nh;
    }
  }
  if (emit != nullptr) {  // frame-major: the nq columns of a frame are adjacent
    for (int i = tid; i < nq * T; i += NT) {
      const int t = i / nq, qi = i % nq;
      emit[((int64_t)b * T + t) * lde + l0 + qi] = logf(fmaxf(sacc[qi * T + t] * inv_nh, FLT_MIN));
    }
  }
}

// q bf16 [B*L, ldq], kv bf16 [B*T, ldkv]: block (x, b) owns queries QB*x .. of clip b
__global__ __launch_bounds__(NT) void align_matrix_kernel(const bf16* q, int64_t ldq, const bf16* kv, int64_t ldkv,
                                                        const int32_t* kmask, int L, int T, int P, int nh,
                                                        float scale, float inv_nh, float* matrix, float* emit,
                                                        int64_t lde, bf16* out, int64_t ldo) {
  extern __shared__ float ss[];
  __shared__ float sq[QB][DMAX];
  align_matrix_block<false>(q, ldq, kv, ldkv, kmask, blockIdx.x * QB, blockIdx.y, L, T, P, nh, scale, inv_nh, matrix, T,
                            emit, lde, out, ldo, ss, sq);
}

STE_DEV int64_t uniform64(int64_t v) {  // readfirstlane of both halves
  const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The segmented form: block (x, y) owns queries QB*x .. of pair r = r0 + y, which is query
// block qblk[r] of q against the F = seg_len[g] rows from seg_row[g] of kv, g = pseg[r]: the dense
// block at T = F, with the pair's rows of matrix [R, L, Tmax], emit [R, Tmax, lde] and out [R*L, ldo].
// An empty pair (a negative index, a segment outside [0, G), F == 0 or F > Tmax) zeroes its out
// rows, reads no row of q or kv and leaves matrix and emit alone.  The test is uniform per block.
__global__ __launch_bounds__(NT) void align_matrix_seg_kernel(const bf16* q, int64_t ldq, const int32_t* qblk,
                                                            const int32_t* pseg, const bf16* kv, int64_t ldkv,
                                                            const int64_t* seg_row, const int32_t* seg_len, int r0,
                                                            int G, int L, int Tmax, int P, int nh, float scale,
                                                            float inv_nh, float* matrix, float* emit, int64_t lde,
                                                            bf16* out, int64_t ldo) {
  extern __shared__ float ss[];
  __shared__ float sq[QB][DMAX];
  const int64_t r = (int64_t)r0 + blockIdx.y;
  const int l0 = blockIdx.x * QB;
  // the pair's table entries are the same in every lane: held in scalar registers (92 -> 63 vector registers)
  const int u = __builtin_amdgcn_readfirstlane(qblk[r]), g = __builtin_amdgcn_readfirstlane(pseg[r]);
  const int F = __builtin_amdgcn_readfirstlane(g >= 0 && g < G ? seg_len[g] : 0);
  if (u < 0 || F <= 0 || F > Tmax) {
    if (out != nullptr) {
      const int nq = min(QB, L - l0);
      for (int i = threadIdx.x; i < nq * P; i += NT) out[(r * L + l0 + i / P) * ldo + i % P] = (bf16)0.f;
    }
    return;
  }
  align_matrix_block<true>(q + (int64_t)u * L * ldq, ldq, kv + uniform64(seg_row[g]) * ldkv, ldkv, nullptr, l0, 0, L, F, P,
                           nh, scale, inv_nh, matrix == nullptr ? nullptr : matrix + r * L * Tmax, Tmax,
                           emit == nullptr ? nullptr : emit + r * Tmax * lde, lde,
                           out == nullptr ? nullptr : out + r * L * ldo, ldo, ss, sq);
}

// ------------------------------------------------------------------ monotone decode
// lane i of the wave owns tokens TPL*i .. TPL*i + TPL - 1
// Branch-free (a branch around a load would make the compiler drain the rows in flight): a token
// >= L reads column 0 instead.  Its value is never used by a token below it, and only those count.
// VEC (lde % 4 == 0, 16-byte aligned rows): one 16-byte load, which for a lane straddling L reads
// up to 3 padding columns inside the row.
template <int TPL, bool VEC>
STE_DEV void load_row(const float* row, int l0, int L, float (&r)[TPL]) {
  if constexpr (VEC) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + (l0 < L ? l0 : 0));
#pragma unroll
    for (int k = 0; k < TPL; ++k) r[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < TPL; ++k) r[k] = row[l0 + k < L ? l0 + k : 0];
  }
}

// the value of lane - 1 (DPP wave_shr:1), -inf in lane 0
STE_DEV float from_lane_below(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xFF800000u, __builtin_bit_cast(int, v), 0x138,
                                                               0xF, 0xF, false));
}

template <int TPL>
STE_DEV void decode_step(float (&D)[TPL], const float (&e)[TPL], unsigned long long* advrow, int lane) {
  const float up = from_lane_below(D[TPL - 1]);
  unsigned long long wd[TPL];
#pragma unroll
  for (int k = TPL - 1; k >= 0; --k) {  // downwards: D[k - 1] is still step t - 1's
    const float left = k ? D[k - 1] : up;
    const bool adv = left > D[k];       // strict: a tie stays
    wd[k] = __ballot(adv);
    D[k] = (adv ? left : D[k]) + e[k];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < TPL; ++k) advrow[k] = wd[k];
  }
}

template <int TPL, bool VEC>
__global__ __launch_bounds__(64) void align_decode_kernel(const float* emit, int64_t lde, const int32_t* ntok,
                                                        const int32_t* nfrm, int L, int T, int32_t* spans,
                                                        float* score) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sadv[];  // [T][TPL]: bit i of word k = token TPL*i + k
  __shared__ int s_start[DEC_LMAX + 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = ntok[b], F = nfrm[b];
  int32_t* sp = spans + (int64_t)b * L * 2;
  if (n < 1 || n > L || F < n || F > T) {  // infeasible pair (uniform)
    for (int l = lane; l < L; l += 64) { sp[2 * l] = -1; sp[2 * l + 1] = -1; }
    if (lane == 0) score[b] = -INFINITY;
    return;
  }
  const float* e = emit + (int64_t)b * T * lde;
  const int l0 = lane * TPL;
  float D[TPL], buf[PF][TPL];
  load_row<TPL, VEC>(e, l0, L, D);
#pragma unroll
  for (int k = 0; k < TPL; ++k) D[k] = l0 + k == 0 ? D[k] : -INFINITY;
#pragma unroll
  for (int j = 0; j < PF; ++j) load_row<TPL, VEC>(e + (int64_t)min(1 + j, F - 1) * lde, l0, L, buf[j]);
  int t0 = 1;
  for (; t0 + PF <= F; t0 += PF) {  // buf[j] holds row t0 + j; its slot is refilled with row t0 + j + PF
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      decode_step<TPL>(D, buf[j], sadv + (t0 + j) * TPL, lane);
      load_row<TPL, VEC>(e + (int64_t)min(t0 + j + PF, F - 1) * lde, l0, L, buf[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < PF - 1; ++j)
    if (t0 + j < F) decode_step<TPL>(D, buf[j], sadv + (t0 + j) * TPL, lane);
  {
    const int k = (n - 1) % TPL;
    float v = D[0];
#pragma unroll
    for (int kk = 1; kk < TPL; ++kk) v = k == kk ? D[kk] : v;
    if (lane == (n - 1) / TPL) score[b] = v;
  }
  if (lane == 0) {  // the walk back: s_start[l(t)] = t for t downwards leaves each token's first frame
    int l = n - 1;
    s_start[n] = F;
#pragma unroll 4  // the rows' addresses do not depend on l: their reads run ahead of the chain
    for (int t = F - 1; t >= 1; --t) {
      s_start[l] = t;
      const unsigned long long* r = sadv + t * TPL;
      unsigned long long wd = r[0];
      if constexpr (TPL == 4) {
        const unsigned long long w1 = r[1], w2 = r[2], w3 = r[3];
        const int k = l & 3;
        wd = (k & 2) ? ((k & 1) ? w3 : w2) : ((k & 1) ? w1 : wd);
      }
      l -= (int)((wd >> (l / TPL)) & 1ull);
    }
    s_start[0] = 0;  // frame 0 is token 0's
  }
  __syncthreads();
  for (int l = lane; l < L; l += 64) {
    const bool live = l < n;
    sp[2 * l] = live ? s_start[l] : -1;
    sp[2 * l + 1] = live ? s_start[l + 1] : -1;
  }
}

// Dynamic LDS of a matrix kernel: beyond what every device grants, ask this one and raise the
// kernel's limit.  0, STE_ERR_SHAPE when the device cannot hold it, or the runtime's error.
int matrix_lds(const void* kernel, size_t lds) {
  if (lds <= 48 * 1024) return 0;
  int dev = 0, lim = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) return (int)e;
  if (lds + sizeof(float) * QB * DMAX > (size_t)lim) return STE_ERR_SHAPE;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" int ste_align_matrix_fwd(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const int32_t* kmask,
                                    int B, int L, int T, int P, int nh, float* matrix, float* emit, int64_t lde,
                                    void* out, int64_t ldo, void* stream) {
  if (matrix == nullptr && emit == nullptr && out == nullptr) return STE_ERR_ARG;
  if (B <= 0 || L <= 0 || T <= 0 || nh <= 0 || P <= 0 || P % nh) return STE_ERR_SHAPE;
  const int d = P / nh;
  if (d > DMAX || d % 8 || T > TMAX || B > 65535 || (emit != nullptr && lde < L)) return STE_ERR_SHAPE;
  const size_t lds = (size_t)2 * QB * T * sizeof(float);
  if (const int rc = matrix_lds(reinterpret_cast<const void*>(align_matrix_kernel), lds)) return rc;
  hipLaunchKernelGGL(align_matrix_kernel, dim3((L + QB - 1) / QB, B), dim3(NT), lds, (hipStream_t)stream,
                     (const bf16*)q, ldq, (const bf16*)kv, ldkv, kmask, L, T, P, nh, 1.0f / sqrtf((float)d),
                     1.0f / (float)nh, matrix, emit, lde, (bf16*)out, ldo);
  STE_CHECK_LAUNCH();
  return 0;
}

extern "C" int ste_align_matrix_seg_fwd(const void* q, int64_t ldq, const int32_t* qblk, const int32_t* pseg,
                                        const void* kv, int64_t ldkv, const int64_t* seg_row, const int32_t* seg_len,
                                        int R, int G, int L, int Tmax, int P, int nh, float* matrix, float* emit,
                                        int64_t lde, void* out, int64_t ldo, void* stream) {
  if (q == nullptr || qblk == nullptr || pseg == nullptr || kv == nullptr || seg_row == nullptr || seg_len == nullptr)
    return STE_ERR_ARG;
  if (matrix == nullptr && emit == nullptr && out == nullptr) return STE_ERR_ARG;
  if (R <= 0 || G <= 0 || L <= 0 || Tmax <= 0 || nh <= 0 || P <= 0 || P % nh) return STE_ERR_SHAPE;
  const int d = P / nh;
  if (d > DMAX || d % 8 || Tmax > TMAX) return STE_ERR_SHAPE;
  if (ldq < P || ldkv < 2 * (int64_t)P || ldkv % 8 || (uintptr_t)kv % 16) return STE_ERR_SHAPE;  // 16-byte key loads
  if ((int64_t)Tmax * ldkv + 2 * (int64_t)P > INT32_MAX) return STE_ERR_SHAPE;      // 32-bit offsets inside a segment
  if ((emit != nullptr && lde < L) || (out != nullptr && ldo < P)) return STE_ERR_SHAPE;
  const size_t lds = (size_t)2 * QB * Tmax * sizeof(float);
  if (const int rc = matrix_lds(reinterpret_cast<const void*>(align_matrix_seg_kernel), lds)) return rc;
  const float scale = 1.0f / sqrtf((float)d), inv_nh = 1.0f / (float)nh;
  for (int r0 = 0; r0 < R; r0 += 65535) {  // the pair rides grid.y
    hipLaunchKernelGGL(align_matrix_seg_kernel, dim3((L + QB - 1) / QB, min(R - r0, 65535)), dim3(NT), lds,
                       (hipStream_t)stream, (const bf16*)q, ldq, qblk, pseg, (const bf16*)kv, ldkv, seg_row, seg_len,
                       r0, G, L, Tmax, P, nh, scale, inv_nh, matrix, emit, lde, (bf16*)out, ldo);
    STE_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int ste_align_decode(const float* emit, int64_t lde, const int32_t* ntok, const int32_t* nfrm, int B,
                                int L, int T, int32_t* spans, float* score, void* stream) {
  if (emit == nullptr || ntok == nullptr || nfrm == nullptr || spans == nullptr || score == nullptr)
    return STE_ERR_ARG;
  if (B <= 0 || L <= 0 || T <= 0 || L > DEC_LMAX || T > TMAX || lde < L) return STE_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (L <= 64) {
    hipLaunchKernelGGL((align_decode_kernel<1, false>), dim3(B), dim3(64), (size_t)T * 8, s, emit, lde, ntok, nfrm,
                       L, T, spans, score);
  } else if (lde % 4 == 0 && (uintptr_t)emit % 16 == 0) {
    hipLaunchKernelGGL((align_decode_kernel<4, true>), dim3(B), dim3(64), (size_t)T * 32, s, emit, lde, ntok, nfrm,
                       L, T, spans, score);
  } else {
    hipLaunchKernelGGL((align_decode_kernel<4, false>), dim3(B), dim3(64), (size_t)T * 32, s, emit, lde, ntok, nfrm,
                       L, T, spans, score);
  }
  STE_CHECK_LAUNCH();
  return 0;
}
