// Word timestamps from the alignment head, forward only:
//   ste_align_matrix_fwd  the head-averaged text->audio attention matrix of
//                         WordLevelAlignmentModule (ref:training/trainer_unfreeze.py:295,
//                         alignment_weights.mean(dim=1)), its frame-major log and the attention
//                         output, one block per query group looping over all heads so that
//                         per-head probabilities stay in LDS;
//   ste_align_matrix_seg_fwd  the same block for (query, segment) pairs over runs of rows of one K/V
//                         buffer, an AudioStateStore's alignment rows read in place;
//   ste_align_matrix_seg_mx8_fwd  the same on rows stored as MX-fp8 (e4m3 bytes + one E8M0 scale per
//                         32 columns): the bits of the bf16 kernel on the dequantised rows;
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
// MX: key fragments loaded together in the score loop; queries per thread (of QB) and value rows in
// flight in the out loop.  Out loop at Q = 64, k = 10, P = 768, 4 heads, T = 500 / 1500, one launch of 640
// pairs: MXQ = 2, MXU = 16: 4.28 / 13.1 ms; 8, 32: 5.68 / 16.2; 4, 16: 13.0 / 38.4; 4, 32:
// 12.0 / 35.1 (the bf16 kernel: 5.46 / 16.5).  MXK = 1 -> 4: the kernel without out 1.57 -> 1.35 / 9.45 -> 4.54.
constexpr int MXK = 4;
constexpr int MXQ = 2;
constexpr int MXU = 16;
static_assert(QB % MXQ == 0, "a group's queries are split evenly over the threads of a column");

template <bool MX> struct kv_elem { typedef bf16 type; };
template <> struct kv_elem<true> { typedef uint8_t type; };

// 8 key columns from c of one row against the QB scaled query rows: 64 FMAs, column by column
STE_DEV void score_fragment(float (&acc)[QB], bf16x8 kk, const float (&sq)[QB][DMAX], int c) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float kf = (float)kk[e];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) acc[qi] += kf * sq[qi][c + e];
  }
}

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
//   MX (with SEG)  kv is e4m3 bytes (ldkv in bytes) and sc row 0 of the segment's E8M0 scales, row stride
//                lsc bytes, one scale per 32 columns of [K | V].  The code differs where an
//                element enters a register and nowhere else: a key fragment comes through mx8_dequant8
//                as the bf16x8 the bf16 code loads, a value element through mx8_dequant1 as the bf16 it
//                loads.  The out loop gives a thread one value column and MXQ queries of the group
//                (one byte and one scale byte per value row, MXU rows in flight, dequantised once and
//                used MXQ times) where the bf16 code gives it one column of one query: an output
//                element is still one fp32 sum of p_t * v_t in ascending t, so its bits are the same
//                whichever thread holds it.
template <bool SEG, bool MX = false>
STE_DEV void align_matrix_block(const bf16* q, int64_t ldq, const typename kv_elem<MX>::type* kv, int64_t ldkv,
                                const uint8_t* sc, int lsc, const int32_t* kmask, int l0, int b, int L, int T, int P,
                                int nh, float scale, float inv_nh, float* matrix, int64_t ldm, float* emit,
                                int64_t lde, bf16* out, int64_t ldo, float* ss, float (&sq)[QB][DMAX]) {
  static_assert(SEG || !MX, "MX rows are read by the segmented kernel only");
  typedef typename kv_elem<MX>::type kv_t;
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
      const kv_t* kr = SEG ? kv + (t * ldk + h * d) : kv + (int64_t)(b * T + t) * ldkv + h * d;
      float acc[QB];
#pragma unroll
      for (int qi = 0; qi < QB; ++qi) acc[qi] = 0.f;
      if constexpr (MX) {
        // MXK fragments (32 columns) are loaded together, then used in the same order: a lane's
        // fragments share a cache line, and between two fragments' 64 FMAs the other waves' rows
        // would evict it (the bf16 code makes half as many loads for the same columns)
        for (int c0 = 0; c0 < d; c0 += 8 * MXK) {
          uint2 raw[MXK];
          uint32_t E[MXK];
#pragma unroll
          for (int j = 0; j < MXK; ++j) {
            if (c0 + 8 * j < d) {
              raw[j] = *reinterpret_cast<const uint2*>(kr + c0 + 8 * j);
              E[j] = sc[t * lsc + ((h * d + c0 + 8 * j) >> 5)];
            }
          }
#pragma unroll
          for (int j = 0; j < MXK; ++j) {
            if (c0 + 8 * j < d) score_fragment(acc, mx8_dequant8(raw[j], E[j]), sq, c0 + 8 * j);
          }
        }
      } else {
        for (int c = 0; c < d; c += 8) score_fragment(acc, *reinterpret_cast<const bf16x8*>(kr + c), sq, c);
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
    if constexpr (MX) {
      if (out != nullptr) {
        for (int i = tid; i < (QB / MXQ) * d; i += NT) {
          const int q0 = (i / d) * MXQ, c = i % d;  // queries q0 .. q0 + MXQ - 1, value column c of the head
          if (q0 >= nq) continue;
          const float* pr = ss + q0 * T;
          // kv and sc are uniform (scalar) bases: an element is one 32-bit offset from them
          const uint32_t vcol = P + h * d + c, scol = vcol >> 5;
          float acc[MXQ];  // rows qi >= nq of ss hold the zero queries' scores: summed, never stored
#pragma unroll
          for (int qi = 0; qi < MXQ; ++qi) acc[qi] = 0.f;
          int t = 0;
          for (; t + MXU <= T; t += MXU) {  // MXU value rows in flight, then the same sums in the same order
            uint32_t v[MXU], E[MXU];
#pragma unroll
            for (int u = 0; u < MXU; ++u) {
              v[u] = kv[(uint32_t)((t + u) * ldk) + vcol];
              E[u] = sc[(uint32_t)((t + u) * lsc) + scol];
            }
#pragma unroll
            for (int u = 0; u < MXU; ++u) {
              const float vf = (float)mx8_dequant1(v[u], E[u]);
#pragma unroll
              for (int qi = 0; qi < MXQ; ++qi) acc[qi] += pr[qi * T + t + u] * vf;
            }
          }
          for (; t < T; ++t) {
            const float vf = (float)mx8_dequant1(kv[(uint32_t)(t * ldk) + vcol], sc[(uint32_t)(t * lsc) + scol]);
#pragma unroll
            for (int qi = 0; qi < MXQ; ++qi) acc[qi] += pr[qi * T + t] * vf;
          }
#pragma unroll
          for (int qi = 0; qi < MXQ; ++qi)
            if (q0 + qi < nq) out[(int64_t)(b * L + l0 + q0 + qi) * ldo + h * d + c] = (bf16)acc[qi];
        }
      }
    } else if (out != nullptr) {
      for (int i = tid; i < nq * d; i += NT) {
        const int qi = i / d, c = i % d;
        const float* pr = ss + qi * T;
        const kv_t* vc = SEG ? kv + (P + h * d + c) : kv + (int64_t)(b * T) * ldkv + P + h * d + c;
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
  align_matrix_block<false>(q, ldq, kv, ldkv, nullptr, 0, kmask, blockIdx.x * QB, blockIdx.y, L, T, P, nh, scale,
                            inv_nh, matrix, T, emit, lde, out, ldo, ss, sq);
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
// MX: kv is the buffer of e4m3 bytes and sc that of its rows' E8M0 scales, row stride lsc (else NULL, 0).
template <bool MX>
__global__ __launch_bounds__(NT) void align_matrix_seg_kernel(const bf16* q, int64_t ldq, const int32_t* qblk,
                                                            const int32_t* pseg, const typename kv_elem<MX>::type* kv,
                                                            int64_t ldkv, const uint8_t* sc, int64_t lsc,
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
  const int64_t row0 = uniform64(seg_row[g]);
  align_matrix_block<true, MX>(q + (int64_t)u * L * ldq, ldq, kv + row0 * ldkv, ldkv, MX ? sc + row0 * lsc : nullptr,
                               (int)lsc, nullptr, l0, 0, L, F, P, nh, scale, inv_nh,
                               matrix == nullptr ? nullptr : matrix + r * L * Tmax, Tmax,
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

namespace {
// the checks and launches shared by ste_align_matrix_seg_fwd (MX = false) and ste_align_matrix_seg_mx8_fwd
// (sc / lsc: the E8M0 scales and their row stride)
template <bool MX>
int align_matrix_seg_launch(const void* q, int64_t ldq, const int32_t* qblk, const int32_t* pseg, const void* kv,
                            int64_t ldkv, const void* sc, int64_t lsc, const int64_t* seg_row, const int32_t* seg_len,
                            int R, int G, int L, int Tmax, int P, int nh, float* matrix, float* emit, int64_t lde,
                            void* out, int64_t ldo, void* stream) {
  if (q == nullptr || qblk == nullptr || pseg == nullptr || kv == nullptr || seg_row == nullptr || seg_len == nullptr ||
      (MX && sc == nullptr))
    return STE_ERR_ARG;
  if (matrix == nullptr && emit == nullptr && out == nullptr) return STE_ERR_ARG;
  if (R <= 0 || G <= 0 || L <= 0 || Tmax <= 0 || nh <= 0 || P <= 0 || P % nh) return STE_ERR_SHAPE;
  const int d = P / nh;
  if (d > DMAX || d % 8 || Tmax > TMAX) return STE_ERR_SHAPE;
  // 16-byte key loads of bf16, 8-byte ones of e4m3
  if (ldq < P || ldkv < 2 * (int64_t)P || ldkv % 8 || (uintptr_t)kv % (MX ? 8 : 16)) return STE_ERR_SHAPE;
  if (MX && (P % 32 || lsc < 2 * (int64_t)P / 32)) return STE_ERR_SHAPE;             // whole 32-column scale blocks
  if ((int64_t)Tmax * ldkv + 2 * (int64_t)P > INT32_MAX) return STE_ERR_SHAPE;      // 32-bit offsets inside a segment
  if (MX && (int64_t)Tmax * lsc + 2 * (int64_t)P / 32 > INT32_MAX) return STE_ERR_SHAPE;
  if ((emit != nullptr && lde < L) || (out != nullptr && ldo < P)) return STE_ERR_SHAPE;
  typedef typename kv_elem<MX>::type kv_t;
  const size_t lds = (size_t)2 * QB * Tmax * sizeof(float);
  if (const int rc = matrix_lds(reinterpret_cast<const void*>(align_matrix_seg_kernel<MX>), lds)) return rc;
  const float scale = 1.0f / sqrtf((float)d), inv_nh = 1.0f / (float)nh;
  for (int r0 = 0; r0 < R; r0 += 65535) {  // the pair rides grid.y
    hipLaunchKernelGGL(align_matrix_seg_kernel<MX>, dim3((L + QB - 1) / QB, min(R - r0, 65535)), dim3(NT), lds,
                       (hipStream_t)stream, (const bf16*)q, ldq, qblk, pseg, (const kv_t*)kv, ldkv, (const uint8_t*)sc,
                       lsc, seg_row, seg_len, r0, G, L, Tmax, P, nh, scale, inv_nh, matrix, emit, lde, (bf16*)out, ldo);
    STE_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

extern "C" int ste_align_matrix_seg_fwd(const void* q, int64_t ldq, const int32_t* qblk, const int32_t* pseg,
                                        const void* kv, int64_t ldkv, const int64_t* seg_row, const int32_t* seg_len,
                                        int R, int G, int L, int Tmax, int P, int nh, float* matrix, float* emit,
                                        int64_t lde, void* out, int64_t ldo, void* stream) {
  return align_matrix_seg_launch<false>(q, ldq, qblk, pseg, kv, ldkv, nullptr, 0, seg_row, seg_len, R, G, L, Tmax, P, nh,
                                        matrix, emit, lde, out, ldo, stream);
}

extern "C" int ste_align_matrix_seg_mx8_fwd(const void* q, int64_t ldq, const int32_t* qblk, const int32_t* pseg,
                                            const void* kv, int64_t ldkv, const void* scales, int64_t lds,
                                            const int64_t* seg_row, const int32_t* seg_len, int R, int G, int L,
                                            int Tmax, int P, int nh, float* matrix, float* emit, int64_t lde, void* out,
                                            int64_t ldo, void* stream) {
  return align_matrix_seg_launch<true>(q, ldq, qblk, pseg, kv, ldkv, scales, lds, seg_row, seg_len, R, G, L, Tmax, P, nh,
                                       matrix, emit, lde, out, ldo, stream);
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
