// Cross attention for reranking retrieved transcripts (forward only, no dropout, no probs):
//   ste_xattn_mq_fwd      C single-vector queries per clip against that clip's K/V (text -> audio):
//                         online softmax over key tiles, Q·Kᵀ and P·V on the bf16 MFMA;
//   ste_xattn_gather_fwd  one query per pair against a K/V block chosen per pair (audio -> text):
//                         xattn_fwd_kernel<1> of xattn_fwd.h with gathered addresses;
//   ste_xattn_seg_fwd     (query, segment) pairs against runs of rows of one K/V buffer (a text query
//                         against stored corpus clips): the body of ste_xattn_mq_fwd on tiles of
//                         pairs that share a segment;
//   ste_xattn_seg_mx8_fwd the same on rows stored as MX-fp8 (e4m3 bytes + one E8M0 scale per 32
//                         columns): a fragment is dequantised to the bf16 values the body already
//                         takes, so the arithmetic from there on is that of ste_xattn_seg_fwd.
#include "common.h"
#include "xattn_fwd.h"
#include "../../include/ste.h"

namespace {

constexpr int NT = XATTN_NT;  // 4 waves
constexpr int KT = 32;        // keys per tile: one k-step of the P·V MFMA

// max / sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48), same bits in all four
STE_DEV float xrow_max(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const float y = fmaxf(__builtin_bit_cast(float, (uint32_t)p[0]), __builtin_bit_cast(float, (uint32_t)p[1]));
  const uint32_t w = __builtin_bit_cast(uint32_t, y);
  auto q = __builtin_amdgcn_permlane16_swap(w, w, false, false);
  return fmaxf(__builtin_bit_cast(float, (uint32_t)q[0]), __builtin_bit_cast(float, (uint32_t)q[1]));
}

// The work of one block, shared by the two kernels below: up to 16 query slots against one head slice
// of one run of S key/value rows.  All MFMAs are 16x16x32 bf16 with the
// query on the B side, so a lane's column (lane & 15 = li) is its query slot throughout and the
// softmax state (m, l) of a query lives in the four lanes li, li+16, li+32, li+48:
//   Sᵀ   = K·Qᵀ      A = K rows (key li of a 16-key half, d = 32·ds + 8g + j), B = Q (hi, then lo)
//                    -> lane holds keys 4g + r (r = 0..3) of each half for query li;
//   outᵀ = Vᵀ·Pᵀ     B = the lane's own 8 probabilities (k slot (g, j): key 4g + j of half 0 for
//                    j < 4, of half 1 for j >= 4), A = V read transposed from LDS in that k order
//                    -> lane holds out columns 16·ct + 4g + r of query li.
// Wave w takes key tiles w, w + 4, ... (a function of S alone) and wave 0 folds the waves' (m, l, acc)
// in the order 0, 1, 2, 3, so a slot's result does not depend on C, B, its position or its neighbours.
// DHMAX: head dim rounded up to 32, 64, 128 or 256 (register arrays are sized by it).
// row: the lane's row of q (-1 = empty slot); k / v: row 0 of the run; mask: the run's key mask or
// NULL; o: the lane's out row (NULL = no slot), columns from c0 on.  S >= 1.
// MX: k / v are e4m3 bytes (ldkv in bytes) and ks / vs row 0 of their E8M0 scales (row stride lds
// bytes, one byte per 32 columns of the WHOLE row, so column c0 + d has scale byte (c0 + d) / 32).
// c0 + d is a multiple of 8 at every fragment, so its 8 columns lie in one block: 8 bytes and one
// scale byte become the bf16x8 the bf16 path loads (mx8_dequant8) and nothing after it differs.
template <bool MX>
STE_DEV bf16x8 xattn_load8(const void* base, int64_t ld, const uint8_t* sc, int64_t lds, int64_t r, int col) {
  if constexpr (MX) {
    const uint2 b = *reinterpret_cast<const uint2*>(static_cast<const uint8_t*>(base) + r * ld + col);
    return mx8_dequant8(b, sc[r * lds + (col >> 5)]);
  } else {
    return *reinterpret_cast<const bf16x8*>(static_cast<const bf16*>(base) + r * ld + col);
  }
}

template <int DHMAX, bool MX = false>
STE_DEV void xattn_mq_tile(const float* __restrict__ q, int row, const void* __restrict__ k,
                           const void* __restrict__ v, int64_t ldkv, const uint8_t* __restrict__ ks,
                           const uint8_t* __restrict__ vs, int64_t lds, const int32_t* __restrict__ mask, int S,
                           int P, int dh, int c0, float scale, float* __restrict__ o) {
  constexpr int NDS = DHMAX / 32;                 // d steps of Q·Kᵀ
  constexpr int NCT = DHMAX / 16;                 // 16-column tiles of out
  constexpr int VC = DHMAX < 128 ? DHMAX : 128;   // V columns staged at a time
  constexpr int VLD = VC + 8;                     // LDS row stride (elements) of the V tile
  constexpr int VREG = KT * VLD * 2;              // bytes of a wave's V tile
  constexpr int MREG = NCT * 64 * 16;             // bytes of a wave's accumulators in the merge
  constexpr int LDSB = 4 * VREG > 3 * MREG ? 4 * VREG : 3 * MREG;
  __shared__ __attribute__((aligned(16))) char smem[LDSB];
  __shared__ float sml[3][2][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, g = lane >> 4;
  const int dh16 = (dh + 15) & ~15;

  // the query as bf16 hi + lo (zero for an empty slot and past dh)
  bf16x8 qh[NDS], ql[NDS];
#pragma unroll
  for (int ds = 0; ds < NDS; ++ds) {
    const int d = 32 * ds + 8 * g;
    const bool on = row >= 0 && d < dh;
    const float* qp = q + (int64_t)(on ? row : 0) * P + c0 + (on ? d : 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = on ? qp[j] : 0.f;
      const bf16 h = (bf16)x;
      qh[ds][j] = h;
      ql[ds][j] = (bf16)(x - (float)h);
    }
  }

  float m = -INFINITY, l = 0.f;  // running max (same in the query's 4 lanes), this lane's share of the sum
  f32x4 acc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  char* vt = smem + w * VREG;
  const bf16x8 zero8 = {};
  const int nt = (S + KT - 1) / KT;
  for (int t = w; t < nt; t += 4) {
    const int s0 = t * KT;
    // scores of the tile's two 16-key halves
    float sc[2][4];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int key = min(s0 + 16 * hf + li, S - 1);  // rows past S are masked below
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) {
        const int d = 32 * ds + 8 * g;
        if (32 * ds < dh) {
          const bf16x8 kf = d < dh ? xattn_load8<MX>(k, ldkv, ks, lds, key, c0 + d) : zero8;
          a = mfma16(kf, qh[ds], a);
          a = mfma16(kf, ql[ds], a);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = s0 + 16 * hf + 4 * g + r;
        float x = a[r] * scale;
        if (kk >= S) x = -INFINITY;
        else if (mask && mask[kk] == 0) x = -1e9f;
        sc[hf][r] = x;
      }
    }
    // online softmax: the tile's first key is < S, so the new maximum is finite
    float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),
                     fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
    mx = fmaxf(m, xrow_max(mx));
    const float alpha = __expf(m - mx);
    m = mx;
    bf16x8 pf;
    float ps = 0.f;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(sc[hf][r] - mx);
        ps += p;
        pf[4 * hf + r] = (bf16)p;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = acc[ct] * alpha;
    // outᵀ += Vᵀ·Pᵀ, VC columns of V at a time through the wave's LDS tile
#pragma unroll
    for (int cbi = 0; cbi < DHMAX / VC; ++cbi) {
      const int cb = cbi * VC;
      if (cb < dh) {
        const int ncc = (min(VC, dh16 - cb)) >> 3;  // 8-column chunks per row, zero past dh
        for (int ch = lane; ch < KT * ncc; ch += 64) {
          const int kr = ch / ncc, cc = ch - kr * ncc;
          const int col = cb + 8 * cc;
          bf16x8 x = zero8;
          if (s0 + kr < S && col < dh)
            x = xattn_load8<MX>(v, ldkv, vs, lds, s0 + kr, c0 + col);
          *reinterpret_cast<bf16x8*>(vt + (kr * VLD + 8 * cc) * 2) = x;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ctl = 0; ctl < VC / 16; ++ctl) {
          if (cb + 16 * ctl < dh) {
            const char* a0 = vt + ((4 * g + (li >> 2)) * VLD + 16 * ctl + 4 * (li & 3)) * 2;
            const bf16x8 vf = join_tr(ds_read_tr16(a0), ds_read_tr16(a0 + 16 * VLD * 2));
            acc[cbi * (VC / 16) + ctl] = mfma16(vf, pf, acc[cbi * (VC / 16) + ctl]);
          }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
      }
    }
  }

  // fold the waves in the order 0, 1, 2, 3 (a wave without tiles holds m = -inf, l = 0, acc = 0)
  __syncthreads();
  if (w > 0) {
    char* mr = smem + (w - 1) * MREG;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) *reinterpret_cast<f32x4*>(mr + (ct * 64 + lane) * 16) = acc[ct];
    sml[w - 1][0][lane] = m;
    sml[w - 1][1][lane] = l;
  }
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int ww = 0; ww < 3; ++ww) {
    const float mw = sml[ww][0][lane], lw = sml[ww][1][lane];
    const float mn = fmaxf(m, mw);  // wave 0 owns tile 0: m is finite
    const float a0 = __expf(m - mn), a1 = __expf(mw - mn);
    const char* mr = smem + ww * MREG;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      acc[ct] = acc[ct] * a0 + *reinterpret_cast<const f32x4*>(mr + (ct * 64 + lane) * 16) * a1;
    l = l * a0 + lw * a1;
    m = mn;
  }
  const float inv = 1.f / xrow32_sum(l);
  if (o) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int col = 16 * ct + 4 * g;
      if (col < dh)
        *reinterpret_cast<f32x4*>(o + col) = row >= 0 ? acc[ct] * inv : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// ste_xattn_mq_fwd: one block per (clip b, head hh, tile of 16 query slots of the clip's C)
template <int DHMAX>
__global__ __launch_bounds__(NT) void xattn_mq_kernel(const float* __restrict__ q, const int32_t* __restrict__ qrow,
                                                    const bf16* __restrict__ k, const bf16* __restrict__ v,
                                                    int64_t ldkv, const int32_t* __restrict__ mask, int C, int S,
                                                    int P, int nh, int QT, float scale, float* __restrict__ out) {
  const int bid = blockIdx.x, qt = bid % QT, hh = (bid / QT) % nh, b = bid / (QT * nh);
  const int dh = P / nh, c0 = hh * dh;
  const int c = qt * 16 + (threadIdx.x & 15);  // this lane's query slot
  const int row = c < C ? qrow[(int64_t)b * C + c] : -1;
  xattn_mq_tile<DHMAX>(q, row, k + (int64_t)b * S * ldkv, v + (int64_t)b * S * ldkv, ldkv, nullptr, nullptr, 0,
                       mask ? mask + (int64_t)b * S : nullptr, S, P, dh, c0, scale,
                       c < C ? out + ((int64_t)b * C + c) * P + c0 : nullptr);
}

// ste_xattn_seg_fwd: one block per (tile, head hh).  Tile t is the cnt <= 16 consecutive pairs from
// tile_first[t] on, all of segment pseg[tile_first[t]]: rows seg_row[g] .. seg_row[g] + seg_len[g] - 1
// of k / v.  An empty tile (count 0) or a tile of an empty or negative segment returns before it
// reads a key: its out rows keep the zeros the host wrote.  MX: k / v are e4m3 bytes with the
// scales ks / vs (xattn_mq_tile), else bf16 (ks = vs = NULL); ldkv in elements of either.
template <int DHMAX, bool MX>
__global__ __launch_bounds__(NT) void xattn_seg_kernel(const float* __restrict__ q, const int32_t* __restrict__ qrow,
                                                     const int32_t* __restrict__ pseg, const void* __restrict__ k,
                                                     const void* __restrict__ v, int64_t ldkv,
                                                     const uint8_t* __restrict__ ks,
                                                     const uint8_t* __restrict__ vs, int64_t lds,
                                                     const int64_t* __restrict__ seg_row,
                                                     const int32_t* __restrict__ seg_len,
                                                     const int32_t* __restrict__ tile_first,
                                                     const int32_t* __restrict__ tile_cnt, int R, int G, int P, int nh,
                                                     float scale, float* __restrict__ out) {
  const int t = blockIdx.x / nh, hh = blockIdx.x % nh;
  const int first = tile_first[t], cnt = min(tile_cnt[t], 16);
  if (cnt <= 0 || first < 0 || first > R - cnt) return;
  const int g = pseg[first];
  if (g < 0 || g >= G) return;
  const int S = seg_len[g];
  if (S <= 0) return;
  const int dh = P / nh, c0 = hh * dh;
  const int c = threadIdx.x & 15;
  const int r = first + c;
  const int row = c < cnt ? qrow[r] : -1;
  const int64_t base = seg_row[g] * ldkv * (MX ? 1 : 2), sbase = MX ? seg_row[g] * lds : 0;  // bytes
  xattn_mq_tile<DHMAX, MX>(q, row, static_cast<const char*>(k) + base, static_cast<const char*>(v) + base, ldkv,
                           ks + sbase, vs + sbase, lds, nullptr, S, P, dh, c0, scale,
                           c < cnt ? out + (int64_t)r * P + c0 : nullptr);
}

// the rule of ste_xattn_fwd (heads.hip), without its cap on S
bool xattn_dims_ok(int P, int nh) {
  if (nh <= 0 || P <= 0 || P > 1024 || P % nh) return false;
  const int dh = P / nh;
  return dh % 8 == 0 && dh <= 256;
}

}  // namespace

extern "C" int ste_xattn_mq_fwd(const float* q, const int32_t* qrow, const void* k, const void* v, int64_t ldkv,
                                const int32_t* mask, int B, int C, int S, int P, int nh, float scale, float* out,
                                void* stream) {
  if (B <= 0 || C <= 0 || S <= 0 || !xattn_dims_ok(P, nh) || (ldkv & 7) || ldkv < P ||
      (((uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15))
    return STE_ERR_SHAPE;
  const int QT = (C + 15) / 16, dh = P / nh;
  const int64_t blocks = (int64_t)B * nh * QT;
  if (blocks > 0x7fffffff) return STE_ERR_SHAPE;
#define STE_MQ_LAUNCH(D)                                                                                      \
  hipLaunchKernelGGL(xattn_mq_kernel<D>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, q, qrow, \
                     (const bf16*)k, (const bf16*)v, ldkv, mask, C, S, P, nh, QT, scale, out)
  if (dh <= 32) STE_MQ_LAUNCH(32);
  else if (dh <= 64) STE_MQ_LAUNCH(64);
  else if (dh <= 128) STE_MQ_LAUNCH(128);
  else STE_MQ_LAUNCH(256);
#undef STE_MQ_LAUNCH
  STE_CHECK_LAUNCH();
  return 0;
}

extern "C" int ste_xattn_gather_fwd(const float* q, const int32_t* qrow, const void* k, const void* v, int64_t ldkv,
                                    const int32_t* kvblk, const int32_t* mask, int R, int S, int P, int nh,
                                    float scale, float* out, void* stream) {
  if (R <= 0 || S <= 0 || S > 16384 || !xattn_dims_ok(P, nh) || (ldkv & 7) || ldkv < P ||
      (((uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15))
    return STE_ERR_SHAPE;
  hipLaunchKernelGGL((xattn_fwd_kernel<1, true>), dim3(R, nh), dim3(NT), (size_t)S * sizeof(float),
                     (hipStream_t)stream, q, (const bf16*)k, (const bf16*)v, ldkv, mask, R, S, P, nh, scale, 0.f,
                     (uint64_t)0, (uint64_t)0, (float*)nullptr, out, qrow, kvblk);
  STE_CHECK_LAUNCH();
  return 0;
}

namespace {
// the launch shared by ste_xattn_seg_fwd (MX = false) and ste_xattn_seg_mx8_fwd, arguments checked
template <bool MX>
int xattn_seg_launch(const float* q, const int32_t* qrow, const int32_t* pseg, const void* k, const void* v,
                     int64_t ldkv, const uint8_t* ks, const uint8_t* vs, int64_t lds, const int64_t* seg_row,
                     const int32_t* seg_len, const int32_t* tile_first, const int32_t* tile_cnt, int NTILE, int R,
                     int G, int P, int nh, float scale, float* out, void* stream) {
  const int dh = P / nh;
  const int64_t blocks = (int64_t)NTILE * nh;
  if (blocks > 0x7fffffff) return STE_ERR_SHAPE;
  // rows of pairs that no tile covers (an empty pair, an empty segment) are zeros
  hipError_t e = hipMemsetAsync(out, 0, (size_t)R * P * sizeof(float), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
#define STE_SEG_LAUNCH(D)                                                                                      \
  hipLaunchKernelGGL((xattn_seg_kernel<D, MX>), dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, q, qrow, \
                     pseg, k, v, ldkv, ks, vs, lds, seg_row, seg_len, tile_first, tile_cnt, R, G, P, nh, scale, out)
  if (dh <= 32) STE_SEG_LAUNCH(32);
  else if (dh <= 64) STE_SEG_LAUNCH(64);
  else if (dh <= 128) STE_SEG_LAUNCH(128);
  else STE_SEG_LAUNCH(256);
#undef STE_SEG_LAUNCH
  STE_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int ste_xattn_seg_fwd(const float* q, const int32_t* qrow, const int32_t* pseg, const void* k,
                                 const void* v, int64_t ldkv, const int64_t* seg_row, const int32_t* seg_len,
                                 const int32_t* tile_first, const int32_t* tile_cnt, int NTILE, int R, int G, int P,
                                 int nh, float scale, float* out, void* stream) {
  if (R <= 0 || G <= 0 || NTILE <= 0 || !xattn_dims_ok(P, nh) || (ldkv & 7) || ldkv < P ||
      (((uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15))
    return STE_ERR_SHAPE;
  return xattn_seg_launch<false>(q, qrow, pseg, k, v, ldkv, nullptr, nullptr, 0, seg_row, seg_len, tile_first,
                                 tile_cnt, NTILE, R, G, P, nh, scale, out, stream);
}

extern "C" int ste_xattn_seg_mx8_fwd(const float* q, const int32_t* qrow, const int32_t* pseg, const void* k,
                                     const void* v, int64_t ldkv, const void* ks, const void* vs, int64_t lds,
                                     const int64_t* seg_row, const int32_t* seg_len, const int32_t* tile_first,
                                     const int32_t* tile_cnt, int NTILE, int R, int G, int P, int nh, float scale,
                                     float* out, void* stream) {
  if (R <= 0 || G <= 0 || NTILE <= 0 || !xattn_dims_ok(P, nh) || (P & 31) || (ldkv & 7) || ldkv < P ||
      lds < P / 32 || !ks || !vs || (((uintptr_t)k | (uintptr_t)v) & 7) || ((uintptr_t)out & 15))
    return STE_ERR_SHAPE;
  return xattn_seg_launch<true>(q, qrow, pseg, k, v, ldkv, (const uint8_t*)ks, (const uint8_t*)vs, lds, seg_row,
                                seg_len, tile_first, tile_cnt, NTILE, R, G, P, nh, scale, out, stream);
}
