// Rational polyphase resampler (include/ste.h "resample"): native-rate clips -> 16 kHz ahead of
// ste_fbank / ste_w2v_wave_norm.  Replaces the CPU resampling of the reference's data workers
// (ref:training/trainer_unfreeze.py:1927 Audio(sampling_rate=16000), ref:processor.py:82-85
// librosa.resample) with one batched launch.
//
// The filter is a Kaiser-windowed sinc evaluated on the host in double precision, one row of
// K taps per output phase (L phases), rounded once to fp32; the device only multiplies and adds.
//
// Two kernels, chosen by (M, L, K) alone.  Every output sample is summed by exactly one thread as
// one fp32 FMA chain in an order that is the same for every output of a rate pair, whatever the
// tile, the batch row or the row stride: results are bit-identical across batch compositions.
//
// General kernel (resample_kernel).  A workgroup of NT threads (NT a multiple of L, so a thread's
// phase is tid mod L for every output it owns) produces a tile of T = NT·R consecutive outputs of
// one clip; thread tid owns outputs n0 + tid + j·NT, j < R, which share their phase and so their
// coefficient: one table read feeds R FMAs.  The tile's source samples form one contiguous
// window of (T/L)·M + K floats, staged in LDS with the zero extension applied (samples outside
// [0, len) are stored as 0.0f and the padding of the row is never loaded).  Tables of at most
// 4096 floats (24 k, 8 k) are staged in LDS too; the 441:160 family (60-87 k floats) is read
// through the cache, consecutive lanes reading consecutive floats of the tap-major table.
// FMA chain over t = 0 .. K-1.
//
// Integer decimation (resample_dec_kernel, L = 1 and M = 2 or 3: 32 k, 48 k): see below.
#include "common.h"
#include "ste.h"

#include <cmath>

namespace {

constexpr double ZEROS = 64.0;
constexpr double ROLLOFF = 0.9475937167399596;
constexpr double BETA = 14.769656459379492;
constexpr int MAX_L = 1024, MAX_K = 2048;
constexpr int TABLE_LDS_FLOATS = 4096;
constexpr int64_t LDS_BYTES = 64 * 1024;

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// I0 by its power series Σ ((x/2)^2)^k / (k!)^2, summed until a term no longer changes the sum
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

struct Plan {
  int nt, r;         // threads per workgroup, outputs per thread
  int window;        // staged source floats per tile
  bool table_lds;
  int64_t lds_bytes;
};

// the tile of (M, L, K): NT = the multiple of L next to 256, the largest R in {4, 2, 1} whose
// window (and table, when small) fits 64 KB of LDS.  false: no R fits.
bool plan_tile(int M, int L, int K, Plan* p) {
  p->nt = L <= 256 ? L * ((256 + L - 1) / L) : L;
  p->table_lds = (int64_t)L * K <= TABLE_LDS_FLOATS;
  for (int r = 4; r >= 1; r >>= 1) {
    const int64_t window = (int64_t)(p->nt / L) * r * M + K;
    const int64_t bytes = 4 * (window + (p->table_lds ? (int64_t)L * K : 0));
    if (bytes <= LDS_BYTES) {
      p->r = r;
      p->window = (int)window;
      p->lds_bytes = bytes;
      return true;
    }
  }
  return false;
}

// Stage `total` consecutive source samples starting at src0 through store(w, value), w < total:
// samples outside [0, len) are stored as 0.0f and nothing outside the clip is read.  len >= 1.
// The loads are unconditional at indices clamped into the clip, 8 per thread in flight before the
// first store (a bounds-checked load per iteration would wait for each one in turn), and the zero
// extension is a select after them.
template <class Store>
STE_DEV void stage_window(const float* __restrict__ x, int64_t src0, int64_t len, int total, int tid, int nt,
                          Store store) {
  for (int base = 0; base < total; base += 8 * nt) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t m = src0 + base + u * nt + tid;
      v[u] = x[min(max(m, (int64_t)0), len - 1)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int w = base + u * nt + tid;
      const int64_t m = src0 + w;
      if (w < total) store(w, (m >= 0 && m < len) ? v[u] : 0.0f);
    }
  }
}

template <int R, bool TABLE_LDS>
__global__ void resample_kernel(const float* __restrict__ wav, int64_t ld_wav, const int32_t* __restrict__ lengths,
                                int M, int L, int K, int window, const float* __restrict__ table,
                                float* __restrict__ out, int64_t ld_out, int n_out_max,
                                int32_t* __restrict__ out_lengths) {
  extern __shared__ float smem[];
  float* xs = smem;
  const int tid = threadIdx.x, NT = blockDim.x, b = blockIdx.y;
  const int T = NT * R;
  const int64_t n0 = (int64_t)blockIdx.x * T;
  const int64_t len = max(lengths[b], 0);
  const int64_t n_out = (len * L + M - 1) / M;
  if (blockIdx.x == 0 && tid == 0 && out_lengths) out_lengths[b] = (int32_t)n_out;
  float* o = out + (int64_t)b * ld_out;
  if (n0 >= n_out) {  // the whole tile lies past the clip (uniform over the workgroup)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t n = n0 + tid + (int64_t)j * NT;
      if (n < n_out_max) o[n] = 0.0f;
    }
    return;
  }
  const int hw = K >> 1;
  // n0 is a multiple of L, so n0·M/L is exact: the tile's first source sample
  const int64_t src0 = n0 / L * M - hw + 1;
  const float* x = wav + (int64_t)b * ld_wav;
  stage_window(x, src0, len, window, tid, NT, [&](int w, float v) { xs[w] = v; });
  const float* tab = table;
  if (TABLE_LDS) {
    float* ts = smem + window;
    for (int e = tid; e < L * K; e += NT) ts[e] = table[e];
    tab = ts;
  }
  __syncthreads();
  const int i = tid % L;  // phase of every output this thread owns
  const int step = NT / L * M;
  const float* xw = xs + (int)((int64_t)tid * M / L);
  const float* cf = tab + i;
  float acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.0f;
#pragma unroll 4
  for (int t = 0; t < K; ++t) {
    const float c = cf[(int64_t)t * L];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = __fmaf_rn(c, xw[j * step + t], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int64_t n = n0 + tid + (int64_t)j * NT;
    if (n < n_out_max) o[n] = n < n_out ? acc[j] : 0.0f;
  }
}

// Integer decimation (L = 1, M = 2 or 3: 32 k and 48 k -> 16 k).  Every output has the same K
// coefficients, and the general kernel above spends one 4-byte LDS read per FMA, four times what
// the vector ALUs can absorb.  Here the tile's window is staged de-interleaved, plane r holding
// X_r[q] = x[src0 + q·M + r], so that output n reads tap t = M·d + r at X_r[n + d]: a thread that
// owns 4 CONSECUTIVE outputs n .. n+3 walks each plane with aligned 16-byte reads, and every float4
// it loads serves 4 taps x 4 outputs (16 FMAs per ds_read_b128, plus one broadcast float4 of
// coefficients, repacked per plane and zero-padded to a multiple of 4 taps).
// Each output is one FMA chain over the planes r = 0 .. M-1 and, within a plane, d ascending:
// the same order for every output of a rate pair, whatever the tile, the row or the batch.
constexpr int DEC_NT = 256, DEC_T = 4 * DEC_NT;
extern __shared__ f32x4 smem4[];

struct DecPlan {
  int taps4;   // coefficient float4s per plane: ceil(ceil(K/M)/4)
  int64_t lds_bytes;
};

bool dec_plan(int M, int L, int K, DecPlan* p) {
  if (L != 1 || (M != 2 && M != 3)) return false;
  p->taps4 = ((K + M - 1) / M + 3) / 4;
  p->lds_bytes = 4 * (int64_t)M * (DEC_T + 8 * p->taps4);   // M planes of DEC_T + 4·taps4, M·4·taps4 coefficients
  return p->lds_bytes <= LDS_BYTES;
}

template <int M>
__global__ void __launch_bounds__(DEC_NT)
resample_dec_kernel(const float* __restrict__ wav, int64_t ld_wav, const int32_t* __restrict__ lengths, int K,
                    int taps4, const float* __restrict__ table, float* __restrict__ out, int64_t ld_out,
                    int n_out_max, int32_t* __restrict__ out_lengths) {
  const int tid = threadIdx.x, b = blockIdx.y;
  const int CS = 4 * taps4, PS = DEC_T + CS;
  float* planes = reinterpret_cast<float*>(smem4);
  float* coefs = planes + M * PS;
  const int64_t n0 = (int64_t)blockIdx.x * DEC_T;
  const int64_t len = max(lengths[b], 0);
  const int64_t n_out = (len + M - 1) / M;
  if (blockIdx.x == 0 && tid == 0 && out_lengths) out_lengths[b] = (int32_t)n_out;
  float* o = out + (int64_t)b * ld_out;
  const int64_t n_first = n0 + 4 * tid;
  if (n0 >= n_out) {  // the whole tile lies past the clip (uniform over the workgroup)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (n_first + j < n_out_max) o[n_first + j] = 0.0f;
    return;
  }
  const int64_t src0 = n0 * M - (K >> 1) + 1;
  const float* x = wav + (int64_t)b * ld_wav;
  stage_window(x, src0, len, M * PS, tid, DEC_NT, [&](int w, float v) {
    const int q = w / M;
    planes[(w - q * M) * PS + q] = v;
  });
  for (int e = tid; e < M * CS; e += DEC_NT) {
    const int r = e / CS, d = e - r * CS, t = d * M + r;
    coefs[e] = t < K ? table[t] : 0.0f;
  }
  __syncthreads();
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int r = 0; r < M; ++r) {
    const f32x4* X4 = reinterpret_cast<const f32x4*>(planes + r * PS) + tid;
    const f32x4* C4 = reinterpret_cast<const f32x4*>(coefs + r * CS);
    f32x4 lo = X4[0];
#pragma unroll 2
    for (int e = 0; e < taps4; ++e) {
      const f32x4 hi = X4[e + 1];
      const f32x4 c = C4[e];
      const float w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __fmaf_rn(c[s], w[j + s], acc[j]);
      lo = hi;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (n_first + j < n_out_max) o[n_first + j] = n_first + j < n_out ? acc[j] : 0.0f;
}

template <int M>
void launch_dec(const DecPlan& p, dim3 grid, hipStream_t s, const float* wav, int64_t ld_wav, const int32_t* lengths,
                int K, const float* table, float* out, int64_t ld_out, int n_out_max, int32_t* out_lengths) {
  hipLaunchKernelGGL(resample_dec_kernel<M>, grid, dim3(DEC_NT), (size_t)p.lds_bytes, s, wav, ld_wav, lengths, K,
                     p.taps4, table, out, ld_out, n_out_max, out_lengths);
}

template <int R>
void launch(const Plan& p, dim3 grid, hipStream_t s, const float* wav, int64_t ld_wav, const int32_t* lengths, int M,
            int L, int K, const float* table, float* out, int64_t ld_out, int n_out_max, int32_t* out_lengths) {
  if (p.table_lds)
    hipLaunchKernelGGL((resample_kernel<R, true>), grid, dim3(p.nt), (size_t)p.lds_bytes, s, wav, ld_wav, lengths, M,
                       L, K, p.window, table, out, ld_out, n_out_max, out_lengths);
  else
    hipLaunchKernelGGL((resample_kernel<R, false>), grid, dim3(p.nt), (size_t)p.lds_bytes, s, wav, ld_wav, lengths, M,
                       L, K, p.window, table, out, ld_out, n_out_max, out_lengths);
}

}  // namespace

extern "C" int ste_resample_plan(int sr_in, int sr_out, int* M, int* L, int* K) {
  if (sr_in <= 0 || sr_out <= 0) return STE_ERR_ARG;
  const int64_t g = gcd64(sr_in, sr_out);
  const int64_t m = sr_in / g, l = sr_out / g;
  if (l > MAX_L) return STE_ERR_SHAPE;
  const double c = ROLLOFF * (double)(l < m ? l : m);
  const double hw = std::ceil(ZEROS * (double)m / c);
  if (2.0 * hw > (double)MAX_K) return STE_ERR_SHAPE;
  if (M) *M = (int)m;
  if (L) *L = (int)l;
  if (K) *K = 2 * (int)hw;
  return STE_OK;
}

extern "C" int ste_resample_table(int sr_in, int sr_out, float* table, int64_t table_floats) {
  int M, L, K;
  const int rc = ste_resample_plan(sr_in, sr_out, &M, &L, &K);
  if (rc) return rc;
  if (!table || table_floats < (int64_t)L * K) return STE_ERR_ARG;
  const double pi = 3.14159265358979323846;
  const double c = ROLLOFF * (double)(L < M ? L : M);
  const double i0b = bessel_i0(BETA);
  const int hw = K / 2;
  for (int i = 0; i < L; ++i) {
    // output n of phase i: m·L - n·M = (t - hw + 1)·L - (n·M mod L), and n·M mod L = i·M mod L
    const int64_t frac = (int64_t)i * M % L;
    for (int t = 0; t < K; ++t) {
      const int64_t num = (int64_t)(t - hw + 1) * L - frac;
      const double u = (double)num * c / ((double)M * (double)L);
      double h = 0.0;
      if (std::fabs(u) < ZEROS) {
        const double sinc = num == 0 ? 1.0 : std::sin(pi * u) / (pi * u);
        const double r = u / ZEROS;
        h = (c / (double)M) * sinc * bessel_i0(BETA * std::sqrt(1.0 - r * r)) / i0b;
      }
      table[(int64_t)t * L + i] = (float)h;
    }
  }
  return STE_OK;
}

extern "C" int ste_resample_tile(int M, int L, int K) {
  Plan p;
  DecPlan dp;
  if (M <= 0 || L <= 0 || K <= 0 || (K & 1) || L > MAX_L || K > MAX_K || !plan_tile(M, L, K, &p)) return 0;
  return dec_plan(M, L, K, &dp) ? DEC_T : p.nt * p.r;
}

extern "C" int ste_resample(const float* wav, int64_t ld_wav, const int32_t* lengths, int B, int M, int L, int K,
                            const float* table, float* out, int64_t ld_out, int n_out_max, int32_t* out_lengths,
                            void* stream) {
  if (B < 0 || ld_wav < 0 || ld_out < 0 || n_out_max < 0 || M <= 0 || L <= 0 || K <= 0 || (K & 1)) return STE_ERR_ARG;
  if (!table || !wav || !lengths || !out) return STE_ERR_ARG;
  if (L > MAX_L || K > MAX_K || B > 65535 || ld_out < n_out_max) return STE_ERR_SHAPE;
  Plan p;
  if (!plan_tile(M, L, K, &p)) return STE_ERR_SHAPE;
  if (B == 0 || n_out_max == 0) return STE_OK;
  hipStream_t s = (hipStream_t)stream;
  DecPlan dp;
  if (dec_plan(M, L, K, &dp)) {
    const dim3 grid((unsigned)(((int64_t)n_out_max + DEC_T - 1) / DEC_T), (unsigned)B);
    if (M == 2)
      launch_dec<2>(dp, grid, s, wav, ld_wav, lengths, K, table, out, ld_out, n_out_max, out_lengths);
    else
      launch_dec<3>(dp, grid, s, wav, ld_wav, lengths, K, table, out, ld_out, n_out_max, out_lengths);
    STE_CHECK_LAUNCH();
    return STE_OK;
  }
  const int T = p.nt * p.r;
  const dim3 grid((unsigned)(((int64_t)n_out_max + T - 1) / T), (unsigned)B);
  if (p.r == 4)
    launch<4>(p, grid, s, wav, ld_wav, lengths, M, L, K, table, out, ld_out, n_out_max, out_lengths);
  else if (p.r == 2)
    launch<2>(p, grid, s, wav, ld_wav, lengths, M, L, K, table, out, ld_out, n_out_max, out_lengths);
  else
    launch<1>(p, grid, s, wav, ld_wav, lengths, M, L, K, table, out, ld_out, n_out_max, out_lengths);
  STE_CHECK_LAUNCH();
  return STE_OK;
}
