// pfb.hip — polyphase analysis filter bank: all K bands of a capture from ONE read of its samples (no reference counterpart; spec in
// DESIGN.md §4, plan in sy11/data/channelize.py).  Channel k is the DDC of ddc.hip with P = 1, Q = D and a mixer step of -k/K cycles
// per sample:
//
//   y_k[m] = sum_n h[n] x[mD + c - n] e^{-j 2 pi k (mD + c - n) / K}
//          = sum_{r < K} e^{-j 2 pi k r / K} v_m[r],     v_m[r] = sum_{i = r (mod K)} h[mD + c - i] x[i],   x = 0 outside the capture
//
//  * A 256-thread workgroup owns `tile` consecutive time steps for all K channels.  It stages the input span they read
//    ((tile - 1) D + N samples, ddc.hip's 16-byte pair loads, zeros outside in[]) and the N taps into LDS.
//  * Fold: one item per (t, r), lanes along r, so the LDS reads of x (stride +1) and of h (stride -1) are conflict-free.  i is the
//    ABSOLUTE sample index, r = i mod K, so there is no circular shift and no dependence on where a chunk was cut.  Each v_m[r] is
//    ONE sequential float32 sum in ascending tap index n = n_first + j K.
//  * FFT: K lanes of one wave hold v_m[0 .. K-1] (a wave carries 64 / K time steps); log2 K radix-2 decimation-in-frequency stages
//    through lane exchanges, half = K/2, K/4, .., 1: the lower lane of a pair takes a + b, the upper one (a - b) w with
//    w = twiddle[(p mod half) K / (2 half)].  Lane p then holds channel bitrev(p).  The schedule is the same for every tile and
//    launch shape: a value depends on (k, m, capture) only.
//  * Store through LDS (channel-major, rows padded by one) so that lanes run along m: runs of tile * 8 bytes per channel.
#include "common.h"

namespace {

constexpr int PFB_LDS_BUDGET = 64 * 1024;      // as ddc.hip: two workgroups fit the 160 KiB of a CU
constexpr int PFB_MAX_TILE = 1024;
constexpr int PFB_MAX_ITEMS = 4096;            // tile * K: 16 items per thread, 32 KiB of outputs

__global__ __launch_bounds__(256) void pfb_kernel(int K, int logK, int D, int N, int c, int tile, int span, const float* __restrict__ taps,
                                                  const float2* __restrict__ twiddle, int64_t n0, int n_in, const float2* __restrict__ in,
                                                  int64_t m0, int M, int64_t out_stride, float2* __restrict__ out) {
  extern __shared__ float4 lds_raw[];
  float2* xs = (float2*)lds_raw;                                          // span + 1 staged samples
  float2* ys = xs + span + 1;                                             // K rows of tile + 1 outputs
  float2* ws = ys + K * (tile + 1);                                       // K / 2 twiddles (at least one slot)
  float* hs = (float*)(ws + max(K / 2, 1));                               // N taps
  const int t0 = blockIdx.x * tile;                                       // first time step of the tile, relative to m0
  const int nt = min(tile, M - t0);
  const int64_t a_first = (m0 + t0) * (int64_t)D + c;                     // newest sample the tile's first time step reads
  // staged samples: absolute [lo, lo + len), lo = the oldest sample the first time step reads, moved one down where that makes
  // the first staged sample 16-byte aligned in in[]
  int64_t lo = a_first - (N - 1);
  const int odd = (int)((((uintptr_t)in >> 3) + (uint64_t)(lo - n0)) & 1);
  lo -= odd;
  const int len = (nt - 1) * D + N + odd;                                 // <= span
  const int64_t rel0 = lo - n0;                                           // index into in[] of the first staged sample (may be < 0)
  for (int s = threadIdx.x * 2; s < len; s += 2 * blockDim.x) {
    const int64_t r = rel0 + s;
    float2 a = make_float2(0.f, 0.f), b = make_float2(0.f, 0.f);
    if (r >= 0 && r + 1 < n_in) {
      const float4 v = *(const float4*)(in + r);
      a = make_float2(v.x, v.y);
      b = make_float2(v.z, v.w);
    } else {
      if (r >= 0 && r < n_in) a = in[r];
      if (r + 1 >= 0 && r + 1 < n_in) b = in[r + 1];
    }
    xs[s] = a;
    if (s + 1 < len) xs[s + 1] = b;
  }
  for (int k = threadIdx.x; k < N; k += blockDim.x) hs[k] = taps[k];
  for (int k = threadIdx.x; k < K / 2; k += blockDim.x) ws[k] = twiddle[k];
  __syncthreads();
  const int items = tile * K;                                             // a multiple of 64: a wave holds whole time steps
  for (int e = threadIdx.x; e < items; e += blockDim.x) {
    const int t = e >> logK, p = e & (K - 1);
    float re = 0.f, im = 0.f;
    if (t < nt) {                                                         // uniform over the K lanes of a time step
      // newest sample of residue p at or below A = a_first + t D: tap n_first = (A - p) mod K; taps n_first + j K, samples going down
      const int n_first = (int)((a_first + (int64_t)t * D - p) & (int64_t)(K - 1));
      const float2* x = xs + t * D + N - 1 + odd;                         // x[-n] = the sample tap n meets
      for (int n = n_first; n < N; n += K) {
        const float w = hs[n];
        const float2 v = x[-n];
        re = fmaf(w, v.x, re);
        im = fmaf(w, v.y, im);
      }
    }
    for (int half = K >> 1, sh = 0; half >= 1; half >>= 1, ++sh) {
      const float ore = __shfl_xor(re, half), oim = __shfl_xor(im, half);
      if (p & half) {
        const float2 w = ws[(p & (half - 1)) << sh];
        const float dr = ore - re, di = oim - im;
        re = dr * w.x - di * w.y;
        im = dr * w.y + di * w.x;
      } else {
        re += ore;
        im += oim;
      }
    }
    const int k = (int)(__brev((unsigned)p) >> (32 - logK));
    ys[k * (tile + 1) + t] = make_float2(re, im);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < items; e += blockDim.x) {
    const int k = e / tile, t = e - k * tile;
    if (t < nt) out[k * out_stride + t0 + t] = ys[k * (tile + 1) + t];
  }
}

inline long pfb_span(long tile, int D, int N) { return (tile - 1) * D + N + 2; }      // + the alignment sample, + the last pair store

inline long pfb_lds(long tile, int K, int D, int N) {
  return (pfb_span(tile, D, N) + (long)K * (tile + 1) + (K / 2 > 1 ? K / 2 : 1)) * 8 + (long)N * 4;
}

}  // namespace

extern "C" int sy11_iq_channelize(int32_t K, int32_t D, int32_t N, int32_t c, const float* taps, const float* twiddle, int64_t n0,
                                  int32_t n_in, const float* in, int64_t m0, int32_t M, int64_t out_stride, float* out, void* stream) {
  SY11_REQUIRE(taps && twiddle && in && out, "iq_channelize: null taps / twiddle / input / output");
  SY11_REQUIRE(K >= 2 && K <= 64 && (K & (K - 1)) == 0, "iq_channelize: K = %d must be a power of two in [2, 64]", K);
  SY11_REQUIRE(D == K || 2 * D == K, "iq_channelize: D = %d must be K or K / 2 (K = %d)", D, K);
  SY11_REQUIRE(N == 32 * D + 1 && c == 16 * D, "iq_channelize: need N = 32 D + 1 and c = 16 D (N=%d c=%d D=%d)", N, c, D);
  SY11_REQUIRE(M > 0 && n_in > 0, "iq_channelize: M and n_in must be positive and below 2^31 (M=%d n_in=%d)", M, n_in);
  SY11_REQUIRE(n0 >= 0 && m0 >= 0 && m0 < (1LL << 48), "iq_channelize: n0 and m0 must be non-negative indices (m0 below 2^48)");
  SY11_REQUIRE(out_stride >= M, "iq_channelize: out_stride = %ld is below M = %d", (long)out_stride, M);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 7) == 0, "iq_channelize: in / out must be 8-byte aligned (complex64 samples)");
  int logK = 0;
  while ((1 << logK) < K) ++logK;
  // the largest tile (a multiple of 32 time steps, so that tile * K is a whole number of waves) within the LDS budget
  int tile = PFB_MAX_ITEMS / K < PFB_MAX_TILE ? PFB_MAX_ITEMS / K : PFB_MAX_TILE;
  while (tile > 32 && pfb_lds(tile, K, D, N) > PFB_LDS_BUDGET) tile -= 32;
  SY11_REQUIRE(pfb_lds(tile, K, D, N) <= PFB_LDS_BUDGET, "iq_channelize: K = %d, D = %d: a %d-step tile needs %ld bytes of LDS", K, D, tile,
               pfb_lds(tile, K, D, N));
  const int span = (int)pfb_span(tile, D, N) - 1;
  hipLaunchKernelGGL(pfb_kernel, dim3(cdiv(M, tile)), dim3(256), (size_t)pfb_lds(tile, K, D, N), (hipStream_t)stream, K, logK, D, N, c, tile,
                     span, taps, (const float2*)twiddle, n0, n_in, (const float2*)in, m0, M, out_stride, (float2*)out);
  SY11_LAUNCH_CHECK("iq_channelize");
  return SY11_OK;
}
