// measure.hip — measure every detection of a scan: Welch power spectra of all boxes of a staged span in one launch (stage 1), then
// one reduction launch to power, noise median, occupied bandwidth and centroid sums (stage 2).  No reference counterpart; spec in
// DESIGN.md §4, plan in sy11/data/measure.py.
//
//   frame j = capture samples [j H, j H + N), H = N / 2, anchored at sample 0;   X_j = FFT_N(w x_j),   w = periodic Hann (f32, from the host)
//   stage 1, per item (box, group g = j / G):   S[k] = f32(sum_j |X_j[k]|^2)  (ascending j, sequential)      -> partial[row N + k], k = 0 .. N-1
//                                               E[j] = f32((sum over the in-box bins of |X_j[k]|^2) / (N W2)) -> env[env_off + (j - j0)]
//   stage 2, per box, float64:                  P[k] = (sum_g S_g[k]) scale, median of the noise bins, ordered sums over the search span
//
//  * Stage 1: one workgroup of 256 threads per item.  Its LDS image holds 1024 complex values = 1024 / N frames, transformed together:
//    the butterflies of a stage never cross a multiple of N, so the 1024 slots are one index space for every N.  Decimation in frequency
//    in radix-2 order, two stages per round as one radix-4 butterfly in registers (4 values per thread, one twiddle product per value
//    and round), one barrier per round: 5 rounds at N = 1024; an odd log2 N ends with one radix-2 stage.  The input is
//    read in natural order straight from global memory into the first round (coalesced, 8 bytes per lane, so any 8-byte base works),
//    the output stays in bit-reversed order: powers are summed per slot, and only the finished row is put in bin order, through LDS.
//  * Stage 1 computes in float64 and rounds ONCE, to the f32 it stores: w x is exact in float64 (24 + 24 bits), the transform and the
//    sums carry about 1e-16, so a stored value is the f32 nearest to the definition's (but for a rare double rounding) - no f32
//    evaluation of the same sums, in any order, can be closer.  An f32 transform is 1 - 3 ulp off per bin, which a measurement of one
//    frame or one bin shows undiluted; the price is the half-rate f64 VALU and twice the LDS bytes (DESIGN.md §6 has the figures).
//  * Every sum has one order: a slot's frames ascending, one after the other; the in-box bins of a frame lane by lane in ascending
//    slot, then a xor butterfly over the 64 lanes.  Nothing depends on the item's place in the launch or on the chunk.
//  * Stage 2 is tiny: a bitonic sort of at most 1024 doubles in LDS for the median, the ordered sums by one thread.
#include "common.h"
#include "fft_lds.h"

#include <math.h>

#include <vector>

namespace {

using namespace sy11_fft;                      // the FFT rounds and the bitonic sort, shared with cyclo.hip

constexpr int PSD_GROUP = 16;                  // frames per group: at N = 64 one pass of the 1024-slot image is one group
constexpr int PSD_SLOTS = FFT_SLOTS;

template <int L>
__global__ __launch_bounds__(256) void psd_kernel(const sy11_psd_item* __restrict__ items, const float* __restrict__ window,
                                                  const double2* __restrict__ twiddle, int64_t n0, const float2* __restrict__ in,
                                                  float* __restrict__ partial, float* __restrict__ env, double nw2) {
  constexpr int N = 1 << L, H = N / 2, F = PSD_SLOTS / N, A = N >= 256 ? N / 256 : 1;
  __shared__ double2 xs[PSD_SLOTS];
  __shared__ double pw[PSD_SLOTS];
  __shared__ double2 tw[H];
  const sy11_psd_item it = items[blockIdx.x];
  const int t = threadIdx.x;
  for (int i = t; i < H; i += 256) tw[i] = twiddle[i];
  __syncthreads();
  double acc[A];
#pragma unroll
  for (int m = 0; m < A; ++m) acc[m] = 0.0;
  for (int f0 = 0; f0 < it.nf; f0 += F) {
    const int nfp = min(F, it.nf - f0);                                   // frames of this pass
    double2 e[4];
    {                                                                     // the first round's input: from global memory, windowed
      constexpr int h2 = N / 4;
      const int base = fft_first_slot<L>(t), f = base >> L, p = base & (N - 1);
      const float2* src = in + ((it.j0 + f0 + f) * H + p - n0);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        e[m] = make_double2(0.0, 0.0);
        if (f < nfp) {
          const float2 v = src[m * h2];
          const double w = (double)window[p + m * h2];
          e[m] = make_double2((double)v.x * w, (double)v.y * w);                // exact: 24 + 24 bits
        }
      }
    }
    fft_rounds<L>(e, xs, tw, t);
    // after the last round thread t holds slots 4 t .. 4 t + 3; slot q of a frame is bin bitrev_L(q)
#pragma unroll
    for (int m = 0; m < 4; ++m) pw[4 * t + m] = e[m].x * e[m].x + e[m].y * e[m].y;
    __syncthreads();
#pragma unroll
    for (int m = 0; m < A; ++m) {
      const int p = t + 256 * m;
      if (p < N)
        for (int f = 0; f < nfp; ++f) acc[m] += pw[f * N + p];
    }
    if (env) {
      const int lane = t & 63;
      for (int f = t >> 6; f < nfp; f += 4) {                              // a wave per frame
        double s = 0.0;
        for (int p = lane; p < N; p += 64) {
          const int ku = (int)(__brev((unsigned)p) >> (32 - L)), k = ku >= H ? ku - N : ku;
          if (k >= it.k_lo && k <= it.k_hi) s += pw[f * N + p];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) env[it.env_off + f0 + f] = (float)(s / nw2);
      }
    }
    // the next pass writes xs after these reads of xs are long done, and pw only after at least two more barriers
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < A; ++m) {
    const int p = t + 256 * m;
    if (p < N) pw[__brev((unsigned)p) >> (32 - L)] = acc[m];
  }
  __syncthreads();
  float* dst = partial + (int64_t)it.row * N;
  for (int i = t; i < N; i += 256) dst[i] = (float)pw[i];                   // the one rounding of a row
}

__global__ __launch_bounds__(256) void psd_measure_kernel(int N, const sy11_psd_box* __restrict__ boxes, double frac_lo, double frac_hi,
                                                          const float* __restrict__ partial, double* __restrict__ psd,
                                                          double* __restrict__ out_f, int32_t* __restrict__ out_i) {
#pragma clang fp contract(off)   // every product and sum below is rounded on its own, as numpy does (the build contracts a * b + c otherwise)
  __shared__ double P[1024];
  __shared__ double srt[1024];
  __shared__ int n_noise_s;
  const sy11_psd_box b = boxes[blockIdx.x];
  const int t = threadIdx.x, H = N / 2;
  if (t == 0) n_noise_s = 0;
  __syncthreads();
  for (int i = t; i < N; i += 256) {                                      // i = k + N / 2: signed-bin order
    const int k = i - H, ku = k & (N - 1);
    double s = 0.0;
    for (int g = 0; g < b.n_rows; ++g) s = (s + (double)partial[(b.row0 + g) * N + ku]);
    const double p = (s * b.scale);
    P[i] = p;
    psd[(int64_t)blockIdx.x * N + i] = p;
    const bool noise = k >= -b.noise_l && k <= b.noise_l - 1 && (k < b.s_lo || k > b.s_hi);
    srt[i] = noise ? p : __longlong_as_double(0x7ff0000000000000LL);
    if (noise) atomicAdd(&n_noise_s, 1);
  }
  __syncthreads();
  bitonic_sort(srt, N, t);                                                // ascending; the non-noise slots (+inf) go last
  if (t != 0) return;
  const int n_noise = n_noise_s;
  const double med = sorted_median(srt, n_noise);
  const double nd = (med * b.corr);
  double p_in = 0.0;
  for (int k = b.k_lo; k <= b.k_hi; ++k) p_in = (p_in + P[k + H]);
  double sum_c = 0.0, sum_kc = 0.0;
  for (int k = b.s_lo; k <= b.s_hi; ++k) {
    const double d = P[k + H] - nd, c = n_noise > 0 ? (d > 0.0 ? d : 0.0) : P[k + H];
    sum_c = (sum_c + c);
    sum_kc = sum_kc + (double)k * c;                                   // two roundings: contraction is off in this function
  }
  const double thr_lo = (frac_lo * sum_c), thr_hi = (frac_hi * sum_c);
  int k_dn = b.s_hi, k_up = b.s_hi;
  bool have_dn = false, have_up = false;
  double run = 0.0;
  for (int k = b.s_lo; k <= b.s_hi; ++k) {
    const double d = P[k + H] - nd, c = n_noise > 0 ? (d > 0.0 ? d : 0.0) : P[k + H];
    run = (run + c);
    if (!have_dn && run >= thr_lo) k_dn = k, have_dn = true;
    if (!have_up && run >= thr_hi) k_up = k, have_up = true;
  }
  double* of = out_f + (int64_t)blockIdx.x * 4;
  int32_t* oi = out_i + (int64_t)blockIdx.x * 4;
  of[0] = p_in, of[1] = med, of[2] = sum_c, of[3] = sum_kc;
  oi[0] = k_dn, oi[1] = k_up, oi[2] = b.k_hi - b.k_lo + 1, oi[3] = n_noise;
}

}  // namespace

extern "C" int32_t sy11_iq_psd_group(void) { return PSD_GROUP; }

extern "C" int sy11_iq_psd(int32_t n_fft, int32_t n_item, const sy11_psd_item* item_host, const sy11_psd_item* item, const float* window,
                           const double* twiddle, double nw2, int64_t n_total, int64_t n0, int32_t n_in, const float* in, int64_t n_rows,
                           float* partial, int64_t env_len, float* env, void* stream) {
  const int L = log2_fft(n_fft);
  SY11_REQUIRE(L != 0, "iq_psd: n_fft = %d is not one of 64, 128, 256, 512, 1024", n_fft);
  SY11_REQUIRE(item_host && item && window && twiddle && in && partial, "iq_psd: null item table / window / twiddle table / input / partial table");
  SY11_REQUIRE(n_item > 0 && n_in > 0 && n_rows > 0 && n_rows < (1LL << 31), "iq_psd: need items, input and partial rows (n_item=%d n_in=%d n_rows=%ld)",
               n_item, n_in, (long)n_rows);
  SY11_REQUIRE(env_len >= 0 && (env != nullptr) == (env_len > 0), "iq_psd: env and env_len go together (env_len=%ld)", (long)env_len);
  SY11_REQUIRE(nw2 > 0.0 && isfinite(nw2), "iq_psd: nw2 = N sum w^2 must be positive and finite");
  SY11_REQUIRE(n0 >= 0 && n_total > 0 && n0 + n_in <= n_total && n_total < (1LL << 48),
               "iq_psd: in[] = samples [%ld, %ld) must lie inside the capture's %ld (below 2^48)", (long)n0, (long)n0 + n_in, (long)n_total);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)item) & 7) == 0 && ((uintptr_t)twiddle & 15) == 0 && (((uintptr_t)partial | (uintptr_t)env | (uintptr_t)window) & 3) == 0,
               "iq_psd: in / item table must be 8-byte aligned, the twiddle table 16-byte, partial / env / window 4-byte");
  const int64_t N = n_fft, H = N / 2;
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {                                      // no item reads outside in[] or writes outside partial / env
    const sy11_psd_item& s = item_host[i];
    SY11_REQUIRE(s.nf >= 1 && s.nf <= PSD_GROUP && s.j0 >= 0 && s.j0 < (1LL << 48) && s.j0 / PSD_GROUP == (s.j0 + s.nf - 1) / PSD_GROUP,
                 "iq_psd: item %d: frames [%ld, %ld) are not 1 .. %d frames of one group", i, (long)s.j0, (long)s.j0 + s.nf, PSD_GROUP);
    const int64_t a = s.j0 * H, b = (s.j0 + s.nf - 1) * H + N;
    SY11_REQUIRE(b <= n_total, "iq_psd: item %d: frames [%ld, %ld) leave the capture's %ld samples", i, (long)s.j0, (long)s.j0 + s.nf, (long)n_total);
    SY11_REQUIRE(a >= n0 && b <= n0 + n_in, "iq_psd: item %d reads samples [%ld, %ld); in[] holds [%ld, %ld)", i, (long)a, (long)b, (long)n0,
                 (long)n0 + n_in);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "iq_psd: item %d writes row %d of a partial table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "iq_psd: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
    SY11_REQUIRE(s.k_lo >= -H && s.k_lo <= s.k_hi && s.k_hi < H, "iq_psd: item %d: bins [%d, %d] are not in [%ld, %ld)", i, s.k_lo, s.k_hi, (long)-H,
                 (long)H);
    if (env)
      SY11_REQUIRE(s.env_off >= 0 && s.env_off + s.nf <= env_len, "iq_psd: item %d writes [%ld, %ld) of an envelope of %ld values", i,
                   (long)s.env_off, (long)s.env_off + s.nf, (long)env_len);
  }
#define SY11_PSD_LAUNCH(LL)                                                                                                             \
  hipLaunchKernelGGL(psd_kernel<LL>, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, window, (const double2*)twiddle, n0, \
                     (const float2*)in, partial, env, nw2)
  switch (L) {
    case 6: SY11_PSD_LAUNCH(6); break;
    case 7: SY11_PSD_LAUNCH(7); break;
    case 8: SY11_PSD_LAUNCH(8); break;
    case 9: SY11_PSD_LAUNCH(9); break;
    default: SY11_PSD_LAUNCH(10); break;
  }
#undef SY11_PSD_LAUNCH
  SY11_LAUNCH_CHECK("iq_psd");
  return SY11_OK;
}

extern "C" int sy11_psd_measure(int32_t n_fft, int32_t n_box, const sy11_psd_box* box_host, const sy11_psd_box* box, double frac_lo,
                                double frac_hi, int64_t n_rows, const float* partial, double* psd, double* out_f, int32_t* out_i,
                                void* stream) {
  SY11_REQUIRE(log2_fft(n_fft) != 0, "psd_measure: n_fft = %d is not one of 64, 128, 256, 512, 1024", n_fft);
  SY11_REQUIRE(box_host && box && partial && psd && out_f && out_i, "psd_measure: null box table / partial table / output");
  SY11_REQUIRE(n_box > 0 && n_rows > 0, "psd_measure: need boxes and partial rows (n_box=%d n_rows=%ld)", n_box, (long)n_rows);
  SY11_REQUIRE(frac_lo >= 0.0 && frac_lo <= frac_hi && frac_hi <= 1.0, "psd_measure: need 0 <= frac_lo <= frac_hi <= 1, got %g / %g", frac_lo, frac_hi);
  SY11_REQUIRE((((uintptr_t)box | (uintptr_t)psd | (uintptr_t)out_f) & 7) == 0 && (((uintptr_t)partial | (uintptr_t)out_i) & 3) == 0,
               "psd_measure: box table / psd / out_f must be 8-byte aligned, partial / out_i 4-byte aligned");
  const int H = n_fft / 2;
  for (int i = 0; i < n_box; ++i) {
    const sy11_psd_box& b = box_host[i];
    SY11_REQUIRE(b.n_rows >= 1 && b.row0 >= 0 && b.row0 + b.n_rows <= n_rows, "psd_measure: box %d sums rows [%ld, %ld) of a partial table of %ld rows", i,
                 (long)b.row0, (long)b.row0 + b.n_rows, (long)n_rows);
    SY11_REQUIRE(-H <= b.s_lo && b.s_lo <= b.k_lo && b.k_lo <= b.k_hi && b.k_hi <= b.s_hi && b.s_hi < H,
                 "psd_measure: box %d: need -N/2 <= s_lo <= k_lo <= k_hi <= s_hi < N/2, got %d %d %d %d", i, b.s_lo, b.k_lo, b.k_hi, b.s_hi);
    SY11_REQUIRE(b.noise_l >= 0 && b.noise_l <= H, "psd_measure: box %d: noise_l = %d is not in [0, %d]", i, b.noise_l, H);
    SY11_REQUIRE(b.scale > 0.0 && isfinite(b.scale) && b.corr > 0.0 && isfinite(b.corr), "psd_measure: box %d: scale and corr must be positive and finite", i);
  }
  hipLaunchKernelGGL(psd_measure_kernel, dim3(n_box), dim3(256), 0, (hipStream_t)stream, (int)n_fft, box, frac_lo, frac_hi, partial, psd, out_f, out_i);
  SY11_LAUNCH_CHECK("psd_measure");
  return SY11_OK;
}
