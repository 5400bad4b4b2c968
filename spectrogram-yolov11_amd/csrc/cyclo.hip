// cyclo.hip — characterise every clip of an extraction: the spectra of |x|^2, x^2 and x^4 (their lines give the symbol rate and the
// carrier at order 2 and 4) and the moments behind the cumulant C42, all clips in one launch (stage 1), then one reduction launch to the
// peak, its neighbours and the median floor of every spectrum (stage 2).  No reference counterpart; spec in DESIGN.md §4, plan in
// sy11/data/characterize.py.
//
//   clip x[0 .. M) in the packed buffer; frame j = clip samples [j H, j H + N), H = N / 2; w = periodic Hann (f32, the table of measure)
//   y_0 = |x|^2, y_1 = x^2, y_2 = x^4, formed in float64 from the f32 samples;   Y_q,j = FFT_N(w y_q,j)
//   stage 1, per item (clip, group g = j / G):   S_q[k] = f32(sum_j |Y_q,j[k]|^2)  (ascending j, sequential)  -> partial[(row 3 + q) N + k]
//                                                 sums of x^2 (complex), |x|^2 and |x|^4 over the item's own samples  -> mom[row 4 ..]
//   stage 2, per (clip, q), float64:             P[k] = (sum_g S_q,g[k]) scale, the first maximum over the search set, P[k -+ 1], the median
//
//  * Stage 1 is psd_kernel's frame loop with three transforms per pass: one workgroup of 256 threads per item, the 1024-slot LDS image
//    of fft_lds.h holds 1024 / N frames, and a thread keeps the four samples it read for the first round in registers, so a frame's
//    samples are read ONCE for the three transforms and the moments.  LDS: 16 KB image + 8 KB powers + 8 KB twiddles = 32 KB.
//  * Float64 throughout and ONE rounding, to the f32 row that is stored, for the reasons given in measure.hip; the float64 VALU runs at
//    half rate and this kernel does three transforms per frame, so it costs about three times measure's stage 1 per frame.
//  * Every sum has one order.  A slot's frames ascending, one after the other.  The moments: frame j owns the clip's samples
//    [j H, j H + H) (the clip's last frame: all N), a thread adds the samples it holds pass after pass, then a xor butterfly over the 64
//    lanes and the four waves in ascending order.  Nothing depends on the item's place in the launch.
//  * Stage 2 is tiny: measure's bitonic sort for the median, the scan for the first maximum by one thread.
#include "common.h"
#include "fft_lds.h"

#include <math.h>

#include <vector>

namespace {

using namespace sy11_fft;

constexpr int CYCLO_GROUP = 16;                // frames per group, as measure's

template <int L>
__global__ __launch_bounds__(256) void cyclo_kernel(const sy11_cyclo_item* __restrict__ items, const float* __restrict__ window,
                                                    const double2* __restrict__ twiddle, const float2* __restrict__ in,
                                                    float* __restrict__ partial, double* __restrict__ mom) {
  constexpr int N = 1 << L, H = N / 2, F = FFT_SLOTS / N, A = N >= 256 ? N / 256 : 1, h2 = N / 4;
  __shared__ double2 xs[FFT_SLOTS];
  __shared__ double pw[FFT_SLOTS];
  __shared__ double2 tw[H];
  const sy11_cyclo_item it = items[blockIdx.x];
  const int t = threadIdx.x;
  for (int i = t; i < H; i += 256) tw[i] = twiddle[i];
  __syncthreads();
  double acc[3][A];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int m = 0; m < A; ++m) acc[q][m] = 0.0;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};                                    // Re x^2, Im x^2, |x|^2, |x|^4 over this thread's own samples
  const int base = fft_first_slot<L>(t), f = base >> L, p = base & (N - 1);
  double w[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) w[m] = (double)window[p + m * h2];
  for (int f0 = 0; f0 < it.nf; f0 += F) {
    const int nfp = min(F, it.nf - f0);                                   // frames of this pass
    const bool live = f < nfp;
    double2 x2[4];                                                        // x^2 of the four samples held: y_1; y_0 and y_2 follow from it
    double a2[4];
    if (live) {
      const float2* src = in + (it.off + ((int64_t)it.j0 + f0 + f) * H + p);
      const bool whole = it.last && f0 + f == it.nf - 1;                  // the clip's last frame owns its second half too
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float2 v = src[m * h2];
        const double a = (double)v.x, b = (double)v.y;
        x2[m] = make_double2(a * a - b * b, 2.0 * (a * b));
        a2[m] = a * a + b * b;
        if (m < 2 || whole) ms[0] += x2[m].x, ms[1] += x2[m].y, ms[2] += a2[m], ms[3] += a2[m] * a2[m];
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double2 e[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        e[m] = make_double2(0.0, 0.0);
        if (live) {
          const double2 y = q == 0 ? make_double2(a2[m], 0.0) : q == 1 ? x2[m] : make_double2(x2[m].x * x2[m].x - x2[m].y * x2[m].y, 2.0 * (x2[m].x * x2[m].y));
          e[m] = make_double2(y.x * w[m], y.y * w[m]);
        }
      }
      fft_rounds<L>(e, xs, tw, t);
      // thread t holds slots 4 t .. 4 t + 3; slot s of a frame is bin bitrev_L(s)
#pragma unroll
      for (int m = 0; m < 4; ++m) pw[4 * t + m] = e[m].x * e[m].x + e[m].y * e[m].y;
      __syncthreads();
#pragma unroll
      for (int m = 0; m < A; ++m) {
        const int s = t + 256 * m;
        if (s < N)
          for (int g = 0; g < nfp; ++g) acc[q][m] += pw[g * N + s];
      }
      // the next transform writes xs after every read of xs above (they precede the barrier), and pw only after at least two more barriers
    }
  }
  __syncthreads();
  float* dst = partial + (int64_t)it.row * 3 * N;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int m = 0; m < A; ++m) {
      const int s = t + 256 * m;
      if (s < N) pw[__brev((unsigned)s) >> (32 - L)] = acc[q][m];
    }
    __syncthreads();
    for (int i = t; i < N; i += 256) dst[q * N + i] = (float)pw[i];        // the one rounding of a row
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double s = ms[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((t & 63) == 0) pw[(t >> 6) * 4 + c] = s;
  }
  __syncthreads();
  if (t < 4) mom[(int64_t)it.row * 4 + t] = ((pw[t] + pw[4 + t]) + pw[8 + t]) + pw[12 + t];
}

// out, per clip 22 float64: for q = 0, 1, 2 at 4 q: P[k]  P[k - 1]  P[k + 1]  median; 12 .. 15: Re m20  Im m20  m21  m42;
// 16 + 2 q: k, 17 + 2 q: the size of the search set (integers, exact in float64)
__global__ __launch_bounds__(256) void cyclo_peaks_kernel(int N, const sy11_cyclo_row* __restrict__ rows, const float* __restrict__ partial,
                                                          const double* __restrict__ mom, double* __restrict__ spectra, double* __restrict__ out) {
#pragma clang fp contract(off)   // every product and sum below is rounded on its own, as numpy does
  __shared__ double P[1024];
  __shared__ double srt[1024];
  const sy11_cyclo_row r = rows[blockIdx.x / 3];
  const int q = blockIdx.x % 3, t = threadIdx.x, H = N / 2;
  const int lo = q == 0 ? r.k_min : -H, hi = H - 1;
  double* sp = spectra + ((int64_t)r.clip * 3 + q) * N;
  for (int i = t; i < N; i += 256) {                                      // i = k + N / 2: signed-bin order
    const int k = i - H, ku = k & (N - 1);
    double s = 0.0;
    for (int g = 0; g < r.n_rows; ++g) s = (s + (double)partial[((r.row0 + g) * 3 + q) * N + ku]);
    const double v = (s * r.scale);
    P[i] = v;
    sp[i] = v;
    srt[i] = k >= lo ? v : __longlong_as_double(0x7ff0000000000000LL);
  }
  __syncthreads();
  bitonic_sort(srt, N, t);                                                // ascending; the bins outside the search set (+inf) go last
  if (t != 0) return;
  const int n = hi - lo + 1;
  int kp = lo;
  double best = P[lo + H];
  for (int k = lo + 1; k <= hi; ++k)
    if (P[k + H] > best) best = P[k + H], kp = k;                         // the first maximum in ascending k
  double* o = out + (int64_t)r.clip * 22;
  o[4 * q] = best, o[4 * q + 1] = P[((kp - 1) & (N - 1)) ^ H], o[4 * q + 2] = P[((kp + 1) & (N - 1)) ^ H], o[4 * q + 3] = sorted_median(srt, n);
  o[16 + 2 * q] = (double)kp, o[17 + 2 * q] = (double)n;
  if (q == 0)
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      for (int g = 0; g < r.n_rows; ++g) s = (s + mom[(r.row0 + g) * 4 + c]);
      o[12 + c] = s;
    }
}

}  // namespace

extern "C" int32_t sy11_iq_cyclo_group(void) { return CYCLO_GROUP; }

extern "C" int sy11_iq_cyclo(int32_t n_fft, int32_t n_item, const sy11_cyclo_item* item_host, const sy11_cyclo_item* item, const float* window,
                             const double* twiddle, int64_t n_in, const float* in, int64_t n_rows, float* partial, double* mom, void* stream) {
  const int L = log2_fft(n_fft);
  SY11_REQUIRE(L != 0, "iq_cyclo: n_fft = %d is not one of 64, 128, 256, 512, 1024", n_fft);
  SY11_REQUIRE(item_host && item && window && twiddle && in && partial && mom, "iq_cyclo: null item table / window / twiddle table / input / partial table / moments");
  SY11_REQUIRE(n_item > 0 && n_in > 0 && n_in < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "iq_cyclo: need items, input and partial rows, each below 2^31 (n_item=%d n_in=%ld n_rows=%ld)", n_item, (long)n_in, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)item | (uintptr_t)mom) & 7) == 0 && ((uintptr_t)twiddle & 15) == 0 && (((uintptr_t)partial | (uintptr_t)window) & 3) == 0,
               "iq_cyclo: in / item table / moments must be 8-byte aligned, the twiddle table 16-byte, partial / window 4-byte");
  const int64_t N = n_fft, H = N / 2;
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {                                      // no item reads outside in[] or writes outside partial / mom
    const sy11_cyclo_item& s = item_host[i];
    SY11_REQUIRE(s.off >= 0 && s.len >= N && s.len <= n_in && s.off <= n_in - s.len, "iq_cyclo: item %d: the clip [%ld, %ld) is shorter than a frame or leaves the %ld packed samples",
                 i, (long)s.off, (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.nf >= 1 && s.nf <= CYCLO_GROUP && s.j0 >= 0 && s.j0 / CYCLO_GROUP == (s.j0 + s.nf - 1) / CYCLO_GROUP,
                 "iq_cyclo: item %d: frames [%d, %ld) are not 1 .. %d frames of one group", i, s.j0, (long)s.j0 + s.nf, CYCLO_GROUP);
    const int64_t J = (s.len - N) / H + 1;
    SY11_REQUIRE((int64_t)s.j0 + s.nf <= J, "iq_cyclo: item %d: frames [%d, %ld) leave the clip's %ld frames", i, s.j0, (long)s.j0 + s.nf, (long)J);
    SY11_REQUIRE((s.last == 1) == ((int64_t)s.j0 + s.nf == J) && (s.last == 0 || s.last == 1),
                 "iq_cyclo: item %d: last = %d, but its frames end at %ld of the clip's %ld", i, s.last, (long)s.j0 + s.nf, (long)J);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "iq_cyclo: item %d writes row %d of a partial table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "iq_cyclo: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
#define SY11_CYCLO_LAUNCH(LL) \
  hipLaunchKernelGGL(cyclo_kernel<LL>, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, window, (const double2*)twiddle, (const float2*)in, partial, mom)
  switch (L) {
    case 6: SY11_CYCLO_LAUNCH(6); break;
    case 7: SY11_CYCLO_LAUNCH(7); break;
    case 8: SY11_CYCLO_LAUNCH(8); break;
    case 9: SY11_CYCLO_LAUNCH(9); break;
    default: SY11_CYCLO_LAUNCH(10); break;
  }
#undef SY11_CYCLO_LAUNCH
  SY11_LAUNCH_CHECK("iq_cyclo");
  return SY11_OK;
}

extern "C" int sy11_cyclo_peaks(int32_t n_fft, int32_t n_row, const sy11_cyclo_row* row_host, const sy11_cyclo_row* row, int64_t n_rows,
                                const float* partial, const double* mom, int32_t n_clip, double* spectra, double* out, void* stream) {
  SY11_REQUIRE(log2_fft(n_fft) != 0, "cyclo_peaks: n_fft = %d is not one of 64, 128, 256, 512, 1024", n_fft);
  SY11_REQUIRE(row_host && row && partial && mom && spectra && out, "cyclo_peaks: null row table / partial table / moments / output");
  SY11_REQUIRE(n_row > 0 && n_row < (1 << 29) && n_rows > 0 && n_clip > 0, "cyclo_peaks: need clips and partial rows (n_row=%d n_rows=%ld n_clip=%d)", n_row,
               (long)n_rows, n_clip);
  SY11_REQUIRE((((uintptr_t)row | (uintptr_t)mom | (uintptr_t)spectra | (uintptr_t)out) & 7) == 0 && ((uintptr_t)partial & 3) == 0,
               "cyclo_peaks: row table / moments / spectra / out must be 8-byte aligned, partial 4-byte aligned");
  const int H = n_fft / 2;
  std::vector<bool> seen((size_t)n_clip, false);
  for (int i = 0; i < n_row; ++i) {
    const sy11_cyclo_row& r = row_host[i];
    SY11_REQUIRE(r.n_rows >= 1 && r.row0 >= 0 && r.row0 + r.n_rows <= n_rows, "cyclo_peaks: clip %d sums rows [%ld, %ld) of a partial table of %ld rows", i,
                 (long)r.row0, (long)r.row0 + r.n_rows, (long)n_rows);
    SY11_REQUIRE(r.clip >= 0 && r.clip < n_clip, "cyclo_peaks: clip %d writes output row %d of %d", i, r.clip, n_clip);
    SY11_REQUIRE(!seen[(size_t)r.clip], "cyclo_peaks: clip %d writes output row %d, which an earlier entry of this call writes", i, r.clip);
    seen[(size_t)r.clip] = true;
    SY11_REQUIRE(r.k_min >= 1 && r.k_min <= H - 1, "cyclo_peaks: clip %d: the search range [%d, %d] is empty or holds DC", i, r.k_min, H - 1);
    SY11_REQUIRE(r.scale > 0.0 && isfinite(r.scale), "cyclo_peaks: clip %d: scale must be positive and finite", i);
  }
  hipLaunchKernelGGL(cyclo_peaks_kernel, dim3(3 * n_row), dim3(256), 0, (hipStream_t)stream, (int)n_fft, row, partial, mom, spectra, out);
  SY11_LAUNCH_CHECK("cyclo_peaks");
  return SY11_OK;
}
