// fft_lds.h — what measure.hip and cyclo.hip share: the float64 FFT over a 1024-slot LDS image (radix-4 rounds in registers) and the
// bitonic sort behind their medians.  Both files are built with -ffp-contract=on, so the same source gives the same operations in both.
#pragma once
#include "common.h"

namespace sy11_fft {

constexpr int FFT_SLOTS = 1024;                // complex values of the LDS image: 1024 / N frames are transformed together

__device__ __forceinline__ double2 cmul(double2 a, double2 w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// The first round of thread t reads the slots first + m (N / 4), m = 0 .. 3: frame first >> L, position first & (N - 1) in it.
template <int L>
__device__ __forceinline__ int fft_first_slot(int t) {
  constexpr int l2 = L - 2, h2 = 1 << l2;
  return ((t >> l2) << L) | (t & (h2 - 1));
}

// FFT_N, N = 2^L, of the 1024 / N frames of the image, by 256 threads: decimation in frequency in radix-2 order, two stages per round as
// one radix-4 butterfly in registers (one twiddle product per value and round), one barrier per round; an odd L ends with one radix-2
// stage.  In: e[m] = the value of slot fft_first_slot<L>(t) + m (N / 4) (the first round never reads xs).  Out: e[m] = slot 4 t + m,
// and slot q of a frame is bin bitrev_L(q).  tw: e^{-2 pi i m / N}, m < N / 2, in LDS.  Every round but the last passes a barrier
// after its writes of xs; the caller's next writes of xs need one more barrier only if threads may still be in the last round.
template <int L>
__device__ __forceinline__ void fft_rounds(double2 (&e)[4], double2* xs, const double2* tw, int t) {
  constexpr int H = 1 << (L - 1);
#pragma unroll
  for (int s = L - 1; s >= 0; s -= 2) {                                   // s = log2 of the round's first half-size
    if (s >= 1) {
      const int l2 = s - 1, h2 = 1 << l2;
      const int low = t & (h2 - 1), base = ((t >> l2) << (l2 + 2)) | low;
      if (s != L - 1) {
#pragma unroll
        for (int m = 0; m < 4; ++m) e[m] = xs[base + m * h2];
      }
      // one radix-4 butterfly = the two radix-2 stages: every value passes ONE twiddle product per round (-i is a swap)
      const int i3 = (3 * low) << (L - 1 - s);
      const double2 w1 = tw[low << (L - 1 - s)], w2 = tw[low << (L - s)], w3h = tw[i3 & (H - 1)];
      const double2 w3 = i3 >= H ? make_double2(-w3h.x, -w3h.y) : w3h;         // the table holds half a turn
      const double2 a = cadd(e[0], e[2]), b = cadd(e[1], e[3]), c = csub(e[0], e[2]), dm = csub(e[1], e[3]);
      const double2 d = make_double2(dm.y, -dm.x);
      e[0] = cadd(a, b);
      e[1] = cmul(csub(a, b), w2);
      e[2] = cmul(cadd(c, d), w1);
      e[3] = cmul(csub(c, d), w3);
      if (s >= 2) {
#pragma unroll
        for (int m = 0; m < 4; ++m) xs[base + m * h2] = e[m];
        __syncthreads();
      }
    } else {                                                              // odd L: the last stage alone, slots 4 t .. 4 t + 3
#pragma unroll
      for (int m = 0; m < 4; ++m) e[m] = xs[4 * t + m];
      const double2 a0 = cadd(e[0], e[1]), a1 = csub(e[0], e[1]), a2 = cadd(e[2], e[3]), a3 = csub(e[2], e[3]);
      e[0] = a0, e[1] = a1, e[2] = a2, e[3] = a3;
    }
  }
}

// Ascending bitonic sort of srt[0 .. N), N a power of two <= 1024, by 256 threads; pad with +inf.  Ends on a barrier.
__device__ __forceinline__ void bitonic_sort(double* srt, int N, int t) {
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < N; i += 256) {
        const int q = i ^ j;
        if (q > i) {
          const double a = srt[i], c = srt[q];
          if (((i & k) == 0) ? (a > c) : (a < c)) srt[i] = c, srt[q] = a;
        }
      }
      __syncthreads();
    }
}

// The median of the first n values of a sorted srt (mean of the two middle values for an even n); NaN when n = 0.
__device__ __forceinline__ double sorted_median(const double* srt, int n) {
  if (n <= 0) return __longlong_as_double(0x7ff8000000000000LL);
  return (n & 1) ? srt[n / 2] : ((srt[n / 2 - 1] + srt[n / 2]) * 0.5);
}

inline int log2_fft(int n_fft) {
  for (int l = 6; l <= 10; ++l)
    if (n_fft == 1 << l) return l;
  return 0;
}

}  // namespace sy11_fft
