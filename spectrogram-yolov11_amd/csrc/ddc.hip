// ddc.hip — digital down-converter at the front of a scan: mix -> low-pass -> rational resample in one pass (no reference
// counterpart; spec in DESIGN.md §4, plan in sy11/data/resample.py).
//
//   y[m] = sum_{j < T} taps[phi, j] xm[i0 - j],   i0 = floor((m Q + c) / P),  phi = (m Q + c) mod P,
//   xm[i] = x[i] e^{j 2 pi frac(i dphi / 2^32)},  x = 0 outside the capture
//
//  * A workgroup owns `tile` consecutive outputs.  It stages the input span they read into LDS already mixed (one rotation per input
//    sample, not one per tap; every staged sample then serves ~T P / Q outputs), then each thread accumulates its outputs from LDS
//    against its polyphase row.  The table lives in LDS when the host found room for it, else it is read from global memory (it
//    stays L2-resident: every workgroup reads the same P T floats).
//  * Mixer phase: (uint32) i * dphi in wrapping arithmetic with i the ABSOLUTE sample index, exact for every i; the rotation is
//    evaluated in float64 and rounded once per component (mix() below).  dphi = 0 skips the mixer.
//  * Each output is ONE sequential float32 sum over j = 0 .. T-1 (ascending tap index k = phi + j P), so a value depends on
//    (m, capture) only, never on the tile, the launch shape or the chunk the host cut: chunked scans are bit-identical.
//  * Staging loads pairs of samples with one 16-byte load where base + offset is 16-byte aligned (the span is started one sample
//    early when its first sample is not, uniform per block), else 8-byte loads; samples outside in[] are zeros.
//  * P == Q: no filter, the stage is a pure mixer (one thread per output pair, as iqaug.hip).
#include "common.h"
#include "iqmix.h"                                                        // mix(): shared with extract.hip

namespace {

constexpr int DDC_LDS_BUDGET = 64 * 1024;      // per workgroup: two of them fit the 160 KiB of a CU
constexpr int DDC_MAX_TILE = 1024;

template <bool TAPS_LDS>
__global__ __launch_bounds__(256) void ddc_kernel(int P, int Q, int T, int c, int tile, int span, const float* __restrict__ taps, int64_t n0,
                                                  int n_in, const float2* __restrict__ in, uint32_t dphi, int64_t m0, int M,
                                                  float2* __restrict__ out) {
  extern __shared__ float4 lds_raw[];
  float2* xs = (float2*)lds_raw;                                          // span + 1 staged samples
  float* hs = (float*)(xs + span + 1);                                    // P * T taps (TAPS_LDS)
  const int t0 = blockIdx.x * tile;                                       // first output of the tile, relative to m0
  const int nt = min(tile, M - t0);
  const int64_t q0 = (m0 + t0) * (int64_t)Q + c;                          // m Q + c of the tile's first output (>= 0)
  const int64_t i0_first = q0 / P;
  const int phi_first = (int)(q0 % P);
  // staged samples: absolute [lo, lo + len), lo = the oldest sample the first output reads, moved one down where that makes the
  // first staged sample 16-byte aligned in in[]
  int64_t lo = i0_first - (T - 1);
  const int len_needed = (int)((phi_first + (int64_t)(nt - 1) * Q) / P) + T;
  const bool odd = ((((uintptr_t)in >> 3) + (uint64_t)(lo - n0)) & 1) != 0;
  lo -= odd ? 1 : 0;
  const int len = len_needed + (odd ? 1 : 0);
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
    if (dphi != 0u) {
      const uint32_t ph = (uint32_t)(uint64_t)(lo + s) * dphi;
      a = mix(a, ph);
      b = mix(b, ph + dphi);
    }
    xs[s] = a;
    if (s + 1 < len) xs[s + 1] = b;
  }
  if (TAPS_LDS)
    for (int k = threadIdx.x; k < P * T; k += blockDim.x) hs[k] = taps[k];
  __syncthreads();
  const int base = (int)(i0_first - lo);                                  // LDS slot of the first output's newest sample
  for (int t = threadIdx.x; t < nt; t += blockDim.x) {
    const uint32_t r = (uint32_t)phi_first + (uint32_t)t * (uint32_t)Q;   // < P + tile * Q < 2^23
    const int phi = (int)(r % (uint32_t)P);
    const float2* x = xs + base + (int)(r / (uint32_t)P);                 // x[-j] = xm[i0 - j]
    const float* h = (TAPS_LDS ? hs : taps) + (long)phi * T;
    float re = 0.f, im = 0.f;
    for (int j = 0; j < T; ++j) {
      const float w = h[j];
      const float2 v = x[-j];
      re = fmaf(w, v.x, re);
      im = fmaf(w, v.y, im);
    }
    out[t0 + t] = make_float2(re, im);
  }
}

__global__ __launch_bounds__(256) void mix_kernel(int64_t n0, const float2* __restrict__ in, uint32_t dphi, int64_t off, int M,
                                                  float2* __restrict__ out) {
  const int n = (blockIdx.x * 256 + threadIdx.x) * 2;                     // this thread: outputs n, n + 1
  if (n >= M) return;
  const bool two = n + 1 < M;
  const float2* s = in + off + n;                                         // output m0 + n is sample m0 + n = in[m0 - n0 + n]
  float2 a, b = make_float2(0.f, 0.f);
  if (two && (((uintptr_t)s) & 15) == 0) {
    const float4 v = *(const float4*)s;
    a = make_float2(v.x, v.y);
    b = make_float2(v.z, v.w);
  } else {
    a = s[0];
    if (two) b = s[1];
  }
  if (dphi != 0u) {
    const uint32_t ph = (uint32_t)(uint64_t)(n0 + off + n) * dphi;
    a = mix(a, ph);
    b = mix(b, ph + dphi);
  }
  float2* o = out + n;
  if (two && (((uintptr_t)o) & 15) == 0) {
    *(float4*)o = make_float4(a.x, a.y, b.x, b.y);
  } else {
    o[0] = a;
    if (two) o[1] = b;
  }
}

// staged samples of a tile of `tile` outputs (+ 1 for the alignment sample, + 1 so that the pair store of the last thread fits)
inline long span_of(long tile, int P, int Q, int T) { return ((P - 1) + (tile - 1) * (long)Q) / P + T + 2; }

inline int pick_tile(int P, int Q, int T, long bytes) {
  for (int tile = DDC_MAX_TILE; tile >= 64; tile -= 64)
    if (span_of(tile, P, Q, T) * 8 <= bytes) return tile;
  return 0;
}

}  // namespace

extern "C" int sy11_iq_resample(int32_t P, int32_t Q, int32_t T, int32_t c, const float* taps, int64_t n0, int32_t n_in, const float* in,
                                uint32_t dphi, int64_t m0, int32_t M, float* out, void* stream) {
  SY11_REQUIRE(taps && in && out, "iq_resample: null tap table / input / output");
  SY11_REQUIRE(P > 0 && Q > 0 && T > 0, "iq_resample: P, Q and T must be positive (P=%d Q=%d T=%d)", P, Q, T);
  SY11_REQUIRE(M > 0 && n_in > 0, "iq_resample: M and n_in must be positive and below 2^31 (M=%d n_in=%d)", M, n_in);
  SY11_REQUIRE(P <= 4096 && Q <= 4096 && P <= 64 * Q && Q <= 64 * P, "iq_resample: P/Q = %d/%d: need P, Q <= 4096 and 1/64 <= P/Q <= 64", P, Q);
  SY11_REQUIRE(c >= 0 && (long)c < (long)P * T, "iq_resample: centre tap c=%d outside the table (P*T = %ld)", c, (long)P * T);
  SY11_REQUIRE((long)P * T <= (1L << 20), "iq_resample: table of %ld taps exceeds 2^20", (long)P * T);
  SY11_REQUIRE(n0 >= 0 && m0 >= 0 && m0 < (1LL << 48), "iq_resample: n0 and m0 must be non-negative sample indices (m0 below 2^48)");
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 7) == 0, "iq_resample: in / out must be 8-byte aligned (complex64 samples)");
  if (P == Q) {                                                            // no filter: output m is sample m
    SY11_REQUIRE(m0 >= n0 && m0 - n0 + M <= n_in, "iq_resample: mixer outputs [%ld, %ld) leave in[] = samples [%ld, %ld)", (long)m0,
                 (long)m0 + M, (long)n0, (long)n0 + n_in);
    hipLaunchKernelGGL(mix_kernel, dim3(cdiv(cdiv(M, 2), 256)), dim3(256), 0, (hipStream_t)stream, n0, (const float2*)in, dphi, m0 - n0,
                       M, (float2*)out);
    SY11_LAUNCH_CHECK("iq_resample (mixer)");
    return SY11_OK;
  }
  // the largest tile (a multiple of 64 outputs, <= 1024) whose staged span stays in the budget; a table of up to half the budget
  // sits beside it unless that would leave a tile of under 256 outputs (every workgroup loads the whole table)
  const long table_bytes = (long)P * T * 4;
  bool taps_lds = table_bytes <= DDC_LDS_BUDGET / 2;
  int tile = pick_tile(P, Q, T, DDC_LDS_BUDGET - (taps_lds ? table_bytes : 0));
  if (taps_lds && tile < 256) {
    taps_lds = false;
    tile = pick_tile(P, Q, T, DDC_LDS_BUDGET);
  }
  SY11_REQUIRE(tile > 0, "iq_resample: P/Q = %d/%d with T = %d: a 64-output tile needs %ld bytes of LDS", P, Q, T, span_of(64, P, Q, T) * 8);
  const int span = (int)span_of(tile, P, Q, T) - 1;
  const size_t lds = (size_t)(span + 1) * 8 + (taps_lds ? (size_t)table_bytes : 0);
  const dim3 grid(cdiv(M, tile)), block(tile < 256 ? tile : 256);
  if (taps_lds)
    hipLaunchKernelGGL(ddc_kernel<true>, grid, block, lds, (hipStream_t)stream, P, Q, T, c, tile, span, taps, n0, n_in, (const float2*)in, dphi,
                       m0, M, (float2*)out);
  else
    hipLaunchKernelGGL(ddc_kernel<false>, grid, block, lds, (hipStream_t)stream, P, Q, T, c, tile, span, taps, n0, n_in, (const float2*)in,
                       dphi, m0, M, (float2*)out);
  SY11_LAUNCH_CHECK("iq_resample");
  return SY11_OK;
}
