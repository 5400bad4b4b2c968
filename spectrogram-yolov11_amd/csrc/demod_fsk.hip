// demod_fsk.hip — demodulate every frequency-keyed clip (2-FSK / GFSK / GMSK) of an extraction, feed-forward: discriminator + post-detection
// filter + timing partials (launch 1), cubic interpolation at the fitted symbol instants + the per-block level sums (launch 2), the symbols
// scaled to +-1 + decisions + the per-block error sums (launch 3), each over all clips at once.  The two fits between the launches (the timing
// line of demodulate.py, the two level means) are the host's, in float64 numpy.  No reference counterpart; spec in DESIGN.md §4, plan in
// sy11/data/demodulate_fsk.py.
//
//   launch 1, per (clip, tile of TILE usable samples):  f[n] = arg(x[n] conj(x[n - 1]) e^{-2 pi i wc 2^-64}) / 2 pi,  y[n] = f32(sum_k f[n - k] h[k])
//                                                       row = sum y^2 w, sum y w, sum w (Re, Im each), sum y, sum y^2,  w = e^{-2 pi i (n ws mod 2^64) 2^-64}   (f64)
//   launch 2, per (clip, block of symbols):             s_i = f32(cubic Lagrange of y[k - 1 .. k + 2] at mu), t_i = t0 + i step = (k + mu) 2^32
//                                                       row = #(s_i >= m), sum s_i over s_i >= m, sum s_i over s_i < m, sum s_i^2                          (f64)
//   launch 3, per (clip, block of symbols):             r_i = f32((s_i - f0) / dev) stored as (r_i, 0),  d_i = (r_i < 0),  row = sum r^2, sum |r|, n        (f64)
//
//  * Float64 throughout and ONE rounding, to the f32 value that is stored (y, s, r), as demod.hip does and for its reason.
//  * Launch 1 is the hot path and has the shape of demod_filter_kernel: one workgroup of ONE wave per item.  The discriminator (two loads, a
//    complex product, a float64 atan2) is evaluated ONCE per sample of the tile and its 2 hw halo, while they are written to LDS as float64
//    (1040 samples) next to the taps (520 float64): 12.5 KB, so 12 workgroups fit the LDS of a CU.  A thread owns 8 ADJACENT outputs and walks the
//    taps 8 at a time with a 16-sample register window: per 8 taps it reads 8 new samples and 8 broadcast taps from LDS for 64 float64 FMAs
//    (the samples are real: half the FMAs of the PSK filter).  Sample i lies at [i % 8][i / 8], so that the 64 lanes, whose windows are 8
//    samples apart, read 64 consecutive float64 with every read (no bank conflict).
//  * The usable span of a clip is [hw + 1, len - hw): f[n] needs x[n - 1], so the first tile's halo starts at sample 1.  The first tile also
//    writes the zeros of y[0, hw + 1), the last tile those of y[len - hw, len): the items of a clip write every y[n] of the clip once.
//  * Every sum has one order: a thread's taps ascending, its 8 outputs ascending, a xor butterfly over the 64 lanes (and, in launches 2
//    and 3, the four waves ascending).  Nothing depends on the item's place in the launch.  No atomics.
#include "common.h"

#include <math.h>

#include <vector>

namespace {

constexpr int FSK_TILE = 512;                   // usable samples per item of launch 1: the value of sy11_iq_demod_tile
constexpr int FSK_TAPS = 513;                   // 2 * 16 * 16 + 1
constexpr int FSK_TAPS_LDS = 520;               // the taps padded with zeros to a multiple of 8
constexpr int FSK_SPAN = FSK_TILE + FSK_TAPS_LDS + 8;         // samples in LDS: the last window read ends at sample 504 + 512 + 15
constexpr int FSK_BLOCK = 256;                  // symbols per block at most: one thread each

// e^{-2 pi i ph 2^-64} in float64
__device__ __forceinline__ void fsk_rot64(uint64_t ph, double& c, double& s) {
  double sn, cs;
  sincospi((double)(int64_t)ph * 0x1p-63, &sn, &cs);                      // half turns in [-1, 1)
  c = cs, s = -sn;
}

__device__ __forceinline__ double fsk_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// acc[j] += w[j + m] h[m] for the 8 outputs j and the 8 taps m of one step, w = lo ++ hi; taps ascending, fused multiply-adds
__device__ __forceinline__ void fsk_mac(double (&acc)[8], const double (&lo)[8], const double (&hi)[8], const double* __restrict__ tp) {
  double h[8];
#pragma unroll
  for (int m = 0; m < 8; m += 2) {
    const double2 v = *(const double2*)(tp + m);
    h[m] = v.x, h[m + 1] = v.y;
  }
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fma(j + m < 8 ? lo[j + m] : hi[j + m - 8], h[m], acc[j]);
}

__global__ __launch_bounds__(64) void fsk_filter_kernel(const sy11_fsk_item* __restrict__ items, const float* __restrict__ taps,
                                                        const float2* __restrict__ in, float* __restrict__ y, double* __restrict__ rows) {
  __shared__ double sm[8][FSK_SPAN / 8];                                  // f of sample i of the item's span at sm[i % 8][i / 8]
  __shared__ __attribute__((aligned(16))) double tp[FSK_TAPS_LDS];
  const sy11_fsk_item it = items[blockIdx.x];
  const int t = threadIdx.x, hw = it.hw, cnt = it.cnt, nblk = (it.n_taps + 7) >> 3;
  for (int i = t; i < FSK_TAPS_LDS; i += 64) tp[i] = i < it.n_taps ? (double)taps[it.tap_off + (it.n_taps - 1 - i)] : 0.0;
  if (it.first)                                                           // y = 0 outside the usable span [hw + 1, len - hw)
    for (int i = t; i <= hw; i += 64) y[it.off + i] = 0.0f;
  if (it.last)
    for (int i = t; i < hw; i += 64) y[it.off + it.len - hw + i] = 0.0f;
  double rc, rs;                                                          // the carrier's turn per sample
  fsk_rot64(it.wc, rc, rs);
  const int64_t base = it.n0 - hw;                                        // >= 1: the span's first sample has a sample before it
  for (int i = t; i < FSK_SPAN; i += 64) {
    const int64_t n = base + i;
    double f = 0.0;
    if (i < cnt + 2 * hw && n >= 1 && n < it.len) {
      const float2 a = in[it.off + n], b = in[it.off + n - 1];
      const double ax = (double)a.x, ay = (double)a.y, bx = (double)b.x, by = (double)b.y;
      const double zr = ax * bx + ay * by, zi = ay * bx - ax * by;        // x[n] conj(x[n - 1])
      f = atan2(zr * rs + zi * rc, zr * rc - zi * rs) * 0.15915494309189533577;      // cycles per sample
    }
    sm[i & 7][i >> 3] = f;
  }
  __syncthreads();
  // the window is lo ++ hi; the two halves change roles from one step to the next, so that no register is moved
  double acc[8], wa[8], wb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0, wa[j] = sm[j][t];              // samples 8 t + j
  int blk = 0;
  for (; blk + 1 < nblk; blk += 2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) wb[j] = sm[j][t + blk + 1];                // samples 8 t + 8 blk + 8 + j: the lanes read consecutive float64
    fsk_mac(acc, wa, wb, &tp[8 * blk]);
#pragma unroll
    for (int j = 0; j < 8; ++j) wa[j] = sm[j][t + blk + 2];
    fsk_mac(acc, wb, wa, &tp[8 * blk + 8]);
  }
  if (blk < nblk) {
#pragma unroll
    for (int j = 0; j < 8; ++j) wb[j] = sm[j][t + blk + 1];
    fsk_mac(acc, wa, wb, &tp[8 * blk]);
  }
  float ar[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ar[j] = (float)acc[j];                       // the one rounding of y
  float* dst = y + (it.off + it.n0 + 8 * t);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (8 * t + j < cnt) dst[j] = ar[j];
  // the row of the usable samples, from the float32 values just stored
  {
#pragma clang fp contract(off)
    double er, ei, qr, qi, S[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = 0.0;
    fsk_rot64((uint64_t)(it.n0 + 8 * t) * it.ws, er, ei);
    fsk_rot64(it.ws, qr, qi);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (8 * t + j < cnt) {
        const double a = (double)ar[j];
        const double p = a * a;
        S[0] += p * er, S[1] += p * ei, S[2] += a * er, S[3] += a * ei, S[4] += er, S[5] += ei, S[6] += a, S[7] += p;
      }
      const double nr = er * qr - ei * qi, ni = er * qi + ei * qr;
      er = nr, ei = ni;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = fsk_wave_sum(S[k]);
    if (t == 0) {
      double* o = rows + (int64_t)it.row * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = S[k];
    }
  }
}

// the four waves' sums in ascending order -> thread 0
__device__ __forceinline__ double fsk_block_sum(double v, double* sh, int t) {
  v = fsk_wave_sum(v);
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void fsk_symbols_kernel(const sy11_fsk_block* __restrict__ items, const float* __restrict__ y, float* __restrict__ sym,
                                                          double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  const sy11_fsk_block it = items[blockIdx.x];
  const int t = threadIdx.x;
  double nh = 0.0, sh_hi = 0.0, sh_lo = 0.0, p = 0.0;
  if (t < it.n) {
    const int64_t ti = it.t0 + (int64_t)t * it.step;
    const int64_t k = ti >> 32;
    const double mu = (double)(uint32_t)(((uint64_t)ti & 0xffffffffull) >> 8) * 0x1p-24;      // the top 24 bits of the fraction
    const float* src = y + (it.off + k - 1);
    const double y0 = (double)src[0], y1 = (double)src[1], y2 = (double)src[2], y3 = (double)src[3];
    const double a = mu + 1.0, b = mu - 1.0, c = mu - 2.0;
    const double c0 = ((-mu * b) * c) / 6.0, c1 = ((a * b) * c) / 2.0, c2 = ((-a * mu) * c) / 2.0, c3 = ((a * mu) * b) / 6.0;
    const float s = (float)(((c0 * y0 + c1 * y1) + c2 * y2) + c3 * y3);   // the one rounding of s
    sym[it.sym_off + t] = s;
    const double u = (double)s;
    if (u >= it.m) nh = 1.0, sh_hi = u;
    else sh_lo = u;
    p = u * u;
  }
  nh = fsk_block_sum(nh, sh, t), sh_hi = fsk_block_sum(sh_hi, sh, t), sh_lo = fsk_block_sum(sh_lo, sh, t), p = fsk_block_sum(p, sh, t);
  if (t == 0) {
    double* o = rows + (int64_t)it.row * 4;
    o[0] = nh, o[1] = sh_hi, o[2] = sh_lo, o[3] = p;
  }
}

__global__ __launch_bounds__(256) void fsk_decide_kernel(const sy11_fsk_dec* __restrict__ items, const float* __restrict__ sym, float2* __restrict__ r,
                                                         uint8_t* __restrict__ d, double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  const sy11_fsk_dec it = items[blockIdx.x];
  const int t = threadIdx.x;
  double e2 = 0.0, ea = 0.0;
  if (t < it.n) {
    const float v = (float)(((double)sym[it.sym_off + t] - it.f0) / it.dev);                  // the one rounding of r
    r[it.sym_off + t] = make_float2(v, 0.0f);
    d[it.sym_off + t] = (uint8_t)(v < 0.0f);
    const double u = (double)v;
    e2 = u * u, ea = fabs(u);
  }
  e2 = fsk_block_sum(e2, sh, t), ea = fsk_block_sum(ea, sh, t);
  if (t == 0) {
    double* o = rows + (int64_t)it.row * 3;
    o[0] = e2, o[1] = ea, o[2] = (double)it.n;
  }
}

}  // namespace

extern "C" int sy11_iq_fsk_filter(int32_t n_item, const sy11_fsk_item* item_host, const sy11_fsk_item* item, int64_t n_tap, const float* taps,
                                  int64_t n_in, const float* in, float* y, int64_t n_rows, double* rows, void* stream) {
  SY11_REQUIRE(item_host && item && taps && in && y && rows, "iq_fsk_filter: null item table / taps / input / output / row table");
  SY11_REQUIRE(n_item > 0 && n_tap > 0 && n_tap < (1LL << 31) && n_in > 0 && n_in < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "iq_fsk_filter: need items, taps, input and rows, each below 2^31 (n_item=%d n_tap=%ld n_in=%ld n_rows=%ld)", n_item, (long)n_tap,
               (long)n_in, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)item | (uintptr_t)rows) & 7) == 0 && (((uintptr_t)taps | (uintptr_t)y) & 3) == 0 && (const void*)in != (const void*)y,
               "iq_fsk_filter: in / item table / rows must be 8-byte aligned, y and the taps 4-byte, and y may not be in");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {                                      // no item reads outside in[] / taps[] or writes outside y / rows
    const sy11_fsk_item& s = item_host[i];
    SY11_REQUIRE(s.off >= 0 && s.len >= 1 && s.len <= n_in && s.off <= n_in - s.len, "iq_fsk_filter: item %d: the clip [%ld, %ld) leaves the %ld packed samples", i,
                 (long)s.off, (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.hw >= 1 && s.n_taps == 2 * s.hw + 1 && s.n_taps <= FSK_TAPS, "iq_fsk_filter: item %d: %d taps for a half width of %d (odd, 2 hw + 1, at most %d)", i,
                 s.n_taps, s.hw, FSK_TAPS);
    SY11_REQUIRE(s.tap_off >= 0 && s.tap_off <= n_tap - s.n_taps, "iq_fsk_filter: item %d: taps [%ld, %ld) leave the %ld packed taps", i, (long)s.tap_off,
                 (long)s.tap_off + s.n_taps, (long)n_tap);
    SY11_REQUIRE(s.n0 >= s.hw + 1 && (s.n0 - s.hw - 1) % FSK_TILE == 0 && s.cnt >= 1 && s.cnt <= FSK_TILE && s.n0 <= s.len - s.hw - s.cnt,
                 "iq_fsk_filter: item %d: samples [%ld, %ld) are not a tile of the usable span [%d, %ld)", i, (long)s.n0, (long)s.n0 + s.cnt, s.hw + 1,
                 (long)s.len - s.hw);
    SY11_REQUIRE((s.first == 1) == (s.n0 == s.hw + 1) && (s.first == 0 || s.first == 1), "iq_fsk_filter: item %d: first = %d, but it starts at %ld of the usable span from %d", i,
                 s.first, (long)s.n0, s.hw + 1);
    SY11_REQUIRE((s.last == 1) == (s.n0 + s.cnt == s.len - s.hw) && (s.last == 0 || s.last == 1) && (s.last == 1 || s.cnt == FSK_TILE),
                 "iq_fsk_filter: item %d: last = %d with %d samples, but it ends at %ld of the usable span to %ld", i, s.last, s.cnt, (long)s.n0 + s.cnt,
                 (long)s.len - s.hw);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "iq_fsk_filter: item %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "iq_fsk_filter: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(fsk_filter_kernel, dim3(n_item), dim3(64), 0, (hipStream_t)stream, item, taps, (const float2*)in, y, rows);
  SY11_LAUNCH_CHECK("iq_fsk_filter");
  return SY11_OK;
}

extern "C" int sy11_fsk_symbols(int32_t n_item, const sy11_fsk_block* item_host, const sy11_fsk_block* item, int64_t n_in, const float* y,
                                int64_t n_sym, float* sym, int64_t n_rows, double* rows, void* stream) {
  SY11_REQUIRE(item_host && item && y && sym && rows, "fsk_symbols: null item table / filtered samples / symbols / row table");
  SY11_REQUIRE(n_item > 0 && n_in > 0 && n_in < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "fsk_symbols: need items, samples, symbols and rows, each below 2^31 (n_item=%d n_in=%ld n_sym=%ld n_rows=%ld)", n_item, (long)n_in,
               (long)n_sym, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)item | (uintptr_t)rows) & 7) == 0 && (((uintptr_t)y | (uintptr_t)sym) & 3) == 0 && y != sym,
               "fsk_symbols: item table / rows must be 8-byte aligned, y and the symbols 4-byte, and the symbols may not be y");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {
    const sy11_fsk_block& s = item_host[i];
    SY11_REQUIRE(s.off >= 0 && s.len >= 4 && s.len <= n_in && s.off <= n_in - s.len, "fsk_symbols: item %d: the clip [%ld, %ld) leaves the %ld packed samples", i,
                 (long)s.off, (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.n >= 1 && s.n <= FSK_BLOCK && s.sym_off >= 0 && s.sym_off <= n_sym - s.n, "fsk_symbols: item %d: symbols [%ld, %ld) are not 1 .. %d of the %ld packed symbols",
                 i, (long)s.sym_off, (long)s.sym_off + s.n, FSK_BLOCK, (long)n_sym);
    SY11_REQUIRE(s.step >= (1LL << 32) && s.step <= (1LL << 40) && s.t0 >= (1LL << 32) && s.t0 < (s.len << 32) &&
                     ((s.t0 + (int64_t)(s.n - 1) * s.step) >> 32) <= s.len - 3,
                 "fsk_symbols: item %d: positions from %ld in steps of %ld (Q32.32) leave [1, %ld]", i, (long)s.t0, (long)s.step, (long)s.len - 3);
    SY11_REQUIRE(isfinite(s.m), "fsk_symbols: item %d: the mean m is not finite", i);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "fsk_symbols: item %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "fsk_symbols: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(fsk_symbols_kernel, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, y, sym, rows);
  SY11_LAUNCH_CHECK("fsk_symbols");
  return SY11_OK;
}

extern "C" int sy11_fsk_decide(int32_t n_item, const sy11_fsk_dec* item_host, const sy11_fsk_dec* item, int64_t n_sym, const float* sym, float* r,
                               uint8_t* d, int64_t n_rows, double* rows, void* stream) {
  SY11_REQUIRE(item_host && item && sym && r && d && rows, "fsk_decide: null item table / symbols / output / row table");
  SY11_REQUIRE(n_item > 0 && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "fsk_decide: need items, symbols and rows, each below 2^31 (n_item=%d n_sym=%ld n_rows=%ld)", n_item, (long)n_sym, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)r | (uintptr_t)item | (uintptr_t)rows) & 7) == 0 && ((uintptr_t)sym & 3) == 0 && (const void*)sym != (const void*)r,
               "fsk_decide: r / item table / rows must be 8-byte aligned, the symbols 4-byte, and r may not be the symbols");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {
    const sy11_fsk_dec& s = item_host[i];
    SY11_REQUIRE(s.n >= 1 && s.n <= FSK_BLOCK && s.sym_off >= 0 && s.sym_off <= n_sym - s.n, "fsk_decide: item %d: symbols [%ld, %ld) are not 1 .. %d of the %ld packed symbols", i,
                 (long)s.sym_off, (long)s.sym_off + s.n, FSK_BLOCK, (long)n_sym);
    SY11_REQUIRE(isfinite(s.f0) && isfinite(s.dev) && s.dev > 0.0, "fsk_decide: item %d: f0 = %g, dev = %g: both must be finite and dev positive", i, s.f0, s.dev);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "fsk_decide: item %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "fsk_decide: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(fsk_decide_kernel, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, sym, (float2*)r, d, rows);
  SY11_LAUNCH_CHECK("fsk_decide");
  return SY11_OK;
}
