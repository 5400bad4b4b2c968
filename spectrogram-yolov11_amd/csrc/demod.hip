// demod.hip — demodulate every clip of an extraction, feed-forward: de-rotation + matched filter + timing partials (launch 1), cubic
// interpolation at the fitted symbol instants + the per-block sums of s^order (launch 2), de-rotation by the tracked carrier phase +
// decisions + the per-block error sums (launch 3), each over all clips at once.  The two fits between the launches (a line through the
// timing phases of the tiles, the unwrapped carrier phase of the blocks) are the host's, in float64 numpy.  No reference counterpart; spec in
// DESIGN.md §4, plan in sy11/data/demodulate.py.
//
//   launch 1, per (clip, tile of TILE usable samples):  xr[n] = x[n] e^{-2 pi i (n Wc mod 2^64) 2^-64},  y[n] = f32(sum_k xr[n - k] h[k])
//                                                       row = sum |y[n]|^2 e^{-2 pi i (n Ws mod 2^64) 2^-64}, sum |y[n]|^2          (f64)
//   launch 2, per (clip, block of symbols):             s_i = f32(cubic Lagrange of y[k - 1 .. k + 2] at mu), t_i = t0 + i step = (k + mu) 2^32
//                                                       row = sum s_i^order (negated at order 4), sum |s_i|^2                       (f64)
//   launch 3, per (clip, block of symbols):             r_i = f32(s_i e^{-i phi_i}), phi_i interpolated between block centres
//                                                       d_i, row = sum |r|^2, sum Re(r conj(point(d))), n                           (f64)
//
//  * Float64 throughout and ONE rounding, to the f32 value that is stored (y, s, r), as measure.hip and cyclo.hip do and for their reason:
//    the columns derived from the stored values (evm above all) are held to a float64 reference at 1e-9, and float32 sums of 50 .. 500
//    products leave y 1e-7 of its size away from it, which moves evm by several 1e-9 of itself.
//  * Launch 1 is the hot path: 2 hw + 1 complex x real MACs per sample.  One workgroup of ONE wave per item; the tile with its 2 hw halo
//    is de-rotated once while it is written to LDS (1040 complex128 samples) next to the taps (520 float64): 20.3 KB, so 7 workgroups
//    fit a CU.  A thread owns 8 ADJACENT outputs and walks the taps 8 at a time with a 16-sample register window: per 8 taps it reads 8
//    new samples and 8 broadcast taps from LDS for 128 float64 FMAs.  Sample i lies at [i % 8][i / 8], so that the 64 lanes, whose
//    windows are 8 samples apart, read 64 consecutive samples with every 16-byte read (no bank conflict; in their natural order the
//    same reads are 8 samples apart and conflicted).  Timings and what bounds it: DESIGN.md §6.
//  * The phase of sample n is the exact integer n Wc mod 2^64, whatever the tile.  A lane de-rotates the samples t, t + 64, ... of a
//    chunk: one float64 sincospi for its first sample, one for the step of 64 samples, and a float64 complex product per sample (17
//    of them at most: the recurrence stays within a few 1e-15).
//  * Every sum has one order: a thread's taps ascending, its 8 outputs ascending, a xor butterfly over the 64 lanes (and, in launches 2
//    and 3, the four waves ascending).  Nothing depends on the item's place in the launch.  No atomics.
#include "common.h"

#include <math.h>

#include <vector>

namespace {

constexpr int DEMOD_TILE = 512;                 // usable samples per item of launch 1
constexpr int DEMOD_TAPS = 513;                 // 2 * 16 * 16 + 1
constexpr int DEMOD_TAPS_LDS = 520;             // the taps padded with zeros to a multiple of 8
constexpr int DEMOD_SPAN = DEMOD_TILE + DEMOD_TAPS_LDS + 8;   // samples in LDS: the last window read ends at sample 504 + 512 + 15
constexpr int DEMOD_BLOCK = 256;                // symbols per block at most: one thread each

// e^{-2 pi i ph 2^-64} in float64
__device__ __forceinline__ void rot64(uint64_t ph, double& c, double& s) {
  double sn, cs;
  sincospi((double)(int64_t)ph * 0x1p-63, &sn, &cs);                      // half turns in [-1, 1)
  c = cs, s = -sn;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// acc[j] += w[j + m] h[m] for the 8 outputs j and the 8 taps m of one step, w = lo ++ hi; taps ascending, fused multiply-adds
__device__ __forceinline__ void demod_mac(double2 (&acc)[8], const double2 (&lo)[8], const double2 (&hi)[8], const double* __restrict__ tp) {
  double h[8];
#pragma unroll
  for (int m = 0; m < 8; m += 2) {
    const double2 v = *(const double2*)(tp + m);
    h[m] = v.x, h[m + 1] = v.y;
  }
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double2 w = j + m < 8 ? lo[j + m] : hi[j + m - 8];
      acc[j].x = fma(w.x, h[m], acc[j].x);
      acc[j].y = fma(w.y, h[m], acc[j].y);
    }
}

__global__ __launch_bounds__(64) void demod_filter_kernel(const sy11_demod_item* __restrict__ items, const float* __restrict__ taps,
                                                          const float2* __restrict__ in, float2* __restrict__ y, double* __restrict__ rows) {
  __shared__ double2 sm[8][DEMOD_SPAN / 8];                               // sample i of the chunk's span at sm[i % 8][i / 8]
  __shared__ __attribute__((aligned(16))) double tp[DEMOD_TAPS_LDS];
  const sy11_demod_item it = items[blockIdx.x];
  const int t = threadIdx.x, hw = it.hw, nblk = (it.n_taps + 7) >> 3;
  for (int i = t; i < DEMOD_TAPS_LDS; i += 64) tp[i] = i < it.n_taps ? (double)taps[it.tap_off + (it.n_taps - 1 - i)] : 0.0;
  // chunks of outputs: the clip's first hw samples (first item), the item's usable samples, the clip's last hw samples (last item)
  for (int c = 0; c < 3; ++c) {
    if ((c == 0 && !it.first) || (c == 2 && !it.last)) continue;
    const int64_t c0 = c == 0 ? 0 : c == 1 ? it.n0 : it.len - hw;
    const int cnt = c == 1 ? it.cnt : hw;
    __syncthreads();                                                      // the reads of the chunk before
    double cs, sn, qc, qs;                                                // the rotator of sample n and that of 64 samples
    rot64((uint64_t)(c0 - hw + t) * it.wc, cs, sn);
    rot64(64 * it.wc, qc, qs);
    for (int i = t; i < DEMOD_SPAN; i += 64) {
      const int64_t n = c0 - hw + i;
      double re = 0.0, im = 0.0;
      if (i < cnt + 2 * hw && n >= 0 && n < it.len) {
        const float2 v = in[it.off + n];
        const double a = (double)v.x, b = (double)v.y;
        re = a * cs - b * sn;
        im = a * sn + b * cs;
      }
      sm[i & 7][i >> 3] = make_double2(re, im);
      const double nc = cs * qc - sn * qs, ns = cs * qs + sn * qc;
      cs = nc, sn = ns;
    }
    __syncthreads();
    // the window is lo ++ hi; the two halves change roles from one step to the next, so that no register is moved
    double2 acc[8], wa[8], wb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = make_double2(0.0, 0.0), wa[j] = sm[j][t];                      // samples 8 t + j
    int blk = 0;
    for (; blk + 1 < nblk; blk += 2) {
#pragma unroll
      for (int j = 0; j < 8; ++j) wb[j] = sm[j][t + blk + 1];              // samples 8 t + 8 blk + 8 + j: the lanes read consecutive pairs
      demod_mac(acc, wa, wb, &tp[8 * blk]);
#pragma unroll
      for (int j = 0; j < 8; ++j) wa[j] = sm[j][t + blk + 2];
      demod_mac(acc, wb, wa, &tp[8 * blk + 8]);
    }
    if (blk < nblk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) wb[j] = sm[j][t + blk + 1];
      demod_mac(acc, wa, wb, &tp[8 * blk]);
    }
    float ar[8], ai[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ar[j] = (float)acc[j].x, ai[j] = (float)acc[j].y;      // the one rounding of y
    float2* dst = y + (it.off + c0 + 8 * t);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (8 * t + j < cnt) dst[j] = make_float2(ar[j], ai[j]);
    if (c != 1) continue;
    // the timing partials of the usable samples, from the float32 values just stored
    {
#pragma clang fp contract(off)
      double er, ei, qr, qi, Tr = 0.0, Ti = 0.0, P = 0.0;
      rot64((uint64_t)(c0 + 8 * t) * it.ws, er, ei);
      rot64(it.ws, qr, qi);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (8 * t + j < cnt) {
          const double a = (double)ar[j], b = (double)ai[j];
          const double p = a * a + b * b;
          Tr += p * er, Ti += p * ei, P += p;
        }
        const double nr = er * qr - ei * qi, ni = er * qi + ei * qr;
        er = nr, ei = ni;
      }
      Tr = wave_sum(Tr), Ti = wave_sum(Ti), P = wave_sum(P);
      if (t == 0) {
        double* o = rows + (int64_t)it.row * 3;
        o[0] = Tr, o[1] = Ti, o[2] = P;
      }
    }
  }
}

// the four waves' sums in ascending order -> thread 0
__device__ __forceinline__ double block_sum(double v, double* sh, int t) {
  v = wave_sum(v);
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void demod_symbols_kernel(const sy11_demod_block* __restrict__ items, const float2* __restrict__ y,
                                                            float2* __restrict__ sym, double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  const sy11_demod_block it = items[blockIdx.x];
  const int t = threadIdx.x;
  double zr = 0.0, zi = 0.0, p = 0.0;
  if (t < it.n) {
    const int64_t ti = it.t0 + (int64_t)t * it.step;
    const int64_t k = ti >> 32;
    const double mu = (double)(uint32_t)(((uint64_t)ti & 0xffffffffull) >> 8) * 0x1p-24;      // the top 24 bits of the fraction
    const float2* src = y + (it.off + k - 1);
    const float2 y0 = src[0], y1 = src[1], y2 = src[2], y3 = src[3];
    const double a = mu + 1.0, b = mu - 1.0, c = mu - 2.0;
    const double c0 = ((-mu * b) * c) / 6.0, c1 = ((a * b) * c) / 2.0, c2 = ((-a * mu) * c) / 2.0, c3 = ((a * mu) * b) / 6.0;
    const float sr = (float)(((c0 * (double)y0.x + c1 * (double)y1.x) + c2 * (double)y2.x) + c3 * (double)y3.x);      // the one rounding of s
    const float si = (float)(((c0 * (double)y0.y + c1 * (double)y1.y) + c2 * (double)y2.y) + c3 * (double)y3.y);
    sym[it.sym_off + t] = make_float2(sr, si);
    const double u = (double)sr, v = (double)si;
    const double x2r = u * u - v * v, x2i = 2.0 * (u * v);
    p = u * u + v * v;
    if (it.order == 2) zr = x2r, zi = x2i;
    else zr = -(x2r * x2r - x2i * x2i), zi = -(2.0 * (x2r * x2i));
  }
  zr = block_sum(zr, sh, t), zi = block_sum(zi, sh, t), p = block_sum(p, sh, t);
  if (t == 0) {
    double* o = rows + (int64_t)it.row * 3;
    o[0] = zr, o[1] = zi, o[2] = p;
  }
}

__global__ __launch_bounds__(256) void demod_decide_kernel(const sy11_demod_dec* __restrict__ items, const float2* __restrict__ sym,
                                                           const double* __restrict__ theta, float2* __restrict__ r, uint8_t* __restrict__ d,
                                                           double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  const sy11_demod_dec it = items[blockIdx.x];
  const int t = threadIdx.x, b = it.b, nb = it.nb;
  const int64_t j0 = (int64_t)b * it.block;
  const int n = (int)(it.n_sym - j0 < it.block ? it.n_sym - j0 : it.block);
  const double* th = theta + it.row0;
  double e2 = 0.0, er = 0.0;
  if (t < n) {
    // np.interp over the block centres: block q holds the symbols [q block, q block + n_q), its centre is q block + (n_q - 1) / 2
    const double x = (double)(j0 + t);
    const double n_last = (double)(it.n_sym - (int64_t)(nb - 1) * it.block);
    const double c_first = (nb == 1 ? n_last - 1.0 : (double)it.block - 1.0) * 0.5;
    const double c_last = (double)((int64_t)(nb - 1) * it.block) + (n_last - 1.0) * 0.5;
    double phi;
    if (x <= c_first) phi = th[0];
    else if (x >= c_last) phi = th[nb - 1];
    else {
      const double c_b = (double)j0 + ((double)n - 1.0) * 0.5;
      const int lo = x >= c_b ? b : b - 1;
      const double x_lo = (double)((int64_t)lo * it.block) + ((double)it.block - 1.0) * 0.5;      // lo < nb - 1: a full block
      const double x_hi = lo + 1 == nb - 1 ? c_last : (double)((int64_t)(lo + 1) * it.block) + ((double)it.block - 1.0) * 0.5;
      const double slope = (th[lo + 1] - th[lo]) / (x_hi - x_lo);
      phi = slope * (x - x_lo) + th[lo];
    }
    double sn, cs;
    sincos(phi, &sn, &cs);
    const float2 s = sym[it.sym_off + j0 + t];
    const double sx = (double)s.x, sy = (double)s.y;
    const float rr = (float)(sx * cs + sy * sn), ri = (float)(sy * cs - sx * sn);                 // the one rounding of r
    r[it.sym_off + j0 + t] = make_float2(rr, ri);
    const int nr = rr < 0.0f, ni = ri < 0.0f;
    const double u = (double)rr, v = (double)ri;
    e2 = u * u + v * v;
    if (it.order == 2) {
      d[it.sym_off + j0 + t] = (uint8_t)nr;
      er = nr ? -u : u;
    } else {
      d[it.sym_off + j0 + t] = (uint8_t)(2 * nr + ni);
      er = ((nr ? -u : u) + (ni ? -v : v)) * 0.70710678118654752440;
    }
  }
  e2 = block_sum(e2, sh, t), er = block_sum(er, sh, t);
  if (t == 0) {
    double* o = rows + (it.row0 + b) * 3;
    o[0] = e2, o[1] = er, o[2] = (double)n;
  }
}

}  // namespace

extern "C" int32_t sy11_iq_demod_tile(void) { return DEMOD_TILE; }

extern "C" int sy11_iq_demod_filter(int32_t n_item, const sy11_demod_item* item_host, const sy11_demod_item* item, int64_t n_tap, const float* taps,
                                    int64_t n_in, const float* in, float* y, int64_t n_rows, double* rows, void* stream) {
  SY11_REQUIRE(item_host && item && taps && in && y && rows, "iq_demod_filter: null item table / taps / input / output / row table");
  SY11_REQUIRE(n_item > 0 && n_tap > 0 && n_tap < (1LL << 31) && n_in > 0 && n_in < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "iq_demod_filter: need items, taps, input and rows, each below 2^31 (n_item=%d n_tap=%ld n_in=%ld n_rows=%ld)", n_item, (long)n_tap,
               (long)n_in, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)y | (uintptr_t)item | (uintptr_t)rows) & 7) == 0 && ((uintptr_t)taps & 3) == 0 && in != y,
               "iq_demod_filter: in / y / item table / rows must be 8-byte aligned, the taps 4-byte, and y may not be in");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {                                      // no item reads outside in[] / taps[] or writes outside y / rows
    const sy11_demod_item& s = item_host[i];
    SY11_REQUIRE(s.off >= 0 && s.len >= 1 && s.len <= n_in && s.off <= n_in - s.len, "iq_demod_filter: item %d: the clip [%ld, %ld) leaves the %ld packed samples", i,
                 (long)s.off, (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.hw >= 1 && s.n_taps == 2 * s.hw + 1 && s.n_taps <= DEMOD_TAPS, "iq_demod_filter: item %d: %d taps for a half width of %d (odd, 2 hw + 1, at most %d)", i,
                 s.n_taps, s.hw, DEMOD_TAPS);
    SY11_REQUIRE(s.tap_off >= 0 && s.tap_off <= n_tap - s.n_taps, "iq_demod_filter: item %d: taps [%ld, %ld) leave the %ld packed taps", i, (long)s.tap_off,
                 (long)s.tap_off + s.n_taps, (long)n_tap);
    SY11_REQUIRE(s.n0 >= s.hw && (s.n0 - s.hw) % DEMOD_TILE == 0 && s.cnt >= 1 && s.cnt <= DEMOD_TILE && s.n0 <= s.len - s.hw - s.cnt,
                 "iq_demod_filter: item %d: samples [%ld, %ld) are not a tile of the usable span [%d, %ld)", i, (long)s.n0, (long)s.n0 + s.cnt, s.hw,
                 (long)s.len - s.hw);
    SY11_REQUIRE((s.first == 1) == (s.n0 == s.hw) && (s.first == 0 || s.first == 1), "iq_demod_filter: item %d: first = %d, but it starts at %ld of the usable span from %d", i,
                 s.first, (long)s.n0, s.hw);
    SY11_REQUIRE((s.last == 1) == (s.n0 + s.cnt == s.len - s.hw) && (s.last == 0 || s.last == 1) && (s.last == 1 || s.cnt == DEMOD_TILE),
                 "iq_demod_filter: item %d: last = %d with %d samples, but it ends at %ld of the usable span to %ld", i, s.last, s.cnt, (long)s.n0 + s.cnt,
                 (long)s.len - s.hw);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "iq_demod_filter: item %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "iq_demod_filter: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(demod_filter_kernel, dim3(n_item), dim3(64), 0, (hipStream_t)stream, item, taps, (const float2*)in, (float2*)y, rows);
  SY11_LAUNCH_CHECK("iq_demod_filter");
  return SY11_OK;
}

extern "C" int sy11_demod_symbols(int32_t n_item, const sy11_demod_block* item_host, const sy11_demod_block* item, int64_t n_in, const float* y,
                                  int64_t n_sym, float* sym, int64_t n_rows, double* rows, void* stream) {
  SY11_REQUIRE(item_host && item && y && sym && rows, "demod_symbols: null item table / filtered samples / symbols / row table");
  SY11_REQUIRE(n_item > 0 && n_in > 0 && n_in < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "demod_symbols: need items, samples, symbols and rows, each below 2^31 (n_item=%d n_in=%ld n_sym=%ld n_rows=%ld)", n_item, (long)n_in,
               (long)n_sym, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)y | (uintptr_t)sym | (uintptr_t)item | (uintptr_t)rows) & 7) == 0, "demod_symbols: y / symbols / item table / rows must be 8-byte aligned");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {
    const sy11_demod_block& s = item_host[i];
    SY11_REQUIRE(s.off >= 0 && s.len >= 4 && s.len <= n_in && s.off <= n_in - s.len, "demod_symbols: item %d: the clip [%ld, %ld) leaves the %ld packed samples", i,
                 (long)s.off, (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.n >= 1 && s.n <= DEMOD_BLOCK && s.sym_off >= 0 && s.sym_off <= n_sym - s.n, "demod_symbols: item %d: symbols [%ld, %ld) are not 1 .. %d of the %ld packed symbols",
                 i, (long)s.sym_off, (long)s.sym_off + s.n, DEMOD_BLOCK, (long)n_sym);
    SY11_REQUIRE(s.step >= (1LL << 32) && s.step <= (1LL << 40) && s.t0 >= (1LL << 32) && s.t0 < (s.len << 32) &&
                     ((s.t0 + (int64_t)(s.n - 1) * s.step) >> 32) <= s.len - 3,
                 "demod_symbols: item %d: positions from %ld in steps of %ld (Q32.32) leave [1, %ld]", i, (long)s.t0, (long)s.step, (long)s.len - 3);
    SY11_REQUIRE(s.order == 2 || s.order == 4, "demod_symbols: item %d: order %d is not 2 or 4", i, s.order);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "demod_symbols: item %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "demod_symbols: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(demod_symbols_kernel, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, (const float2*)y, (float2*)sym, rows);
  SY11_LAUNCH_CHECK("demod_symbols");
  return SY11_OK;
}

extern "C" int sy11_demod_decide(int32_t n_item, const sy11_demod_dec* item_host, const sy11_demod_dec* item, int64_t n_sym, const float* sym,
                                 int64_t n_rows, const double* theta, float* r, uint8_t* d, double* rows, void* stream) {
  SY11_REQUIRE(item_host && item && sym && theta && r && d && rows, "demod_decide: null item table / symbols / phase table / output / row table");
  SY11_REQUIRE(n_item > 0 && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "demod_decide: need items, symbols and rows, each below 2^31 (n_item=%d n_sym=%ld n_rows=%ld)", n_item, (long)n_sym, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)sym | (uintptr_t)r | (uintptr_t)item | (uintptr_t)rows | (uintptr_t)theta) & 7) == 0 && sym != r,
               "demod_decide: symbols / r / item table / phase table / rows must be 8-byte aligned, and r may not be the symbols");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_item; ++i) {
    const sy11_demod_dec& s = item_host[i];
    SY11_REQUIRE(s.n_sym >= 1 && s.sym_off >= 0 && s.sym_off <= n_sym - s.n_sym, "demod_decide: item %d: symbols [%ld, %ld) leave the %ld packed symbols", i, (long)s.sym_off,
                 (long)s.sym_off + s.n_sym, (long)n_sym);
    SY11_REQUIRE(s.block >= 8 && s.block <= DEMOD_BLOCK && s.nb >= 1 && (int64_t)s.nb == (s.n_sym + s.block - 1) / s.block && s.b >= 0 && s.b < s.nb,
                 "demod_decide: item %d: block %d of %d blocks of %d does not fit %ld symbols", i, s.b, s.nb, s.block, (long)s.n_sym);
    SY11_REQUIRE(s.row0 >= 0 && s.row0 <= n_rows - s.nb, "demod_decide: item %d: rows [%ld, %ld) leave a table of %ld rows", i, (long)s.row0, (long)s.row0 + s.nb,
                 (long)n_rows);
    SY11_REQUIRE(s.order == 2 || s.order == 4, "demod_decide: item %d: order %d is not 2 or 4", i, s.order);
    SY11_REQUIRE(!seen[(size_t)(s.row0 + s.b)], "demod_decide: item %d writes row %ld, which an earlier item of this call writes", i, (long)s.row0 + s.b);
    seen[(size_t)(s.row0 + s.b)] = true;
  }
  hipLaunchKernelGGL(demod_decide_kernel, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, (const float2*)sym, theta, (float2*)r, d, rows);
  SY11_LAUNCH_CHECK("demod_decide");
  return SY11_OK;
}
