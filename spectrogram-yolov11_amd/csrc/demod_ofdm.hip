// demod_ofdm.hip — demodulate every OFDM clip of an extraction, feed-forward: the cyclic-prefix correlation folded over the OFDM period (launch 1),
// the de-rotated FFT of every OFDM symbol with its used carriers, pilot rows and power (launch 2), the data carriers turned by the pilots' fit
// + decisions + the per-symbol error sums (launch 3), each over all clips at once.  The two fits between the launches (the prefix position
// and fractional carrier offset; the pilots' slope, phase and amplitude) are the host's, in float64 numpy.  No reference counterpart; spec in
// DESIGN.md §4, plan in sy11/data/demodulate_ofdm.py.
//
//   clip x[0 .. M), FFT size N, prefix G, S = N + G, L = (M - N) / S whole periods
//   launch 1, per (clip, tile of 64 residues, split of 16 periods):  F[r] = sum_m x[r + m S + N] conj(x[r + m S]),  E[r] = sum_m (|x[r + m S]|^2 + |x[r + m S + N]|^2) / 2   (f64)
//   launch 2, per (clip, group of 1024 / N OFDM symbols):            v[q] = x[start + q] e^{-2 pi i ((start + q) W mod 2^64) 2^-64},  Y[k] = FFT_N(v)[k] e^{+2 pi i k a / N}
//                                                                    Yc = f32(Y) on the used carriers, u_p = Y[k_p] c_p (f64), sum_used |Y|^2 (f64)
//   launch 3, per OFDM symbol:                                       r_j = f32(Yc[data j] rho tau_j),  d_j,  row = sum |r|^2, sum Re(r conj(point(d))), n_data   (f64)
//
//  * Float64 throughout and ONE rounding, to the f32 value that is stored (Yc, r), as demod.hip does and for its reason.
//  * Launch 1 is one thread per residue, consecutive residues in consecutive lanes: both reads, x[n] and x[n + N], are coalesced, every
//    sample is read twice and nothing else is read.  A thread adds its periods in ascending order; the periods of a long clip are split
//    16 at a time over items that write one partial row each, which the host adds in ascending order.  No atomics.
//  * Launch 2 is cyclo_kernel's frame pass with ONE transform: 256 threads, the 1024-slot LDS image of fft_lds.h holds 1024 / N OFDM symbols.
//    The clips of one call may differ in N, so the switch over L sits in the kernel (it is uniform over a workgroup).  The twiddles of every N
//    are a stride of the one table of N = 1024.  The advance turn e^{+2 pi i k a / N} is an entry of that table: exact.
//  * Every sum has one order: a thread's terms ascending, a xor butterfly over the lanes of a symbol, the waves of a symbol ascending.
//    Nothing depends on the item's place in the launch.
#include "common.h"
#include "fft_lds.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace {

using namespace sy11_fft;

constexpr int OFDM_FOLD_TILE = 64;              // residues per item of launch 1: one thread each
constexpr int OFDM_FOLD_PERIODS = 16;           // periods per item of launch 1 at most: the split rule of the plan
constexpr int OFDM_TW = 512;                    // entries of the twiddle table: e^{-2 pi i m / 1024}, m < 512

// e^{-2 pi i ph 2^-64} in float64 (the rotation of demod.hip)
__device__ __forceinline__ void ofdm_rot64(uint64_t ph, double& c, double& s) {
  double sn, cs;
  sincospi((double)(int64_t)ph * 0x1p-63, &sn, &cs);                      // half turns in [-1, 1)
  c = cs, s = -sn;
}

__global__ __launch_bounds__(OFDM_FOLD_TILE) void ofdm_fold_kernel(const sy11_ofdm_fold_item* __restrict__ items, const float2* __restrict__ in,
                                                                   double* __restrict__ out) {
#pragma clang fp contract(off)
  const sy11_ofdm_fold_item it = items[blockIdx.x];
  const int t = threadIdx.x;
  if (t >= it.cnt_r) return;
  const float2* p = in + (it.off + it.r0 + t + (int64_t)it.m0 * it.S);
  double fr = 0.0, fi = 0.0, e = 0.0;
  for (int m = 0; m < it.cnt_m; ++m) {                                    // ascending; the products of two float32 are exact in float64
    const float2 a = p[0], b = p[it.n_fft];
    const double ax = (double)a.x, ay = (double)a.y, bx = (double)b.x, by = (double)b.y;
    fr += bx * ax + by * ay;
    fi += by * ax - bx * ay;
    e += 0.5 * ((ax * ax + ay * ay) + (bx * bx + by * by));
    p += it.S;
  }
  double* o = out + 3 * (it.out_off + t);
  o[0] = fr, o[1] = fi, o[2] = e;
}

template <int L>
__device__ __forceinline__ void ofdm_fft_body(const sy11_ofdm_fft_item& it, const sy11_ofdm_bin* __restrict__ bins, const double2* __restrict__ twiddle,
                                              const float2* __restrict__ in, float2* __restrict__ yc, double2* __restrict__ pil, double* __restrict__ pw_out,
                                              double2* xs, double* pw, double2* tw, double* sh, const int t) {
  constexpr int N = 1 << L, H = N / 2, FR = FFT_SLOTS / N, h2 = N / 4, T = N / 4;      // T threads per OFDM symbol
  for (int i = t; i < H; i += 256) tw[i] = twiddle[i * FR];
  __syncthreads();
  const int base = fft_first_slot<L>(t), f = base >> L, p = base & (N - 1);
  double2 e[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) e[m] = make_double2(0.0, 0.0);
  if (f < it.nf) {
    const int64_t n0 = it.start + (int64_t)f * it.S + p;
    const float2* src = in + (it.off + n0);
    double c, s, qc, qs;
    ofdm_rot64((uint64_t)n0 * it.w, c, s);
    ofdm_rot64((uint64_t)h2 * it.w, qc, qs);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float2 v = src[m * h2];
      const double vx = (double)v.x, vy = (double)v.y;
      e[m] = make_double2(vx * c - vy * s, vx * s + vy * c);
      const double nc = c * qc - s * qs, ns = c * qs + s * qc;
      c = nc, s = ns;
    }
  }
  fft_rounds<L>(e, xs, tw, t);
  __syncthreads();                                                        // every read of the last round precedes the writes below
#pragma unroll
  for (int m = 0; m < 4; ++m) {                                           // slot q of a frame is bin bitrev_L(q): the image in bin order
    const int q = 4 * t + m;
    xs[(q & ~(N - 1)) | (int)(__brev((unsigned)(q & (N - 1))) >> (32 - L))] = e[m];
  }
  __syncthreads();
  const int nu = it.n_used, total = it.nf * nu;
  for (int idx = t; idx < total; idx += 256) {
    const int fr = idx / nu, j = idx - fr * nu;
    const sy11_ofdm_bin b = bins[it.bin_off + j];
    const double2 Y = xs[(fr << L) | (b.k & (N - 1))];
    const int ia = (b.k * it.a) & (N - 1);                                // (k a) mod N
    const double2 wh = tw[ia & (H - 1)];
    const double wx = ia >= H ? -wh.x : wh.x, wy = ia >= H ? -wh.y : wh.y;        // e^{-2 pi i (k a mod N) / N}; Y times its conjugate
    const double yr = Y.x * wx + Y.y * wy, yi = Y.y * wx - Y.x * wy;
    yc[it.yc_off + idx] = make_float2((float)yr, (float)yi);              // the one rounding of Yc
    pw[(fr << L) | j] = yr * yr + yi * yi;
    if (b.pil != 0) {
      const int pp = (b.pil < 0 ? -b.pil : b.pil) - 1;
      pil[it.pil_off + (int64_t)fr * it.n_pil + pp] = b.pil < 0 ? make_double2(-yr, -yi) : make_double2(yr, yi);
    }
  }
  __syncthreads();
  // the power of every OFDM symbol: T threads each, terms ascending, a butterfly over the symbol's lanes, its waves ascending
  {
#pragma clang fp contract(off)
    const int fr = t / T, lt = t % T;
    double v = 0.0;
    if (fr < it.nf)
      for (int j = lt; j < nu; j += T) v += pw[(fr << L) | j];
#pragma unroll
    for (int d = (T < 64 ? T : 64) / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if constexpr (T <= 64) {
      if (lt == 0 && fr < it.nf) pw_out[it.pow_off + fr] = v;
    } else {
      if ((t & 63) == 0) sh[t >> 6] = v;
      __syncthreads();
      if (lt == 0 && fr < it.nf) {
        constexpr int Wv = T / 64 > 0 ? T / 64 : 1;
        double s = sh[fr * Wv];
#pragma unroll
        for (int w = 1; w < Wv; ++w) s += sh[fr * Wv + w];
        pw_out[it.pow_off + fr] = s;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ofdm_fft_kernel(const sy11_ofdm_fft_item* __restrict__ items, const sy11_ofdm_bin* __restrict__ bins,
                                                       const double2* __restrict__ twiddle, const float2* __restrict__ in, float2* __restrict__ yc,
                                                       double2* __restrict__ pil, double* __restrict__ pw_out) {
  __shared__ double2 xs[FFT_SLOTS];
  __shared__ double pw[FFT_SLOTS];
  __shared__ double2 tw[OFDM_TW];
  __shared__ double sh[4];
  const sy11_ofdm_fft_item it = items[blockIdx.x];
  const int t = threadIdx.x;
  switch (it.n_fft) {                                                     // uniform over the workgroup
    case 64: ofdm_fft_body<6>(it, bins, twiddle, in, yc, pil, pw_out, xs, pw, tw, sh, t); break;
    case 128: ofdm_fft_body<7>(it, bins, twiddle, in, yc, pil, pw_out, xs, pw, tw, sh, t); break;
    case 256: ofdm_fft_body<8>(it, bins, twiddle, in, yc, pil, pw_out, xs, pw, tw, sh, t); break;
    case 512: ofdm_fft_body<9>(it, bins, twiddle, in, yc, pil, pw_out, xs, pw, tw, sh, t); break;
    default: ofdm_fft_body<10>(it, bins, twiddle, in, yc, pil, pw_out, xs, pw, tw, sh, t); break;
  }
}

__device__ __forceinline__ double ofdm_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the four waves' sums in ascending order -> every thread
__device__ __forceinline__ double ofdm_block_sum(double v, double* sh, int t) {
  v = ofdm_wave_sum(v);
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void ofdm_decide_kernel(const sy11_ofdm_dec* __restrict__ items, const sy11_ofdm_car* __restrict__ cars,
                                                          const float2* __restrict__ yc, float2* __restrict__ r, uint8_t* __restrict__ d,
                                                          double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  const sy11_ofdm_dec it = items[blockIdx.x];
  const int t = threadIdx.x;
  double e2 = 0.0, er = 0.0;
  for (int j = t; j < it.n_data; j += 256) {                              // a thread's carriers ascending
    const sy11_ofdm_car c = cars[it.car_off + j];
    const float2 y = yc[it.yc_off + c.idx];
    const double yx = (double)y.x, yy = (double)y.y;
    const double ax = yx * it.rho_r - yy * it.rho_i, ay = yx * it.rho_i + yy * it.rho_r;          // (Yc rho) tau
    const float rr = (float)(ax * c.tr - ay * c.ti), ri = (float)(ax * c.ti + ay * c.tr);         // the one rounding of r
    r[it.sym_off + j] = make_float2(rr, ri);
    const int nr = rr < 0.0f, ni = ri < 0.0f;
    const double u = (double)rr, v = (double)ri;
    e2 += u * u + v * v;
    if (it.order == 2) {
      d[it.sym_off + j] = (uint8_t)nr;
      er += nr ? -u : u;
    } else {
      d[it.sym_off + j] = (uint8_t)(2 * nr + ni);
      er += ((nr ? -u : u) + (ni ? -v : v)) * 0.70710678118654752440;
    }
  }
  e2 = ofdm_block_sum(e2, sh, t), er = ofdm_block_sum(er, sh, t);
  if (t == 0) {
    double* o = rows + (int64_t)it.row * 3;
    o[0] = e2, o[1] = er, o[2] = (double)it.n_data;
  }
}

// what an item writes: entries [a, a + n) of a buffer
struct OfdmSpan {
  int64_t a, n;
  int item;
};

// The first item (in table order) that writes an entry an earlier item writes, -1 when no two spans overlap: the spans sorted by their start, each
// against the furthest end before it.  The plan's tables ascend already, which is one pass; any other order is sorted first.
int ofdm_overlap(std::vector<OfdmSpan>& v) {
  const auto before = [](const OfdmSpan& x, const OfdmSpan& y) { return x.a != y.a ? x.a < y.a : x.item < y.item; };
  if (!std::is_sorted(v.begin(), v.end(), before)) std::sort(v.begin(), v.end(), before);
  int bad = -1, end_item = -1;
  int64_t end = INT64_MIN;
  for (const OfdmSpan& s : v) {
    if (s.a < end) {
      const int later = s.item > end_item ? s.item : end_item;
      if (bad < 0 || later < bad) bad = later;
    }
    if (s.a + s.n > end) end = s.a + s.n, end_item = s.item;
  }
  return bad;
}

}  // namespace

extern "C" int sy11_iq_ofdm_fold(int32_t n_item, const sy11_ofdm_fold_item* item_host, const sy11_ofdm_fold_item* item, int64_t n_in, const float* in,
                                 int64_t n_out, double* out, void* stream) {
  SY11_REQUIRE(item_host && item && in && out, "iq_ofdm_fold: null item table / input / output");
  SY11_REQUIRE(n_item > 0 && n_in > 0 && n_in < (1LL << 31) && n_out > 0 && n_out < (1LL << 31),
               "iq_ofdm_fold: need items, input and output triples, each below 2^31 (n_item=%d n_in=%ld n_out=%ld)", n_item, (long)n_in, (long)n_out);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)item | (uintptr_t)out) & 7) == 0, "iq_ofdm_fold: in / item table / out must be 8-byte aligned");
  std::vector<OfdmSpan> spans;
  spans.reserve((size_t)n_item);
  for (int i = 0; i < n_item; ++i) {                                      // no item reads outside in[] or writes outside out
    const sy11_ofdm_fold_item& s = item_host[i];
    SY11_REQUIRE(log2_fft(s.n_fft) != 0, "iq_ofdm_fold: item %d: n_fft = %d is not one of 64, 128, 256, 512, 1024", i, s.n_fft);
    SY11_REQUIRE(s.S > s.n_fft && s.S <= s.n_fft + s.n_fft / 2, "iq_ofdm_fold: item %d: a period of %d samples is not n_fft + a prefix of 1 .. %d", i, s.S, s.n_fft / 2);
    SY11_REQUIRE(s.off >= 0 && s.len >= 1 && s.len <= n_in && s.off <= n_in - s.len, "iq_ofdm_fold: item %d: the clip [%ld, %ld) leaves the %ld packed samples", i,
                 (long)s.off, (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.r0 >= 0 && s.r0 < s.S && s.r0 % OFDM_FOLD_TILE == 0 && s.cnt_r == (s.S - s.r0 < OFDM_FOLD_TILE ? s.S - s.r0 : OFDM_FOLD_TILE),
                 "iq_ofdm_fold: item %d: residues [%d, %ld) are not a tile of %d of the period's %d", i, s.r0, (long)s.r0 + s.cnt_r, OFDM_FOLD_TILE, s.S);
    const int64_t Lp = (s.len - s.n_fft) / s.S;                           // whole periods: r + m S + N < len for every r < S, m < Lp
    SY11_REQUIRE(s.len >= s.n_fft && s.m0 >= 0 && s.m0 % OFDM_FOLD_PERIODS == 0 && s.cnt_m >= 1 && s.cnt_m <= OFDM_FOLD_PERIODS && (int64_t)s.m0 + s.cnt_m <= Lp &&
                     (s.cnt_m == OFDM_FOLD_PERIODS || (int64_t)s.m0 + s.cnt_m == Lp),
                 "iq_ofdm_fold: item %d: periods [%d, %ld) are not a split of %d of the clip's %ld", i, s.m0, (long)s.m0 + s.cnt_m, OFDM_FOLD_PERIODS, (long)Lp);
    SY11_REQUIRE(s.out_off >= 0 && s.out_off <= n_out - s.cnt_r, "iq_ofdm_fold: item %d writes triples [%ld, %ld) of %ld", i, (long)s.out_off, (long)s.out_off + s.cnt_r,
                 (long)n_out);
    spans.push_back({s.out_off, s.cnt_r, i});
  }
  const int twice = ofdm_overlap(spans);
  SY11_REQUIRE(twice < 0, "iq_ofdm_fold: item %d writes triples which an earlier item of this call writes", twice);
  hipLaunchKernelGGL(ofdm_fold_kernel, dim3(n_item), dim3(OFDM_FOLD_TILE), 0, (hipStream_t)stream, item, (const float2*)in, out);
  SY11_LAUNCH_CHECK("iq_ofdm_fold");
  return SY11_OK;
}

extern "C" int sy11_ofdm_fft(int32_t n_item, const sy11_ofdm_fft_item* item_host, const sy11_ofdm_fft_item* item, int32_t n_bin, const sy11_ofdm_bin* bin_host,
                             const sy11_ofdm_bin* bin, const double* twiddle, int64_t n_in, const float* in, int64_t n_yc, float* yc, int64_t n_pil, double* pil,
                             int64_t n_pow, double* pw, void* stream) {
  SY11_REQUIRE(item_host && item && bin_host && bin && twiddle && in && yc && pil && pw, "ofdm_fft: null item table / carrier table / twiddle table / input / output");
  SY11_REQUIRE(n_item > 0 && n_bin > 0 && n_in > 0 && n_in < (1LL << 31) && n_yc > 0 && n_yc < (1LL << 31) && n_pil > 0 && n_pil < (1LL << 31) && n_pow > 0 &&
                   n_pow < (1LL << 31),
               "ofdm_fft: need items, carriers, input, carrier values, pilot values and power rows, each below 2^31 (n_item=%d n_bin=%d n_in=%ld n_yc=%ld n_pil=%ld n_pow=%ld)",
               n_item, n_bin, (long)n_in, (long)n_yc, (long)n_pil, (long)n_pow);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)item | (uintptr_t)bin | (uintptr_t)yc | (uintptr_t)pw) & 7) == 0 && (((uintptr_t)twiddle | (uintptr_t)pil) & 15) == 0 &&
                   (const void*)in != (const void*)yc,
               "ofdm_fft: in / item table / carrier table / yc / power rows must be 8-byte aligned, the twiddle table and the pilot values 16-byte, and yc may not be in");
  std::vector<OfdmSpan> span_y, span_p, span_w;
  span_y.reserve((size_t)n_item), span_p.reserve((size_t)n_item), span_w.reserve((size_t)n_item);
  std::vector<int> slot;
  int32_t ok_off = -1, ok_used = -1, ok_pil = -1, ok_fft = -1;            // the carrier layout checked last: the items of a clip share theirs
  for (int i = 0; i < n_item; ++i) {
    const sy11_ofdm_fft_item& s = item_host[i];
    const int L = log2_fft(s.n_fft);
    SY11_REQUIRE(L != 0, "ofdm_fft: item %d: n_fft = %d is not one of 64, 128, 256, 512, 1024", i, s.n_fft);
    const int N = s.n_fft;
    SY11_REQUIRE(s.S > N && s.S <= N + N / 2 && s.a >= 0 && s.a <= s.S - N, "ofdm_fft: item %d: a period of %d samples with an advance of %d is not n_fft + a prefix of 1 .. %d with 0 <= a <= prefix",
                 i, s.S, s.a, N / 2);
    SY11_REQUIRE(s.off >= 0 && s.len >= 1 && s.len <= n_in && s.off <= n_in - s.len, "ofdm_fft: item %d: the clip [%ld, %ld) leaves the %ld packed samples", i, (long)s.off,
                 (long)s.off + s.len, (long)n_in);
    SY11_REQUIRE(s.nf >= 1 && s.nf <= FFT_SLOTS / N && s.start >= 0 && s.start <= s.len - N - (int64_t)(s.nf - 1) * s.S,
                 "ofdm_fft: item %d: %d OFDM symbols (1 .. %d) from sample %ld leave the clip's %ld samples", i, s.nf, FFT_SLOTS / N, (long)s.start, (long)s.len);
    SY11_REQUIRE(s.n_used >= 1 && s.n_used < N && s.n_pil >= 1 && s.n_pil <= s.n_used && s.bin_off >= 0 && s.bin_off <= n_bin - s.n_used,
                 "ofdm_fft: item %d: carriers [%d, %ld) with %d pilots are not 1 .. %d of the table's %d", i, s.bin_off, (long)s.bin_off + s.n_used, s.n_pil, N - 1, n_bin);
    if (!(s.bin_off == ok_off && s.n_used == ok_used && s.n_pil == ok_pil && s.n_fft == ok_fft)) {
      slot.assign((size_t)s.n_pil, 0);
      int found = 0;
      for (int j = 0; j < s.n_used; ++j) {
        const sy11_ofdm_bin& b = bin_host[s.bin_off + j];
        SY11_REQUIRE(b.k > -N / 2 && b.k < N / 2 && (j == 0 || b.k > bin_host[s.bin_off + j - 1].k),
                     "ofdm_fft: item %d: carrier %d of its table is k = %d: not ascending inside (-%d, %d)", i, j, b.k, N / 2, N / 2);
        const int64_t ap = b.pil < 0 ? -(int64_t)b.pil : (int64_t)b.pil;  // a pilot is named by +-(its slot + 1): the sign is its value
        const int pp = ap >= 1 && ap <= s.n_pil ? (int)(ap - 1) : -1;
        SY11_REQUIRE(b.pil == 0 || (pp >= 0 && !slot[(size_t)pp]), "ofdm_fft: item %d: carrier %d of its table names pilot %d of %d, or names one twice", i, j,
                     b.pil, s.n_pil);
        if (b.pil != 0) slot[(size_t)pp] = 1, ++found;
      }
      SY11_REQUIRE(found == s.n_pil, "ofdm_fft: item %d: its carriers name %d of its %d pilots", i, found, s.n_pil);
      ok_off = s.bin_off, ok_used = s.n_used, ok_pil = s.n_pil, ok_fft = s.n_fft;
    }
    const int64_t ny = (int64_t)s.nf * s.n_used, np = (int64_t)s.nf * s.n_pil;
    SY11_REQUIRE(s.yc_off >= 0 && s.yc_off <= n_yc - ny && s.pil_off >= 0 && s.pil_off <= n_pil - np && s.pow_off >= 0 && s.pow_off <= n_pow - s.nf,
                 "ofdm_fft: item %d writes carrier values [%ld, %ld) of %ld, pilot values [%ld, %ld) of %ld and power rows [%ld, %ld) of %ld", i, (long)s.yc_off,
                 (long)(s.yc_off + ny), (long)n_yc, (long)s.pil_off, (long)(s.pil_off + np), (long)n_pil, (long)s.pow_off, (long)s.pow_off + s.nf, (long)n_pow);
    span_y.push_back({s.yc_off, ny, i}), span_p.push_back({s.pil_off, np, i}), span_w.push_back({s.pow_off, s.nf, i});
  }
  int twice = ofdm_overlap(span_y);
  for (std::vector<OfdmSpan>* v : {&span_p, &span_w}) {
    const int t = ofdm_overlap(*v);
    if (t >= 0 && (twice < 0 || t < twice)) twice = t;
  }
  SY11_REQUIRE(twice < 0, "ofdm_fft: item %d writes carrier values, pilot values or power rows which an earlier item of this call writes", twice);
  hipLaunchKernelGGL(ofdm_fft_kernel, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, bin, (const double2*)twiddle, (const float2*)in, (float2*)yc, (double2*)pil, pw);
  SY11_LAUNCH_CHECK("ofdm_fft");
  return SY11_OK;
}

extern "C" int sy11_ofdm_decide(int32_t n_item, const sy11_ofdm_dec* item_host, const sy11_ofdm_dec* item, int32_t n_car, const sy11_ofdm_car* car_host,
                                const sy11_ofdm_car* car, int64_t n_yc, const float* yc, int64_t n_sym, float* r, uint8_t* d, int64_t n_rows, double* rows,
                                void* stream) {
  SY11_REQUIRE(item_host && item && car_host && car && yc && r && d && rows, "ofdm_decide: null item table / carrier table / carrier values / output / row table");
  SY11_REQUIRE(n_item > 0 && n_car > 0 && n_yc > 0 && n_yc < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "ofdm_decide: need items, carriers, carrier values, symbols and rows, each below 2^31 (n_item=%d n_car=%d n_yc=%ld n_sym=%ld n_rows=%ld)", n_item, n_car,
               (long)n_yc, (long)n_sym, (long)n_rows);
  SY11_REQUIRE((((uintptr_t)yc | (uintptr_t)r | (uintptr_t)item | (uintptr_t)car | (uintptr_t)rows) & 7) == 0 && (const void*)yc != (const void*)r,
               "ofdm_decide: yc / r / item table / carrier table / rows must be 8-byte aligned, and r may not be yc");
  std::vector<bool> seen((size_t)n_rows, false);
  std::vector<OfdmSpan> spans;
  spans.reserve((size_t)n_item);
  int32_t ok_off = -1, ok_data = -1, ok_used = -1;
  for (int i = 0; i < n_item; ++i) {
    const sy11_ofdm_dec& s = item_host[i];
    SY11_REQUIRE(s.n_used >= 1 && s.n_used < FFT_SLOTS && s.n_data >= 1 && s.n_data <= s.n_used && s.car_off >= 0 && s.car_off <= n_car - s.n_data,
                 "ofdm_decide: item %d: data carriers [%d, %ld) of %d used ones are not 1 .. n_used <= %d of the table's %d", i, s.car_off, (long)s.car_off + s.n_data,
                 s.n_used, FFT_SLOTS - 1, n_car);
    SY11_REQUIRE(s.yc_off >= 0 && s.yc_off <= n_yc - s.n_used, "ofdm_decide: item %d: carrier values [%ld, %ld) leave the %ld packed ones", i, (long)s.yc_off,
                 (long)s.yc_off + s.n_used, (long)n_yc);
    SY11_REQUIRE(s.sym_off >= 0 && s.sym_off <= n_sym - s.n_data, "ofdm_decide: item %d: symbols [%ld, %ld) leave the %ld packed symbols", i, (long)s.sym_off,
                 (long)s.sym_off + s.n_data, (long)n_sym);
    SY11_REQUIRE(s.order == 2 || s.order == 4, "ofdm_decide: item %d: order %d is not 2 or 4", i, s.order);
    SY11_REQUIRE(isfinite(s.rho_r) && isfinite(s.rho_i), "ofdm_decide: item %d: rho is not finite", i);
    if (!(s.car_off == ok_off && s.n_data == ok_data && s.n_used == ok_used)) {
      for (int j = 0; j < s.n_data; ++j) {
        const sy11_ofdm_car& c = car_host[s.car_off + j];
        SY11_REQUIRE(c.idx >= 0 && c.idx < s.n_used && isfinite(c.tr) && isfinite(c.ti), "ofdm_decide: item %d: data carrier %d of its table reads value %d of %d, or its turn is not finite",
                     i, j, c.idx, s.n_used);
      }
      ok_off = s.car_off, ok_data = s.n_data, ok_used = s.n_used;
    }
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "ofdm_decide: item %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "ofdm_decide: item %d writes row %d, which an earlier item of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
    spans.push_back({s.sym_off, s.n_data, i});
  }
  const int twice = ofdm_overlap(spans);
  SY11_REQUIRE(twice < 0, "ofdm_decide: item %d writes symbols which an earlier item of this call writes", twice);
  hipLaunchKernelGGL(ofdm_decide_kernel, dim3(n_item), dim3(256), 0, (hipStream_t)stream, item, car, (const float2*)yc, (float2*)r, d, rows);
  SY11_LAUNCH_CHECK("ofdm_decide");
  return SY11_OK;
}
