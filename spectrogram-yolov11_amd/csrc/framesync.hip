// framesync.hip — find framed data in the demodulated clips: the correlation of every clip's corrected symbols with every sync word at
// every position (launch 1), the peaks of it (launch 2) and, for every peak, the word's symbol and bit errors and the packed payload bits
// (launch 3), each over all clips at once.  Between launches 2 and 3 the caller compacts the hits (one torch.nonzero, in position order).
// No reference counterpart; spec in DESIGN.md §4, plan in sy11/data/frames.py.
//
//   launch 1, per (clip, word, tile of TILE positions):  C[p] = sum_k r[p + k] conj(c[k]),  E[p] = sum_k |r[p + k]|^2,  k = 0 .. L - 1 ascending
//                                                        rho2[p] = |C|^2 / ((o / 2) L E)  (0 where E == 0),  q[p] = the quadrant of C      (f64)
//   launch 2, per the same items:                        hit[p] = rho2[p] >= threshold^2, no earlier p' within L - 1 with rho2 >= it, no later with rho2 > it
//   launch 3, per hit:                                   v[k] = r[p + k] turned back by q steps of 2 pi / o; decisions as demod_decide takes them;
//                                                        row = (errors, bit_errors, n_payload), the payload bits packed MSB first
//
//  * The word's points are un-normalised (+-1 at order 2, +-1 +- i at order 4), so every product is a sign flip and exact; the sums are
//    float64 from the stored float32 symbols, every product and sum rounded on its own (contract off), k ascending: the result is the
//    numpy definition's bit for bit, and depends neither on the tile nor on the item's place in the launch.  No atomics.
//  * Launch 1 is the hot path: L steps per position.  One position per thread, TILE = 256 positions per workgroup.  The tile's
//    TILE + L - 1 symbols are converted to float64 ONCE while they are written to LDS, as three planes (re, im and |r|^2: the term of E is a
//    property of the symbol, the same bits at whatever position reads it), next to the word's points.  Per step a lane reads three
//    doubles at consecutive addresses across the lanes (ds_read_b64, 8 bytes per lane: the 32 lanes of a half cover the 64 banks once, no
//    conflict) and two broadcast doubles, for 4 products and 5 sums in float64.  Float64 multiplies and adds issue at the float32 rate
//    here, so a step costs a wave 9 vector operations (36 cycles) against about 10 LDS cycles: the adder, not the LDS, bounds it
//    (measured: DESIGN.md §6).  Kept as products (not sign selects) so that the code reads as the definition does.
//  * Launch 2 stages the tile's rho2 with a halo of L - 1 positions on both sides in LDS; only a position at or above the threshold
//    walks its windows.  Launch 3 is one workgroup per hit; a thread packs whole bytes, so no two threads share a byte.
#include "common.h"

#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace {

constexpr int SYNC_TILE = 256;                  // positions per item of launches 1 and 2: one thread each
constexpr int SYNC_LMIN = 8, SYNC_LMAX = 256;   // symbols of a word
constexpr int SYNC_SPAN = SYNC_TILE + SYNC_LMAX - 1;
constexpr int SYNC_PAYLOAD_MAX = 1 << 20;       // payload symbols per frame, exclusive

__global__ __launch_bounds__(SYNC_TILE) void sync_correlate_kernel(const sy11_sync_item* __restrict__ items, const uint8_t* __restrict__ words,
                                                                   const float2* __restrict__ sym, double* __restrict__ rho2, uint8_t* __restrict__ q) {
#pragma clang fp contract(off)
  __shared__ double sre[SYNC_SPAN], sim[SYNC_SPAN], spw[SYNC_SPAN];
  __shared__ double wre[SYNC_LMAX], wim[SYNC_LMAX];
  const sy11_sync_item it = items[blockIdx.x];
  const int t = threadIdx.x, L = it.L, span = it.cnt + L - 1;
  const float2* src = sym + (it.sym_off + it.p0);
  for (int i = t; i < span; i += SYNC_TILE) {
    const float2 v = src[i];
    const double a = (double)v.x, b = (double)v.y;
    sre[i] = a, sim[i] = b, spw[i] = a * a + b * b;
  }
  if (t < L) {
    const int w = words[it.word_off + t];
    wre[t] = it.order == 2 ? (double)(1 - 2 * (w & 1)) : (double)(1 - 2 * ((w >> 1) & 1));
    wim[t] = it.order == 2 ? 0.0 : (double)(1 - 2 * (w & 1));
  }
  __syncthreads();
  if (t >= it.cnt) return;
  double Cr = 0.0, Ci = 0.0, E = 0.0;
  for (int k = 0; k < L; ++k) {
    const double a = sre[t + k], b = sim[t + k], cr = wre[k], ci = wim[k];
    Cr += a * cr + b * ci;
    Ci += b * cr - a * ci;
    E += spw[t + k];
  }
  const double num = Cr * Cr + Ci * Ci, den = (double)((it.order / 2) * L) * E;
  int best = 0;
  if (it.order == 2) best = Cr < 0.0;
  else {
    const double cand[4] = {Cr, Ci, -Cr, -Ci};
    double top = cand[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (cand[j] > top) top = cand[j], best = j;
  }
  const int64_t at = it.pos_off + it.p0 + t;
  rho2[at] = E == 0.0 ? 0.0 : num / den;
  q[at] = (uint8_t)best;
}

__global__ __launch_bounds__(SYNC_TILE) void sync_peaks_kernel(const sy11_sync_item* __restrict__ items, const double* __restrict__ rho2, double thr2,
                                                               uint8_t* __restrict__ hit) {
  __shared__ double w[SYNC_TILE + 2 * (SYNC_LMAX - 1)];
  const sy11_sync_item it = items[blockIdx.x];
  const int t = threadIdx.x, L = it.L;
  const int64_t P = it.n_sym - L + 1;
  const int64_t lo = it.p0 - (L - 1) > 0 ? it.p0 - (L - 1) : 0, hi = it.p0 + it.cnt + (L - 1) < P ? it.p0 + it.cnt + (L - 1) : P;
  for (int i = t; i < (int)(hi - lo); i += SYNC_TILE) w[i] = rho2[it.pos_off + lo + i];
  __syncthreads();
  if (t >= it.cnt) return;
  const int64_t p = it.p0 + t;
  const double v = w[p - lo];
  bool h = v >= thr2;                                                     // false for a NaN, which also loses every comparison below
  if (h) {
    const int64_t a = p - (L - 1) > lo ? p - (L - 1) : lo, b = p + (L - 1) < hi - 1 ? p + (L - 1) : hi - 1;
    for (int64_t j = a; j < p && h; ++j) h = !(w[j - lo] >= v);
    for (int64_t j = p + 1; j <= b && h; ++j) h = !(w[j - lo] > v);
  }
  hit[it.pos_off + p] = (uint8_t)h;
}

// r turned back by q steps of 2 pi / order -> the decision the demodulator takes of it (exact: negations and swaps)
__device__ __forceinline__ int sync_decide(float2 r, int q, int order) {
  float re = r.x, im = r.y;
  if (order == 2) return (q ? -re : re) < 0.0f;
  if (q == 1) { const float a = re; re = im, im = -a; }
  else if (q == 2) re = -re, im = -im;
  else if (q == 3) { const float a = re; re = -im, im = a; }
  return 2 * (re < 0.0f) + (im < 0.0f);
}

__global__ __launch_bounds__(256) void sync_frames_kernel(const sy11_sync_frame* __restrict__ frames, const uint8_t* __restrict__ words,
                                                          const float2* __restrict__ sym, int32_t* __restrict__ rows, int64_t stride,
                                                          uint8_t* __restrict__ bits) {
  __shared__ int sh[2][4];
  const sy11_sync_frame f = frames[blockIdx.x];
  const int t = threadIdx.x, L = f.L, order = f.order;
  const int64_t room = f.n_sym - f.p - L;
  const int n_pay = (int)(f.payload < room ? f.payload : room);
  const float2* src = sym + (f.sym_off + f.p);
  int e = 0, be = 0;
  if (t < L) {
    const int d = sync_decide(src[t], f.q, order), w = words[f.word_off + t] & (order == 2 ? 1 : 3);
    e = d != w, be = __popc(d ^ w);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) e += __shfl_xor(e, d), be += __shfl_xor(be, d);
  if ((t & 63) == 0) sh[0][t >> 6] = e, sh[1][t >> 6] = be;
  __syncthreads();
  if (t == 0) {
    int32_t* o = rows + (int64_t)f.row * 3;
    o[0] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3], o[1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3], o[2] = n_pay;
  }
  const int per = order == 2 ? 8 : 4, width = order == 2 ? 1 : 2;         // symbols per byte, bits per symbol
  uint8_t* dst = bits + (int64_t)f.row * stride;
  for (int64_t b = t; b < stride; b += 256) {
    int byte = 0;
    for (int j = 0; j < per; ++j) {
      const int64_t s = b * per + j;
      if (s < n_pay) byte |= sync_decide(src[L + s], f.q, order) << (8 - width * (j + 1));
    }
    dst[b] = (uint8_t)byte;
  }
}

// the checks launches 1 and 2 share: no item reads outside sym[] / words[] or touches a position outside [0, n_pos), and no position is
// touched by two items
int sync_check_items(const char* what, int32_t n_item, const sy11_sync_item* item_host, int64_t n_sym, int64_t n_word, int64_t n_pos) {
  std::vector<std::pair<int64_t, int>> first((size_t)n_item);
  for (int i = 0; i < n_item; ++i) {
    const sy11_sync_item& s = item_host[i];
    SY11_REQUIRE(s.order == 2 || s.order == 4, "%s: item %d: order %d is not 2 or 4", what, i, s.order);
    SY11_REQUIRE(s.sym_off >= 0 && s.n_sym >= 1 && s.n_sym <= n_sym && s.sym_off <= n_sym - s.n_sym, "%s: item %d: the clip [%ld, %ld) leaves the %ld packed symbols", what, i,
                 (long)s.sym_off, (long)s.sym_off + s.n_sym, (long)n_sym);
    SY11_REQUIRE(s.L >= SYNC_LMIN && s.L <= SYNC_LMAX && s.L <= s.n_sym, "%s: item %d: a word of %d symbols is not %d .. %d of a clip of %ld", what, i, s.L, SYNC_LMIN,
                 SYNC_LMAX, (long)s.n_sym);
    SY11_REQUIRE(s.word_off >= 0 && s.word_off <= n_word - s.L, "%s: item %d: the word [%ld, %ld) leaves the %ld packed word symbols", what, i, (long)s.word_off,
                 (long)s.word_off + s.L, (long)n_word);
    const int64_t P = s.n_sym - s.L + 1;
    SY11_REQUIRE(s.p0 >= 0 && s.p0 % SYNC_TILE == 0 && s.cnt >= 1 && s.cnt <= SYNC_TILE && s.p0 <= P - s.cnt && (s.cnt == SYNC_TILE || s.p0 + s.cnt == P),
                 "%s: item %d: positions [%ld, %ld) are not a tile of [0, %ld)", what, i, (long)s.p0, (long)s.p0 + s.cnt, (long)P);
    SY11_REQUIRE(s.pos_off >= 0 && s.pos_off <= n_pos - P, "%s: item %d: positions [%ld, %ld) leave the %ld packed positions", what, i, (long)s.pos_off, (long)s.pos_off + P,
                 (long)n_pos);
    first[(size_t)i] = {s.pos_off + s.p0, i};
  }
  std::sort(first.begin(), first.end());
  for (int i = 1; i < n_item; ++i) {
    const sy11_sync_item& a = item_host[first[(size_t)i - 1].second];
    SY11_REQUIRE(a.pos_off + a.p0 + a.cnt <= first[(size_t)i].first, "%s: item %d writes position %ld, which item %d of this call writes", what, first[(size_t)i].second,
                 (long)first[(size_t)i].first, first[(size_t)i - 1].second);
  }
  return SY11_OK;
}

}  // namespace

extern "C" int32_t sy11_sync_tile(void) { return SYNC_TILE; }

extern "C" int sy11_sync_correlate(int32_t n_item, const sy11_sync_item* item_host, const sy11_sync_item* item, int64_t n_word, const uint8_t* words,
                                   int64_t n_sym, const float* sym, int64_t n_pos, double* rho2, uint8_t* q, void* stream) {
  SY11_REQUIRE(item_host && item && words && sym && rho2 && q, "sync_correlate: null item table / words / symbols / rho2 / q");
  SY11_REQUIRE(n_item > 0 && n_word > 0 && n_word < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_pos > 0 && n_pos < (1LL << 31),
               "sync_correlate: need items, word symbols, symbols and positions, each below 2^31 (n_item=%d n_word=%ld n_sym=%ld n_pos=%ld)", n_item, (long)n_word,
               (long)n_sym, (long)n_pos);
  SY11_REQUIRE((((uintptr_t)sym | (uintptr_t)item | (uintptr_t)rho2) & 7) == 0, "sync_correlate: symbols / item table / rho2 must be 8-byte aligned");
  const int rc = sync_check_items("sync_correlate", n_item, item_host, n_sym, n_word, n_pos);
  if (rc != SY11_OK) return rc;
  hipLaunchKernelGGL(sync_correlate_kernel, dim3(n_item), dim3(SYNC_TILE), 0, (hipStream_t)stream, item, words, (const float2*)sym, rho2, q);
  SY11_LAUNCH_CHECK("sync_correlate");
  return SY11_OK;
}

extern "C" int sy11_sync_peaks(int32_t n_item, const sy11_sync_item* item_host, const sy11_sync_item* item, int64_t n_word, int64_t n_sym, int64_t n_pos,
                               const double* rho2, double threshold2, uint8_t* hit, void* stream) {
  SY11_REQUIRE(item_host && item && rho2 && hit, "sync_peaks: null item table / rho2 / hit");
  SY11_REQUIRE(n_item > 0 && n_word > 0 && n_word < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_pos > 0 && n_pos < (1LL << 31),
               "sync_peaks: need items, word symbols, symbols and positions, each below 2^31 (n_item=%d n_word=%ld n_sym=%ld n_pos=%ld)", n_item, (long)n_word, (long)n_sym,
               (long)n_pos);
  SY11_REQUIRE((((uintptr_t)item | (uintptr_t)rho2) & 7) == 0, "sync_peaks: item table / rho2 must be 8-byte aligned");
  SY11_REQUIRE(threshold2 > 0.0 && threshold2 <= 1.0, "sync_peaks: the squared threshold %g is not in (0, 1]", threshold2);
  const int rc = sync_check_items("sync_peaks", n_item, item_host, n_sym, n_word, n_pos);
  if (rc != SY11_OK) return rc;
  hipLaunchKernelGGL(sync_peaks_kernel, dim3(n_item), dim3(SYNC_TILE), 0, (hipStream_t)stream, item, rho2, threshold2, hit);
  SY11_LAUNCH_CHECK("sync_peaks");
  return SY11_OK;
}

extern "C" int sy11_sync_frames(int32_t n_frame, const sy11_sync_frame* frame_host, const sy11_sync_frame* frame, int64_t n_word, const uint8_t* words,
                                int64_t n_sym, const float* sym, int64_t n_rows, int32_t* rows, int64_t stride, uint8_t* bits, void* stream) {
  SY11_REQUIRE(frame_host && frame && words && sym && rows && (bits || stride == 0), "sync_frames: null frame table / words / symbols / rows / bits");
  SY11_REQUIRE(n_frame > 0 && n_word > 0 && n_word < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31) && stride >= 0 &&
                   stride <= SYNC_PAYLOAD_MAX / 4,
               "sync_frames: need frames, word symbols, symbols and rows, each below 2^31, and 0 .. %d bytes per row (n_frame=%d n_word=%ld n_sym=%ld n_rows=%ld stride=%ld)",
               SYNC_PAYLOAD_MAX / 4, n_frame, (long)n_word, (long)n_sym, (long)n_rows, (long)stride);
  SY11_REQUIRE((((uintptr_t)sym | (uintptr_t)frame) & 7) == 0 && ((uintptr_t)rows & 3) == 0, "sync_frames: symbols / frame table must be 8-byte aligned, the rows 4-byte");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_frame; ++i) {
    const sy11_sync_frame& s = frame_host[i];
    SY11_REQUIRE(s.order == 2 || s.order == 4, "sync_frames: frame %d: order %d is not 2 or 4", i, s.order);
    SY11_REQUIRE(s.q >= 0 && s.q < s.order, "sync_frames: frame %d: rotation %d is not below the order %d", i, s.q, s.order);
    SY11_REQUIRE(s.sym_off >= 0 && s.n_sym >= 1 && s.n_sym <= n_sym && s.sym_off <= n_sym - s.n_sym, "sync_frames: frame %d: the clip [%ld, %ld) leaves the %ld packed symbols", i,
                 (long)s.sym_off, (long)s.sym_off + s.n_sym, (long)n_sym);
    SY11_REQUIRE(s.L >= SYNC_LMIN && s.L <= SYNC_LMAX && s.L <= s.n_sym, "sync_frames: frame %d: a word of %d symbols is not %d .. %d of a clip of %ld", i, s.L, SYNC_LMIN,
                 SYNC_LMAX, (long)s.n_sym);
    SY11_REQUIRE(s.word_off >= 0 && s.word_off <= n_word - s.L, "sync_frames: frame %d: the word [%ld, %ld) leaves the %ld packed word symbols", i, (long)s.word_off,
                 (long)s.word_off + s.L, (long)n_word);
    SY11_REQUIRE(s.p >= 0 && s.p <= s.n_sym - s.L, "sync_frames: frame %d: the word at position %ld ends after the clip's %ld symbols", i, (long)s.p, (long)s.n_sym);
    SY11_REQUIRE(s.payload >= 0 && s.payload < SYNC_PAYLOAD_MAX && ((int64_t)s.payload * (s.order / 2) + 7) / 8 <= stride,
                 "sync_frames: frame %d: the bits of %d payload symbols leave the %ld bytes of a row", i, s.payload, (long)stride);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "sync_frames: frame %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "sync_frames: frame %d writes row %d, which an earlier frame of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(sync_frames_kernel, dim3(n_frame), dim3(256), 0, (hipStream_t)stream, frame, words, (const float2*)sym, rows, stride, bits);
  SY11_LAUNCH_CHECK("sync_frames");
  return SY11_OK;
}
