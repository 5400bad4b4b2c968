// equalize.hip — the sync-word least-squares equaliser of the frames the frame search found: per frame the taps of a symbol-spaced FIR
// that maps the received word onto the word as sent (launch 1, sy11_eq_solve), and that FIR over every symbol the frame owns (launch 2,
// sy11_eq_apply), each over all frames / all clips at once.  Feed-forward: no state runs along a clip.
// No reference counterpart; spec in DESIGN.md §4, plan in sy11/data/equalize.py.
//
//   launch 1, per frame:            u_k[j] = r[p + k + D - j], j = 0 .. N - 1, D = (N - 1) / 2, r = 0 outside the clip;  t[k] = A point(word[k]) turned
//                                   FORWARD by q steps (k < L), A point(decision[p + k]) (L <= k < Lt)
//                                   R = sum_k conj(u_k) u_k^T,  z = sum_k conj(u_k) t[k],  k ascending;  R += reg (tr R / N) I;  R = G G^H;  w = R^-1 z      (f64)
//                                   row = (mse_before, mse_after, pivot_min, ok);  a pivot that is not finite and positive: ok = 0, w = the unit impulse
//   launch 2, per (segment, tile):  e[m] = f32(sum_j w[j] r[m + D - j]), j ascending, for a segment with an owner;  e[m] = r[m] bit for bit without;
//                                   d[m] = the decision of e[m] as demod_decide takes it
//
//  * Launch 1 is one wavefront per frame.  The 120 entries of the lower triangle of R and the 15 of z are spread over the 64 lanes, at
//    most 3 to a lane; the training symbols go through LDS in chunks of 256, converted to float64 once; every lane adds its entries for
//    k = 0, 1, ... in that order, so a sum depends neither on the launch's grouping nor on the frame's place in it.  The Cholesky runs
//    column by column across the lanes from R, z and G in LDS (15 x 15 complex doubles: 3.6 KB); lane 0 does the two substitutions; the
//    mse sums are taken by wave reduction.  Per frame Lt steps of up to 3 entries of 4 products and 4 sums in a lane, each step behind
//    four LDS reads, then about N^2 dependent steps of one lane: a chain of latencies, not a rate.  With one frame per clip of a thousand
//    symbols it takes as long as launch 2 or longer (measured: DESIGN.md §6); it grows with Lt and with N^2, not with the payload.
//  * Launch 2 is the hot path: total symbols x N complex multiply-adds in float64.  One output symbol per thread, TILE = 256 symbols per
//    workgroup.  The tile's TILE + 2 D symbols are converted to float64 ONCE while they are written to LDS as two planes, as
//    sync_correlate_kernel does it; the owner's taps are two broadcast doubles per step.  Per step a lane reads two doubles at consecutive
//    addresses across the lanes (ds_read_b64: no bank conflict) for 4 products and 4 sums, every one rounded on its own (contract off): 8 N
//    vector operations per symbol against 17 bytes of memory traffic (8 in, 8 + 1 out).  At N = 15 that is 7 operations per byte, below
//    what the adder sustains per byte of HBM bandwidth, so by the counts the memory bounds it at every N.  Measured on 4.3 million symbols
//     it reaches 2.3 TB/s at N = 7 and 1.8 TB/s and 13 T operations/s at N = 15, a third of the bandwidth a plain copy
//    reaches: a workgroup lives for one load, one barrier, N steps and one store of 256 symbols, so what bounds it is the latency of that
//    chain over the workgroups in flight, not a rate.  More symbols per thread would hide it; the host's checks of the item table cost
//    more than the kernel at that size, so that is where time would be won first.  No two items write the same symbol; no atomics.
#include "common.h"

#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace {

constexpr int EQ_TILE = 256;                    // symbols per item of launch 2: one thread each
constexpr int EQ_NMIN = 3, EQ_NMAX = 15;        // taps, odd
constexpr int EQ_LMAX = 256;                    // symbols of a word (the frame search's)
constexpr int EQ_LTMAX = 4096;                  // training symbols of a frame
constexpr int EQ_CHUNK = 256;                   // training symbols per pass through LDS
constexpr int EQ_TRI = EQ_NMAX * (EQ_NMAX + 1) / 2;
constexpr int EQ_WSTRIDE = 2 * EQ_NMAX;         // doubles per row of w

// the decision demod_decide takes of a symbol
__device__ __forceinline__ int eq_decide(float re, float im, int order) { return order == 2 ? (int)(re < 0.0f) : 2 * (int)(re < 0.0f) + (int)(im < 0.0f); }

__global__ __launch_bounds__(64) void eq_solve_kernel(const sy11_eq_frame* __restrict__ frames, int N, double reg, const uint8_t* __restrict__ words,
                                                      const float2* __restrict__ sym, const uint8_t* __restrict__ dec, double* __restrict__ w,
                                                      double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sre[EQ_CHUNK + EQ_NMAX - 1], sim[EQ_CHUNK + EQ_NMAX - 1], tre[EQ_CHUNK], tim[EQ_CHUNK];
  __shared__ double Rre[EQ_TRI], Rim[EQ_TRI], Gre[EQ_NMAX][EQ_NMAX], Gim[EQ_NMAX][EQ_NMAX];
  __shared__ double zre[EQ_NMAX], zim[EQ_NMAX], yre[EQ_NMAX], yim[EQ_NMAX], wre[EQ_NMAX], wim[EQ_NMAX];
  __shared__ double scal[2];
  const sy11_eq_frame f = frames[blockIdx.x];
  const int lane = threadIdx.x, D = (N - 1) / 2, L = f.L, Lt = f.Lt, order = f.order, q = f.q;
  const int n_tri = N * (N + 1) / 2, n_ent = n_tri + N;
  const double A = f.gain, c4 = A * (1.0 / 1.4142135623730951);
  const float2* clip = sym + f.sym_off;

  // the chunk [k0, k0 + cnt) of the training symbols: r[p + k0 - D  p + k0 + cnt + D) and the targets of its k
  auto stage = [&](int k0, int cnt) {
    for (int i = lane; i < cnt + 2 * D; i += 64) {
      const int64_t m = f.p + k0 - D + i;
      float2 v = make_float2(0.0f, 0.0f);
      if (m >= 0 && m < f.n_sym) v = clip[m];
      sre[i] = (double)v.x, sim[i] = (double)v.y;
    }
    for (int i = lane; i < cnt; i += 64) {
      const int k = k0 + i;
      double a, b;
      if (k < L) {
        const int d = words[f.word_off + k];
        if (order == 2) {
          a = (d & 1) ? -A : A, b = 0.0;
          if (q) a = -a;
        } else {
          const double cr = (d & 2) ? -c4 : c4, ci = (d & 1) ? -c4 : c4;
          a = q == 0 ? cr : q == 1 ? -ci : q == 2 ? -cr : ci;
          b = q == 0 ? ci : q == 1 ? cr : q == 2 ? -ci : -cr;
        }
      } else {
        const int d = dec[f.sym_off + f.p + k];
        if (order == 2) a = (d & 1) ? -A : A, b = 0.0;
        else a = (d & 2) ? -c4 : c4, b = (d & 1) ? -c4 : c4;
      }
      tre[i] = a, tim[i] = b;
    }
  };

  // the entries of this lane: e < n_tri is R[a][b] of the lower triangle, a >= b; the N after them are z[a]
  int ea[3], eb[3];
  double ar[3] = {0.0, 0.0, 0.0}, ai[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int e = lane + 64 * s;
    int a = 0;
    if (e < n_tri) {
      while ((a + 1) * (a + 2) / 2 <= e) ++a;
      ea[s] = a, eb[s] = e - a * (a + 1) / 2;
    } else {
      ea[s] = e < n_ent ? e - n_tri : -1, eb[s] = -1;
    }
  }
  for (int k0 = 0; k0 < Lt; k0 += EQ_CHUNK) {
    const int cnt = Lt - k0 < EQ_CHUNK ? Lt - k0 : EQ_CHUNK;
    __syncthreads();
    stage(k0, cnt);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (ea[s] < 0) continue;
      const int ia = 2 * D - ea[s], ib = 2 * D - eb[s];
      double sr = ar[s], si = ai[s];
      if (eb[s] >= 0) {
        for (int i = 0; i < cnt; ++i) {
          const double xr = sre[i + ia], xi = sim[i + ia], vr = sre[i + ib], vi = sim[i + ib];
          sr += xr * vr + xi * vi;
          si += xr * vi - xi * vr;
        }
      } else {
        for (int i = 0; i < cnt; ++i) {
          const double xr = sre[i + ia], xi = sim[i + ia], vr = tre[i], vi = tim[i];
          sr += xr * vr + xi * vi;
          si += xr * vi - xi * vr;
        }
      }
      ar[s] = sr, ai[s] = si;
    }
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int e = lane + 64 * s;
    if (e < n_tri) Rre[e] = ar[s], Rim[e] = ai[s];
    else if (e < n_ent) zre[e - n_tri] = ar[s], zim[e - n_tri] = ai[s];
  }
  __syncthreads();
  if (lane == 0) {
    double tr = 0.0;
    for (int a = 0; a < N; ++a) tr += Rre[a * (a + 1) / 2 + a];
    scal[0] = tr / (double)N;
  }
  __syncthreads();
  const double mu = scal[0];
  if (lane < N) Rre[lane * (lane + 1) / 2 + lane] += reg * mu;
  __syncthreads();
  // R = G G^H, column by column; every lane follows the pivots, lane i takes row c + 1 + i of column c
  bool ok = true;
  double pmin = INFINITY;
  for (int c = 0; c < N; ++c) {
    double d = Rre[c * (c + 1) / 2 + c];
    for (int k = 0; k < c; ++k) d -= Gre[c][k] * Gre[c][k] + Gim[c][k] * Gim[c][k];
    if (!(d > 0.0) || !(d < INFINITY)) {
      const double v = d / mu;
      pmin = v < pmin || v != v ? v : pmin;
      ok = false;
      break;
    }
    const double g = sqrt(d), v = g * g / mu;
    pmin = v < pmin ? v : pmin;
    const int a = c + 1 + lane;
    if (a < N) {
      double sr = Rre[a * (a + 1) / 2 + c], si = Rim[a * (a + 1) / 2 + c];
      for (int k = 0; k < c; ++k) {
        const double xr = Gre[a][k], xi = Gim[a][k], vr = Gre[c][k], vi = Gim[c][k];    // G[a][k] conj(G[c][k])
        sr -= xr * vr + xi * vi;
        si -= xi * vr - xr * vi;
      }
      Gre[a][c] = sr / g, Gim[a][c] = si / g;
    }
    if (lane == 0) Gre[c][c] = g, Gim[c][c] = 0.0;
    __syncthreads();
  }
  if (lane == 0) {
    if (ok) {
      for (int a = 0; a < N; ++a) {                                                     // G y = z
        double sr = zre[a], si = zim[a];
        for (int k = 0; k < a; ++k) {
          const double xr = Gre[a][k], xi = Gim[a][k], vr = yre[k], vi = yim[k];
          sr -= xr * vr - xi * vi;
          si -= xr * vi + xi * vr;
        }
        yre[a] = sr / Gre[a][a], yim[a] = si / Gre[a][a];
      }
      for (int a = N - 1; a >= 0; --a) {                                                // G^H w = y
        double sr = yre[a], si = yim[a];
        for (int k = a + 1; k < N; ++k) {
          const double xr = Gre[k][a], xi = -Gim[k][a], vr = wre[k], vi = wim[k];
          sr -= xr * vr - xi * vi;
          si -= xr * vi + xi * vr;
        }
        wre[a] = sr / Gre[a][a], wim[a] = si / Gre[a][a];
      }
      for (int a = 0; a < N; ++a) ok = ok && wre[a] - wre[a] == 0.0 && wim[a] - wim[a] == 0.0;
    }
    if (!ok)
      for (int a = 0; a < N; ++a) wre[a] = a == D ? 1.0 : 0.0, wim[a] = 0.0;
    scal[1] = ok ? 1.0 : 0.0;
  }
  __syncthreads();
  stage(0, L);
  __syncthreads();
  double eb0 = 0.0, ea0 = 0.0;
  for (int k = lane; k < L; k += 64) {
    double re = 0.0, im = 0.0;
    for (int j = 0; j < N; ++j) {
      const double wr = wre[j], wi = wim[j], a = sre[k + 2 * D - j], b = sim[k + 2 * D - j];
      re += (wr * a) - (wi * b);
      im += (wr * b) + (wi * a);
    }
    const double br = sre[k + D] - tre[k], bi = sim[k + D] - tim[k], cr = re - tre[k], ci = im - tim[k];
    eb0 += br * br + bi * bi;
    ea0 += cr * cr + ci * ci;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) eb0 += __shfl_xor(eb0, d), ea0 += __shfl_xor(ea0, d);
  double* wo = w + (int64_t)f.row * EQ_WSTRIDE;
  if (lane < EQ_NMAX) wo[2 * lane] = lane < N ? wre[lane] : 0.0, wo[2 * lane + 1] = lane < N ? wim[lane] : 0.0;
  if (lane == 0) {
    const double den = (double)L * (A * A);
    double* o = rows + (int64_t)f.row * 4;
    o[0] = eb0 / den, o[1] = ea0 / den, o[2] = pmin, o[3] = scal[1];
  }
}

__global__ __launch_bounds__(EQ_TILE) void eq_apply_kernel(const sy11_eq_item* __restrict__ items, const sy11_eq_segment* __restrict__ segs, int N,
                                                           const double* __restrict__ w, const float2* __restrict__ sym, float2* __restrict__ out,
                                                           uint8_t* __restrict__ dec) {
#pragma clang fp contract(off)
  __shared__ double sre[EQ_TILE + EQ_NMAX - 1], sim[EQ_TILE + EQ_NMAX - 1];
  __shared__ double wre[EQ_NMAX], wim[EQ_NMAX];
  const sy11_eq_item it = items[blockIdx.x];
  const sy11_eq_segment s = segs[it.seg];
  const int t = threadIdx.x, D = (N - 1) / 2;
  const int64_t m0 = s.start + (int64_t)it.tile * EQ_TILE;
  const int cnt = (int)(s.end - m0 < EQ_TILE ? s.end - m0 : EQ_TILE);
  const float2* clip = sym + s.sym_off;
  if (s.frame < 0) {                                                                    // no owner: the symbol's bits as they are
    if (t < cnt) {
      const int64_t at = s.sym_off + m0 + t;
      const uint2 bits = reinterpret_cast<const uint2*>(sym)[at];
      reinterpret_cast<uint2*>(out)[at] = bits;
      dec[at] = (uint8_t)eq_decide(__uint_as_float(bits.x), __uint_as_float(bits.y), s.order);
    }
    return;
  }
  for (int i = t; i < cnt + 2 * D; i += EQ_TILE) {
    const int64_t m = m0 - D + i;
    float2 v = make_float2(0.0f, 0.0f);
    if (m >= 0 && m < s.n_sym) v = clip[m];
    sre[i] = (double)v.x, sim[i] = (double)v.y;
  }
  if (t < N) wre[t] = w[(int64_t)s.frame * EQ_WSTRIDE + 2 * t], wim[t] = w[(int64_t)s.frame * EQ_WSTRIDE + 2 * t + 1];
  __syncthreads();
  if (t >= cnt) return;
  double re = 0.0, im = 0.0;
  for (int j = 0; j < N; ++j) {
    const double wr = wre[j], wi = wim[j], a = sre[t + 2 * D - j], b = sim[t + 2 * D - j];
    re += (wr * a) - (wi * b);
    im += (wr * b) + (wi * a);
  }
  const float fr = (float)re, fi = (float)im;
  const int64_t at = s.sym_off + m0 + t;
  out[at] = make_float2(fr, fi);
  dec[at] = (uint8_t)eq_decide(fr, fi, s.order);
}

}  // namespace

extern "C" int32_t sy11_eq_tile(void) { return EQ_TILE; }

extern "C" int sy11_eq_solve(int32_t n_frame, const sy11_eq_frame* frame_host, const sy11_eq_frame* frame, int32_t taps, double reg, int64_t n_word,
                             const uint8_t* words, int64_t n_sym, const float* sym, const uint8_t* decisions, int64_t n_rows, double* w, double* rows,
                             void* stream) {
  SY11_REQUIRE(frame_host && frame && words && sym && w && rows, "eq_solve: null frame table / words / symbols / w / rows");
  SY11_REQUIRE(n_frame > 0 && n_word > 0 && n_word < (1LL << 31) && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "eq_solve: need frames, word symbols, symbols and rows, each below 2^31 (n_frame=%d n_word=%ld n_sym=%ld n_rows=%ld)", n_frame, (long)n_word, (long)n_sym,
               (long)n_rows);
  SY11_REQUIRE(taps >= EQ_NMIN && taps <= EQ_NMAX && taps % 2 == 1, "eq_solve: %d taps are not an odd number in [%d, %d]", taps, EQ_NMIN, EQ_NMAX);
  SY11_REQUIRE(reg >= 0.0 && reg <= 1.0, "eq_solve: reg = %g is not in [0, 1]", reg);
  SY11_REQUIRE((((uintptr_t)sym | (uintptr_t)frame | (uintptr_t)w | (uintptr_t)rows) & 7) == 0, "eq_solve: symbols / frame table / w / rows must be 8-byte aligned");
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_frame; ++i) {
    const sy11_eq_frame& s = frame_host[i];
    SY11_REQUIRE(s.order == 2 || s.order == 4, "eq_solve: frame %d: order %d is not 2 or 4", i, s.order);
    SY11_REQUIRE(s.q >= 0 && s.q < s.order, "eq_solve: frame %d: rotation %d is not below the order %d", i, s.q, s.order);
    SY11_REQUIRE(s.sym_off >= 0 && s.n_sym >= 1 && s.n_sym <= n_sym && s.sym_off <= n_sym - s.n_sym, "eq_solve: frame %d: the clip [%ld, %ld) leaves the %ld packed symbols", i,
                 (long)s.sym_off, (long)s.sym_off + s.n_sym, (long)n_sym);
    SY11_REQUIRE(s.L >= 1 && s.L <= EQ_LMAX && s.Lt >= s.L && s.Lt <= EQ_LTMAX, "eq_solve: frame %d: a word of %d and %d training symbols are not 1 .. %d and word .. %d", i,
                 s.L, s.Lt, EQ_LMAX, EQ_LTMAX);
    SY11_REQUIRE(s.word_off >= 0 && s.word_off <= n_word - s.L, "eq_solve: frame %d: the word [%ld, %ld) leaves the %ld packed word symbols", i, (long)s.word_off,
                 (long)s.word_off + s.L, (long)n_word);
    SY11_REQUIRE(s.p >= 0 && s.p <= s.n_sym - s.Lt, "eq_solve: frame %d: %d training symbols at position %ld end after the clip's %ld symbols", i, s.Lt, (long)s.p,
                 (long)s.n_sym);
    SY11_REQUIRE(s.Lt == s.L || decisions, "eq_solve: frame %d trains on %d symbols beyond its word, but the decisions are null", i, s.Lt - s.L);
    SY11_REQUIRE(s.gain > 0.0 && s.gain < INFINITY, "eq_solve: frame %d: the gain %g is not finite and positive", i, s.gain);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "eq_solve: frame %d writes row %d of a table of %ld rows", i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "eq_solve: frame %d writes row %d, which an earlier frame of this call writes", i, s.row);
    seen[(size_t)s.row] = true;
  }
  hipLaunchKernelGGL(eq_solve_kernel, dim3(n_frame), dim3(64), 0, (hipStream_t)stream, frame, taps, reg, words, (const float2*)sym, decisions, w, rows);
  SY11_LAUNCH_CHECK("eq_solve");
  return SY11_OK;
}

extern "C" int sy11_eq_apply(int32_t n_item, const sy11_eq_item* item_host, const sy11_eq_item* item, int32_t n_seg, const sy11_eq_segment* seg_host,
                             const sy11_eq_segment* seg, int32_t taps, int64_t n_rows, const double* w, int64_t n_sym, const float* sym, float* out,
                             uint8_t* decisions, void* stream) {
  SY11_REQUIRE(item_host && item && seg_host && seg && w && sym && out && decisions, "eq_apply: null item table / segment table / w / symbols / out / decisions");
  SY11_REQUIRE(n_item > 0 && n_seg > 0 && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31),
               "eq_apply: need items, segments, symbols and rows of w, each below 2^31 (n_item=%d n_seg=%d n_sym=%ld n_rows=%ld)", n_item, n_seg, (long)n_sym, (long)n_rows);
  SY11_REQUIRE(taps >= EQ_NMIN && taps <= EQ_NMAX && taps % 2 == 1, "eq_apply: %d taps are not an odd number in [%d, %d]", taps, EQ_NMIN, EQ_NMAX);
  SY11_REQUIRE((((uintptr_t)sym | (uintptr_t)out | (uintptr_t)seg | (uintptr_t)w) & 7) == 0 && ((uintptr_t)item & 3) == 0,
               "eq_apply: symbols / out / segment table / w must be 8-byte aligned, the item table 4-byte");
  SY11_REQUIRE(sym != out, "eq_apply: out must not be the symbols");
  std::vector<std::pair<int64_t, int>> first((size_t)n_seg);
  for (int i = 0; i < n_seg; ++i) {
    const sy11_eq_segment& s = seg_host[i];
    SY11_REQUIRE(s.order == 2 || s.order == 4, "eq_apply: segment %d: order %d is not 2 or 4", i, s.order);
    SY11_REQUIRE(s.sym_off >= 0 && s.n_sym >= 1 && s.n_sym <= n_sym && s.sym_off <= n_sym - s.n_sym, "eq_apply: segment %d: the clip [%ld, %ld) leaves the %ld packed symbols", i,
                 (long)s.sym_off, (long)s.sym_off + s.n_sym, (long)n_sym);
    SY11_REQUIRE(s.start >= 0 && s.start < s.end && s.end <= s.n_sym, "eq_apply: segment %d: symbols [%ld, %ld) are not inside the clip's %ld", i, (long)s.start, (long)s.end,
                 (long)s.n_sym);
    SY11_REQUIRE(s.frame >= -1 && s.frame < n_rows, "eq_apply: segment %d: owner %d is not -1 or a row of the %ld of w", i, s.frame, (long)n_rows);
    first[(size_t)i] = {s.sym_off + s.start, i};
  }
  if (!std::is_sorted(first.begin(), first.end())) std::sort(first.begin(), first.end());      // the plan's tables come in order
  for (int i = 1; i < n_seg; ++i) {
    const sy11_eq_segment& a = seg_host[first[(size_t)i - 1].second];
    SY11_REQUIRE(a.sym_off + a.end <= first[(size_t)i].first, "eq_apply: segment %d writes symbol %ld, which segment %d of this call writes", first[(size_t)i].second,
                 (long)first[(size_t)i].first, first[(size_t)i - 1].second);
  }
  std::vector<std::pair<int64_t, int>> at((size_t)n_item);
  for (int i = 0; i < n_item; ++i) {
    const sy11_eq_item& t = item_host[i];
    SY11_REQUIRE(t.seg >= 0 && t.seg < n_seg, "eq_apply: item %d: segment %d is not one of the %d", i, t.seg, n_seg);
    const sy11_eq_segment& s = seg_host[t.seg];
    SY11_REQUIRE(t.tile >= 0 && (int64_t)t.tile * EQ_TILE < s.end - s.start, "eq_apply: item %d: tile %d is not one of segment %d's %ld symbols", i, t.tile, t.seg,
                 (long)(s.end - s.start));
    at[(size_t)i] = {s.sym_off + s.start + (int64_t)t.tile * EQ_TILE, i};
  }
  if (!std::is_sorted(at.begin(), at.end())) std::sort(at.begin(), at.end());
  for (int i = 1; i < n_item; ++i)
    SY11_REQUIRE(at[(size_t)i - 1].first != at[(size_t)i].first, "eq_apply: item %d writes symbol %ld, which item %d of this call writes", at[(size_t)i].second,
                 (long)at[(size_t)i].first, at[(size_t)i - 1].second);
  hipLaunchKernelGGL(eq_apply_kernel, dim3(n_item), dim3(EQ_TILE), 0, (hipStream_t)stream, item, seg, taps, w, (const float2*)sym, (float2*)out, decisions);
  SY11_LAUNCH_CHECK("eq_apply");
  return SY11_OK;
}
