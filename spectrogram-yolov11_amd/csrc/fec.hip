// fec.hip — decode the frames the frame search found: soft bits of every frame's payload symbols, depunctured (launch 1), the Viterbi decoder of
// the rate 1/2, K = 7 convolutional code (launch 2) and, for every decoded frame, the re-encoded channel error count, the de-whitened information
// bits and their CRC (launch 3), each over all frames at once.  No reference counterpart; spec in DESIGN.md §4, plan in sy11/data/decode.py.
//
//   launch 1, per frame:  y[j] = the next received soft bit where the puncture pattern has a 1 at mother position j, else 0, j in [0, 2T);
//                         received bit m = component m % w of symbol m / w turned back by q steps, clamp(rintf(x * scale), -127, 127), NaN -> 0
//   launch 2, per frame:  PM(0) = 0, PM(s != 0) = -2^30;  per step t and next state s':  R_b = (s' << 1) | b,  bm_b = sum_j (1 - 2 parity(R_b & g_j)) y[2t+j],
//                         m_b = PM(R_b & 63) + bm_b,  d_t(s') = m_1 > m_0,  PM'(s') = max(m_0, m_1);  traceback from state 0 (tail) or the best state
//   launch 3, per frame:  c^ = the decided bits encoded again;  n_channel = #{y != 0},  channel_errors = #{y != 0 and (y < 0) != c^};
//                         v = u^ ^ whiten;  crc_calc over the bits before the last `width`, crc_recv = those last bits
//
//  * Everything after the quantiser of launch 1 is integer arithmetic: the results are the numpy definition's bit for bit, and depend neither
//    on the frame's place in the launch nor on the other frames of it.  The quantiser is ONE float32 multiplication and rintf: there is no
//    sum that the product could be fused with, so this file needs no contraction setting of its own.  No atomics.
//  * Launch 2 is the hot path: the code has 64 states and a wavefront 64 lanes, so ONE WAVE IS ONE DECODER, lane = next state s'.  Its two
//    predecessors are lanes (2 s') & 63 and that + 1: two ds_bpermute reads of the path metric per step.  The two sign pairs of a lane are
//    constants.  The step's 64 decisions are one __ballot word (64-bit on a wave of 64), which lane 0 stores as 8 bytes in LDS: T steps
//    take 8 T bytes of DYNAMIC LDS, sized by the call's largest T (64 KiB at T_MAX = 8192: one wave per 64 KiB, two per CU; 20 waves per CU at
//    T = 1024).  The soft values of 64 steps are one coalesced 2-byte load per lane, issued one block ahead and handed round by v_readlane,
//    so no step of the add-compare-select loop waits on memory.
//  * The traceback is SERIAL per frame: T dependent steps.  A lane loads the survivor words of 64 steps with one ds_read_b64, the chain
//    then runs on v_readlane and shifts, without an LDS round trip per step; every lane walks the same path, and lanes 0 .. 7 write the 8
//    bytes of each 64 decided bits.
//  * Launches 1 and 3 are bandwidth-trivial: one workgroup of 256 per frame; the CRC is a serial bit loop of one thread (at most 8192 bits).  What
//    launch 3 shares with the check launches of ldpc.hip and rs.hip (the de-whitened bytes, the CRC, the result row, the CRC's refusals) is frame_check.h.
#include "common.h"
#include "frame_check.h"

#include <math.h>

#include <vector>

namespace {

constexpr int FEC_TMAX = 8192;                  // trellis steps of a frame
constexpr int FEC_K = 7, FEC_STATES = 64;

__device__ __forceinline__ int fec_parity(unsigned v) { return __popc(v) & 1; }

// component c (0: Re, 1: Im) of r turned back by q steps of 2 pi / order, exactly, as sync_decide turns it
__device__ __forceinline__ float fec_component(float2 r, int q, int order, int c) {
  float re = r.x, im = r.y;
  if (order == 2) return q ? -re : re;
  if (q == 1) { const float a = re; re = im, im = -a; }
  else if (q == 2) re = -re, im = -im;
  else if (q == 3) { const float a = re; re = -im, im = a; }
  return c ? im : re;
}

__global__ __launch_bounds__(256) void fec_soft_kernel(const sy11_fec_frame* __restrict__ frames, const float2* __restrict__ sym, uint64_t mask, int period,
                                                       int ones, int64_t stride, int8_t* __restrict__ soft) {
  const sy11_fec_frame f = frames[blockIdx.x];
  const int w = f.order == 2 ? 1 : 2;
  const float2* src = sym + f.sym_off;
  int8_t* dst = soft + (int64_t)f.row * stride;
  for (int j = threadIdx.x; j < 2 * f.T; j += 256) {
    const int full = j / period, at = j - full * period;
    int y = 0;
    if ((mask >> at) & 1) {
      const int m = full * ones + __popcll(mask & ((1ull << at) - 1ull));
      const float x = fec_component(src[m / w], f.q, f.order, m % w) * f.scale;
      const float r = rintf(x);
      y = x != x ? 0 : (r > 127.0f ? 127 : (r < -127.0f ? -127 : (int)r));
    }
    dst[j] = (int8_t)y;
  }
}

__global__ __launch_bounds__(64) void fec_viterbi_kernel(const sy11_fec_frame* __restrict__ frames, int g0, int g1, int64_t stride_soft,
                                                         const int8_t* __restrict__ soft, int64_t stride_bits, uint8_t* __restrict__ bits,
                                                         int32_t* __restrict__ out) {
  extern __shared__ uint64_t surv[];            // surv[t]: bit s' = d_t(s')
  const sy11_fec_frame f = frames[blockIdx.x];
  const int lane = threadIdx.x, T = f.T;
  const int p0 = (2 * lane) & 63, p1 = p0 | 1;
  const unsigned R0 = (unsigned)lane << 1, R1 = R0 | 1u;
  const int a00 = 1 - 2 * fec_parity(R0 & g0), a01 = 1 - 2 * fec_parity(R0 & g1);
  const int a10 = 1 - 2 * fec_parity(R1 & g0), a11 = 1 - 2 * fec_parity(R1 & g1);
  const uint16_t* y2 = (const uint16_t*)(soft + (int64_t)f.row * stride_soft);     // the pair of step t: the row starts 2-byte aligned (stride even)
  int pm = lane == 0 ? 0 : -(1 << 30);
  int next = lane < T ? (int)y2[lane] : 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int cur = next, n = T - t0 < 64 ? T - t0 : 64;
    next = t0 + 64 + lane < T ? (int)y2[t0 + 64 + lane] : 0;
    for (int i = 0; i < n; ++i) {
      const int pair = __builtin_amdgcn_readlane(cur, i);
      const int y0 = (int)(int8_t)(pair & 0xff), y1 = (int)(int8_t)((pair >> 8) & 0xff);
      const int m0 = __shfl(pm, p0) + (a00 * y0 + a01 * y1);
      const int m1 = __shfl(pm, p1) + (a10 * y0 + a11 * y1);
      const bool d = m1 > m0;
      const uint64_t word = __ballot(d);
      pm = d ? m1 : m0;
      if (lane == 0) surv[t0 + i] = word;
    }
  }
  __syncthreads();
  // the end state: 0 with a tail, else the largest final metric, the lowest state on a tie
  int best = pm, s = lane;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int ob = __shfl_xor(best, d), os = __shfl_xor(s, d);
    if (ob > best || (ob == best && os < s)) best = ob, s = os;
  }
  if (f.tail) s = 0, best = __shfl(pm, 0);
  if (lane == 0) out[2 * (int64_t)f.row] = best, out[2 * (int64_t)f.row + 1] = s;
  uint8_t* dst = bits + (int64_t)f.row * stride_bits;
  const int n_bytes = (T + 7) / 8;
  for (int t0 = (T - 1) & ~63; t0 >= 0; t0 -= 64) {
    const int n = T - t0 < 64 ? T - t0 : 64;
    const uint64_t mine = lane < n ? surv[t0 + lane] : 0ull;
    const int lo = (int)(uint32_t)mine, hi = (int)(uint32_t)(mine >> 32);
    uint64_t u = 0;                             // bit 63 - i: the decided bit of step t0 + i
    for (int i = n - 1; i >= 0; --i) {
      const unsigned wlo = (unsigned)__builtin_amdgcn_readlane(lo, i), whi = (unsigned)__builtin_amdgcn_readlane(hi, i);
      const unsigned d = ((s < 32 ? wlo : whi) >> (s & 31)) & 1u;
      u |= (uint64_t)(s >> 5) << (63 - i);
      s = ((s << 1) | (int)d) & 63;
    }
    if (lane < 8 && t0 / 8 + lane < n_bytes) dst[t0 / 8 + lane] = (uint8_t)(u >> (56 - 8 * lane));
  }
  for (int64_t b = n_bytes + lane; b < stride_bits; b += 64) dst[b] = 0;
}

__global__ __launch_bounds__(256) void fec_check_kernel(const sy11_fec_frame* __restrict__ frames, int g0, int g1, int n_info, const uint8_t* __restrict__ whiten,
                                                        sy11_fec_crc crc, int64_t stride_soft, const int8_t* __restrict__ soft, int64_t stride_bits,
                                                        const uint8_t* __restrict__ bits, int64_t stride_data, uint8_t* __restrict__ data,
                                                        int32_t* __restrict__ rows) {
  __shared__ uint8_t ub[FEC_TMAX / 8], vb[FEC_TMAX / 8];
  __shared__ int sh[2][4];
  const sy11_fec_frame f = frames[blockIdx.x];
  const int t = threadIdx.x, T = f.T, n_bytes = (T + 7) / 8;
  const uint8_t* src = bits + (int64_t)f.row * stride_bits;
  for (int b = t; b < n_bytes; b += 256) ub[b] = src[b];
  __syncthreads();
  // the decided bits encoded again, from state 0: R of step k holds u_k at bit 6 down to u_(k - 6) at bit 0
  const int8_t* y = soft + (int64_t)f.row * stride_soft;
  int n_ch = 0, n_err = 0;
  for (int k = t; k < T; k += 256) {
    unsigned R = 0;
#pragma unroll
    for (int i = 0; i < FEC_K; ++i) {
      const int at = k - i;
      if (at >= 0) R |= (unsigned)((ub[at >> 3] >> (7 - (at & 7))) & 1) << (6 - i);
    }
    const int y0 = y[2 * k], y1 = y[2 * k + 1];
    n_ch += (y0 != 0) + (y1 != 0);
    n_err += (y0 != 0 && (y0 < 0) != fec_parity(R & g0)) + (y1 != 0 && (y1 < 0) != fec_parity(R & g1));
  }
  frame_count_reduce(n_ch, n_err, sh, t);
  frame_dewhiten_pack(ub, n_info, whiten, stride_data, data + (int64_t)f.row * stride_data, vb, t);
  __syncthreads();
  if (t != 0) return;
  uint32_t calc, recv;
  const int ok = frame_crc_bits(vb, n_info, crc, &calc, &recv);
  frame_row_write(rows + (int64_t)f.row * 5, calc, recv, ok, sh);
}

bool fec_poly_ok(int32_t g) { return g >= 0 && g < 128 && (g & 0x41) == 0x41; }

// the checks the three launches share: order, rotation, T against the tail, the row inside the tables and written once -> the largest T
int fec_check_frames(const char* what, int32_t n_frame, const sy11_fec_frame* frame_host, int64_t n_rows, int32_t* t_max) {
  std::vector<bool> seen((size_t)n_rows, false);
  int32_t top = 0;
  for (int i = 0; i < n_frame; ++i) {
    const sy11_fec_frame& s = frame_host[i];
    SY11_REQUIRE(s.order == 2 || s.order == 4, "%s: frame %d: order %d is not 2 or 4", what, i, s.order);
    SY11_REQUIRE(s.q >= 0 && s.q < s.order, "%s: frame %d: rotation %d is not below the order %d", what, i, s.q, s.order);
    SY11_REQUIRE(s.tail == 0 || s.tail == 1, "%s: frame %d: tail %d is not 0 or 1", what, i, s.tail);
    SY11_REQUIRE(s.T >= (s.tail ? FEC_K : 1) && s.T <= FEC_TMAX, "%s: frame %d: %d trellis steps are not %d .. %d", what, i, s.T, s.tail ? FEC_K : 1, FEC_TMAX);
    SY11_REQUIRE(s.row >= 0 && s.row < n_rows, "%s: frame %d writes row %d of a table of %ld rows", what, i, s.row, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)s.row], "%s: frame %d writes row %d, which an earlier frame of this call writes", what, i, s.row);
    seen[(size_t)s.row] = true;
    top = s.T > top ? s.T : top;
  }
  *t_max = top;
  return SY11_OK;
}

}  // namespace

extern "C" int32_t sy11_fec_tmax(void) { return FEC_TMAX; }

extern "C" int sy11_fec_soft(int32_t n_frame, const sy11_fec_frame* frame_host, const sy11_fec_frame* frame, int32_t period, uint64_t pattern, int64_t n_sym,
                             const float* sym, int64_t n_rows, int64_t stride, int8_t* soft, void* stream) {
  SY11_REQUIRE(frame_host && frame && sym && soft, "fec_soft: null frame table / symbols / soft");
  SY11_REQUIRE(n_frame > 0 && n_sym > 0 && n_sym < (1LL << 31) && n_rows > 0 && n_rows < (1LL << 31) && stride >= 2 && stride <= 2 * FEC_TMAX && stride % 2 == 0,
               "fec_soft: need frames, symbols and rows, each below 2^31, and an even 2 .. %d bytes per row (n_frame=%d n_sym=%ld n_rows=%ld stride=%ld)", 2 * FEC_TMAX, n_frame,
               (long)n_sym, (long)n_rows, (long)stride);
  SY11_REQUIRE((((uintptr_t)sym | (uintptr_t)frame) & 7) == 0 && ((uintptr_t)soft & 1) == 0, "fec_soft: symbols / frame table must be 8-byte aligned, soft 2-byte");
  SY11_REQUIRE(period >= 2 && period <= 64 && period % 2 == 0, "fec_soft: the pattern's period %d is not even and in [2, 64]", period);
  const uint64_t live = period == 64 ? ~0ull : (1ull << period) - 1ull;
  SY11_REQUIRE((pattern & live) != 0 && (pattern & ~live) == 0, "fec_soft: the pattern 0x%llx holds no 1 among, or a 1 beyond, its %d positions", (unsigned long long)pattern, period);
  const int ones = __builtin_popcountll(pattern);
  int32_t t_max = 0;
  const int rc = fec_check_frames("fec_soft", n_frame, frame_host, n_rows, &t_max);
  if (rc != SY11_OK) return rc;
  for (int i = 0; i < n_frame; ++i) {
    const sy11_fec_frame& s = frame_host[i];
    const int64_t full = 2 * (int64_t)s.T / period, rest = 2 * (int64_t)s.T % period;
    const int64_t n_coded = full * ones + __builtin_popcountll(pattern & ((1ull << rest) - 1ull)), w = s.order / 2, need = (n_coded + w - 1) / w;
    SY11_REQUIRE(s.sym_off >= 0 && s.sym_off <= n_sym - need, "fec_soft: frame %d: the %ld payload symbols at %ld leave the %ld packed symbols", i, (long)need, (long)s.sym_off,
                 (long)n_sym);
    SY11_REQUIRE(2 * (int64_t)s.T <= stride, "fec_soft: frame %d: the soft bits of %d steps leave the %ld bytes of a row", i, s.T, (long)stride);
    SY11_REQUIRE(isfinite(s.scale) && s.scale > 0.0f, "fec_soft: frame %d: the scale %g is not finite and above 0", i, (double)s.scale);
  }
  hipLaunchKernelGGL(fec_soft_kernel, dim3(n_frame), dim3(256), 0, (hipStream_t)stream, frame, (const float2*)sym, pattern, period, ones, stride, soft);
  SY11_LAUNCH_CHECK("fec_soft");
  return SY11_OK;
}

extern "C" int sy11_fec_viterbi(int32_t n_frame, const sy11_fec_frame* frame_host, const sy11_fec_frame* frame, int32_t g0, int32_t g1, int64_t n_rows,
                                int64_t stride_soft, const int8_t* soft, int64_t stride_bits, uint8_t* bits, int32_t* out, void* stream) {
  SY11_REQUIRE(frame_host && frame && soft && bits && out, "fec_viterbi: null frame table / soft / bits / out");
  SY11_REQUIRE(n_frame > 0 && n_rows > 0 && n_rows < (1LL << 31) && stride_soft >= 2 && stride_soft <= 2 * FEC_TMAX && stride_soft % 2 == 0 && stride_bits >= 1 &&
                   stride_bits <= FEC_TMAX / 8,
               "fec_viterbi: need frames, rows below 2^31, an even 2 .. %d soft bytes and 1 .. %d bit bytes per row (n_frame=%d n_rows=%ld stride_soft=%ld stride_bits=%ld)",
               2 * FEC_TMAX, FEC_TMAX / 8, n_frame, (long)n_rows, (long)stride_soft, (long)stride_bits);
  SY11_REQUIRE(((uintptr_t)frame & 7) == 0 && ((uintptr_t)soft & 1) == 0 && ((uintptr_t)out & 3) == 0, "fec_viterbi: the frame table must be 8-byte aligned, soft 2-byte, out 4-byte");
  SY11_REQUIRE(fec_poly_ok(g0) && fec_poly_ok(g1), "fec_viterbi: the generators 0%o, 0%o are not 7-bit with bits 6 and 0 set", g0, g1);
  int32_t t_max = 0;
  const int rc = fec_check_frames("fec_viterbi", n_frame, frame_host, n_rows, &t_max);
  if (rc != SY11_OK) return rc;
  for (int i = 0; i < n_frame; ++i) {
    const sy11_fec_frame& s = frame_host[i];
    SY11_REQUIRE(2 * (int64_t)s.T <= stride_soft && (s.T + 7) / 8 <= stride_bits, "fec_viterbi: frame %d: %d steps leave a row of %ld soft bytes or %ld bit bytes", i, s.T,
                 (long)stride_soft, (long)stride_bits);
  }
  hipLaunchKernelGGL(fec_viterbi_kernel, dim3(n_frame), dim3(FEC_STATES), (size_t)t_max * sizeof(uint64_t), (hipStream_t)stream, frame, (int)g0, (int)g1, stride_soft, soft,
                     stride_bits, bits, out);
  SY11_LAUNCH_CHECK("fec_viterbi");
  return SY11_OK;
}

extern "C" int sy11_fec_check(int32_t n_frame, const sy11_fec_frame* frame_host, const sy11_fec_frame* frame, int32_t g0, int32_t g1, int32_t n_info,
                              const uint8_t* whiten, const sy11_fec_crc* crc, int64_t n_rows, int64_t stride_soft, const int8_t* soft, int64_t stride_bits,
                              const uint8_t* bits, int64_t stride_data, uint8_t* data, int32_t* rows, void* stream) {
  SY11_REQUIRE(frame_host && frame && crc && soft && bits && data && rows, "fec_check: null frame table / crc / soft / bits / data / rows");
  SY11_REQUIRE(n_frame > 0 && n_rows > 0 && n_rows < (1LL << 31) && stride_soft >= 2 && stride_soft <= 2 * FEC_TMAX && stride_bits >= 1 && stride_bits <= FEC_TMAX / 8 &&
                   stride_data >= 1 && stride_data <= FEC_TMAX / 8,
               "fec_check: need frames, rows below 2^31, 2 .. %d soft bytes and 1 .. %d bit and data bytes per row (n_frame=%d n_rows=%ld strides %ld / %ld / %ld)", 2 * FEC_TMAX,
               FEC_TMAX / 8, n_frame, (long)n_rows, (long)stride_soft, (long)stride_bits, (long)stride_data);
  SY11_REQUIRE(((uintptr_t)frame & 7) == 0 && ((uintptr_t)rows & 3) == 0, "fec_check: the frame table must be 8-byte aligned, the rows 4-byte");
  SY11_REQUIRE(fec_poly_ok(g0) && fec_poly_ok(g1), "fec_check: the generators 0%o, 0%o are not 7-bit with bits 6 and 0 set", g0, g1);
  SY11_REQUIRE(n_info >= 1 && n_info <= FEC_TMAX && (n_info + 7) / 8 <= stride_data, "fec_check: %d information bits are not 1 .. %d or leave the %ld bytes of a data row", n_info,
               FEC_TMAX, (long)stride_data);
  int rc = frame_crc_refused("fec_check", crc, n_info, false);
  if (rc != SY11_OK) return rc;
  int32_t t_max = 0;
  rc = fec_check_frames("fec_check", n_frame, frame_host, n_rows, &t_max);
  if (rc != SY11_OK) return rc;
  for (int i = 0; i < n_frame; ++i) {
    const sy11_fec_frame& s = frame_host[i];
    SY11_REQUIRE(s.T == n_info + (s.tail ? FEC_K - 1 : 0), "fec_check: frame %d: %d steps are not the %d information bits%s", i, s.T, n_info, s.tail ? " and a tail of 6" : "");
    SY11_REQUIRE(2 * (int64_t)s.T <= stride_soft && (s.T + 7) / 8 <= stride_bits, "fec_check: frame %d: %d steps leave a row of %ld soft bytes or %ld bit bytes", i, s.T,
                 (long)stride_soft, (long)stride_bits);
  }
  hipLaunchKernelGGL(fec_check_kernel, dim3(n_frame), dim3(256), 0, (hipStream_t)stream, frame, (int)g0, (int)g1, (int)n_info, whiten, *crc, stride_soft, soft, stride_bits, bits,
                     stride_data, data, rows);
  SY11_LAUNCH_CHECK("fec_check");
  return SY11_OK;
}
