// rs.hip — the outer code behind the frame decoder: de-interleave the Reed-Solomon codewords of every decoded frame and correct up to t byte
// errors in each (launch 1), then the sums of a frame and the CRC of its information bytes (launch 2), each over all frames at once.  No
// reference counterpart; spec in DESIGN.md §4, plan in sy11/data/correct.py.
//
//   field     GF(2^8) modulo `poly` (9 bits, primitive), alpha = 0x02, beta = alpha^prim
//   code      c[0 .. n), c[0] the coefficient of x^(n-1), the first k bytes the information;  S_j = sum_i c[i] beta^((fcr + j)(n - 1 - i)) = 0,  j in [0, nroots)
//   layout    byte offset + m of a frame's row, m in [0, I n), is byte m / I of codeword m % I
//   launch 1  per (frame, codeword): the codeword within t = nroots / 2 byte errors of the received word, if there is one -> its k information bytes and
//             (errors, bit_errors); else the received bytes and (-1, 0)
//   launch 2  per frame: n_failed, the sums of errors and bit_errors over the corrected codewords, crc_calc / crc_recv / crc_ok over the information bytes
//
//  * Exact integer arithmetic: the results are the definition's byte for byte and depend neither on the frame's place in the launch nor on the
//    other frames of it.  No atomics, no floating point.
//  * ONE WAVE IS ONE CODEWORD, as in fec_viterbi_kernel one wave is one frame.  A workgroup takes whole frames (4 / I of them, at least one), so its
//    threads read each frame's I n interleaved bytes as one contiguous, coalesced stretch and scatter them to the codewords' rows in LDS; after
//    the workgroup's only barrier a wave keeps its codeword in registers, 4 bytes per lane, and the rest of the decoder exchanges values between
//    lanes with shuffles and ballots alone: no LDS is written after the barrier, so no wave waits for another and none needs an LDS fence.
//  * GF multiply: log / exp tables in LDS, built per workgroup from `poly` (thread e computes alpha^e by square-and-multiply with the shift-and-reduce
//    product).  A product is then two log reads, an add and one read of the doubled exp table (no reduction modulo 255); the Horner-like loops
//    (syndromes, Chien, Forney) keep the exponent of the fixed factor in a register and step it by an add and a conditional subtract.
//  * syndromes: a lane holds 4 bytes, S_j is the wave's XOR over the lanes' terms, lane j keeps S_j.  All zero (a wave-uniform test) skips the rest.
//    Berlekamp-Massey: nroots steps, lane i holds Lambda_i and B_i, the discrepancy is a wave XOR.  Chien: 4 of the 255 positions per lane, the
//    roots as 4 ballot words.  Forney: lane r takes the r-th root.  Every branch around a wave-level operation is wave-uniform.
//  * Launch 2: one wave per frame; the CRC is the byte-serial form of frame_check.h, which also holds the refusals of a CRC and of a table of rows.
#include "common.h"
#include "frame_check.h"

namespace {

constexpr int RS_WAVE = 64;
constexpr int RS_NROOTS_MAX = 64, RS_I_MAX = 8;
constexpr int RS_ROWS = 8;                      // codewords of a workgroup at the most: 4 / I frames (at least one) of I codewords

__host__ __device__ inline unsigned rs_mul_slow(unsigned a, unsigned b, unsigned poly) {
  unsigned p = 0;
  for (int i = 0; i < 8; ++i) {
    p ^= (b & 1u) ? a : 0u;
    b >>= 1;
    a <<= 1;
    a ^= (a & 0x100u) ? poly : 0u;
  }
  return p;
}

__device__ __forceinline__ int rs_wave_xor(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ int rs_step(int e, int q) {          // (e + q) mod 255 for e, q in [0, 255)
  e += q;
  return e >= 255 ? e - 255 : e;
}

// the position of the r-th 1 of the 256 bits w[0] (bits 0 .. 63) .. w[3], r below their count
__device__ __forceinline__ int rs_nth_bit(const uint64_t* w, int r) {
  int pos = 0;
  bool found = false;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int c = __popcll(w[m]);
    if (!found) {
      if (r < c) {
        uint64_t v = w[m];
        for (int i = 0; i < r; ++i) v &= v - 1ull;
        pos = 64 * m + __ffsll((unsigned long long)v) - 1;
        found = true;
      } else {
        r -= c;
      }
    }
  }
  return pos;
}

__global__ __launch_bounds__(512) void rs_decode_kernel(const int32_t* __restrict__ frame_row, int n_frame, sy11_rs_code code, int offset, int frames_per_block,
                                                        int64_t stride_data, const uint8_t* __restrict__ data, int64_t stride_info, uint8_t* __restrict__ info,
                                                        int32_t* __restrict__ cw) {
  __shared__ uint8_t gf_exp[512], gf_log[256];
  __shared__ uint8_t rx[RS_ROWS][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = code.n, k = code.k, I = code.interleave, nroots = n - k, t = nroots / 2;
  const unsigned poly = (unsigned)code.poly;
  // alpha^e by square-and-multiply; the table twice over, so that the sum of two logarithms needs no reduction
  for (int e = tid; e < 255; e += blockDim.x) {
    unsigned v = 1, b = 2;
    for (int i = 0; i < 8; ++i) {
      if ((e >> i) & 1) v = rs_mul_slow(v, b, poly);
      b = rs_mul_slow(b, b, poly);
    }
    gf_exp[e] = (uint8_t)v, gf_exp[e + 255] = (uint8_t)v, gf_log[v] = (uint8_t)e;
  }
  if (tid == 0) gf_log[0] = 0, gf_exp[510] = 0, gf_exp[511] = 0;
  // the frames of this workgroup: I n contiguous bytes each, byte m to codeword m % I
  const int f0 = blockIdx.x * frames_per_block;
  for (int s = 0; s < frames_per_block; ++s) {
    if (f0 + s >= n_frame) break;
    const uint8_t* src = data + (int64_t)frame_row[f0 + s] * stride_data + offset;
    for (int m = tid; m < I * n; m += blockDim.x) rx[s * I + m % I][m / I] = src[m];
  }
  __syncthreads();
  const int s = wave / I, w = wave - s * I;
  if (f0 + s >= n_frame) return;                                  // a wave without a codeword (the last workgroup); no barrier follows
  const int row = frame_row[f0 + s];

  // ---- the wave's codeword: lane holds bytes i = lane + 64 m
  int c[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int i = lane + 64 * m;
    c[m] = i < n ? (int)rx[wave][i] : 0;
  }
  const int prim = code.prim, fcr = code.fcr;
  // ---- syndromes: the exponent of byte i under S_j is prim (fcr + j) (n - 1 - i) mod 255, stepped by prim (n - 1 - i) from one j to the next
  int S = 0;
  {
    int e[4], q[4], lc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = lane + 64 * m, pw = i < n ? n - 1 - i : 0;
      q[m] = (prim * pw) % 255;
      e[m] = (q[m] * fcr) % 255;
      lc[m] = gf_log[c[m]];
    }
    for (int j = 0; j < nroots; ++j) {
      int acc = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc ^= c[m] ? (int)gf_exp[lc[m] + e[m]] : 0;
        e[m] = rs_step(e[m], q[m]);
      }
      acc = rs_wave_xor(acc);
      if (lane == j) S = acc;
    }
  }
  int L = 0, bit_errors = 0, root = 0, value = 0;                 // lane r < L: the power of x its root stands for, and the error value there
  bool failed = false;
  if (__ballot(S != 0) != 0ull) {                                 // wave-uniform
    // ---- Berlekamp-Massey: lane i holds Lambda_i and B_i (B already multiplied by x for the step)
    int lam = lane == 0, B = lane == 0, b = 1;
    for (int N = 0; N < nroots; ++N) {
      const int up = __shfl_up(B, 1);
      B = lane == 0 ? 0 : up;
      const int sv = __shfl(S, (N - lane) & 63);
      int d = (lane <= L && lane <= N && lam && sv) ? (int)gf_exp[gf_log[lam] + gf_log[sv]] : 0;
      d = rs_wave_xor(d);
      if (d != 0) {                                               // wave-uniform
        const int coef = gf_log[d] + 255 - gf_log[b];             // log(d / b), below 510
        const int old = lam;
        lam ^= B ? (int)gf_exp[(coef >= 255 ? coef - 255 : coef) + gf_log[B]] : 0;
        if (2 * L <= N) L = N + 1 - L, B = old, b = d;
      }
    }
    failed = L > t;
    uint64_t roots[4] = {0ull, 0ull, 0ull, 0ull};
    if (!failed) {                                                // wave-uniform
      // ---- Chien: position p = lane + 64 m stands for x^p; Lambda has the root beta^(-p) there
      int val[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0}, q[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) q[m] = (255 - (prim * (lane + 64 * m)) % 255) % 255;
      for (int i = 0; i <= L; ++i) {
        const int li = __shfl(lam, i), ll = gf_log[li];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          val[m] ^= li ? (int)gf_exp[ll + e[m]] : 0;
          e[m] = rs_step(e[m], q[m]);
        }
      }
      int count = 0;
      bool outside = false;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int p = lane + 64 * m;
        roots[m] = __ballot(p < 255 && val[m] == 0);
        outside = outside || (p < 255 && val[m] == 0 && p >= n);   // a root among the bytes that are not transmitted
        count += __popcll(roots[m]);
      }
      failed = count != L || __ballot(outside) != 0ull;
    }
    if (!failed) {                                                // wave-uniform
      // ---- Forney: Omega_i = sum_(j <= i) S_(i - j) Lambda_j for i < L (lane i), then lane r evaluates at its root
      int omega = 0;
      for (int j = 0; j < L; ++j) {
        const int lj = __shfl(lam, j), sv = __shfl(S, (lane - j) & 63);
        omega ^= (j <= lane && lane < L && lj && sv) ? (int)gf_exp[gf_log[lj] + gf_log[sv]] : 0;
      }
      root = lane < L ? rs_nth_bit(roots, lane) : 0;
      const int lx = (prim * root) % 255, q = (255 - lx) % 255;   // log of X = beta^root and of 1 / X
      int num = 0, den = 0, e = 0, e_prev = 0;
      for (int i = 0; i <= L; ++i) {
        const int oi = __shfl(omega, i), li = __shfl(lam, i);
        if (i < L && oi) num ^= (int)gf_exp[gf_log[oi] + e];
        if ((i & 1) && li) den ^= (int)gf_exp[gf_log[li] + e_prev];   // the derivative: the odd terms, one power lower
        e_prev = e;
        e = rs_step(e, q);
      }
      if (__ballot(lane < L && (num == 0 || den == 0)) != 0ull) {    // not with L distinct roots of a shortest Lambda; a 0 must not reach the logarithms
        failed = true;
      } else {
        const int lv = (lx * ((256 - fcr) % 255)) % 255 + gf_log[num] + 255 - gf_log[den];          // X^(1 - fcr) Omega(1 / X) / Lambda'(1 / X)
        value = lane < L ? (int)gf_exp[lv % 255] : 0;
        int bits = __popc((unsigned)value);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) bits += __shfl_xor(bits, d);
        bit_errors = bits;
      }
    }
  }
  const int n_fix = failed ? 0 : L;
  // ---- the k information bytes, corrected, codeword-major
  uint8_t* dst = info + (int64_t)row * stride_info + (int64_t)w * k;
  for (int r = 0; r < n_fix; ++r) {
    const int at = n - 1 - __shfl(root, r), ev = __shfl(value, r);
#pragma unroll
    for (int m = 0; m < 4; ++m) c[m] ^= (lane + 64 * m == at) ? ev : 0;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int i = lane + 64 * m;
    if (i < k) dst[i] = (uint8_t)c[m];
  }
  if (lane < 2) cw[((int64_t)row * I + w) * 2 + lane] = lane == 0 ? (failed ? -1 : L) : (failed ? 0 : bit_errors);
}

__global__ __launch_bounds__(64) void rs_check_kernel(const int32_t* __restrict__ frame_row, int I, int k, sy11_fec_crc crc, int64_t stride_info,
                                                      const uint8_t* __restrict__ info, const int32_t* __restrict__ cw, int32_t* __restrict__ rows) {
  __shared__ uint8_t vb[RS_I_MAX * 255];
  const int row = frame_row[blockIdx.x], lane = threadIdx.x, n_bytes = I * k;
  const uint8_t* src = info + (int64_t)row * stride_info;
  for (int b = lane; b < n_bytes; b += 64) vb[b] = src[b];
  int n_failed = 0, n_err = 0, n_bit = 0;
  if (lane < I) {
    const int e = cw[((int64_t)row * I + lane) * 2], be = cw[((int64_t)row * I + lane) * 2 + 1];
    n_failed = e < 0, n_err = e < 0 ? 0 : e, n_bit = e < 0 ? 0 : be;
  }
#pragma unroll
  for (int d = 4; d >= 1; d >>= 1) n_failed += __shfl_xor(n_failed, d), n_err += __shfl_xor(n_err, d), n_bit += __shfl_xor(n_bit, d);
  __syncthreads();
  if (lane != 0) return;
  int32_t* o = rows + (int64_t)row * 6;
  uint32_t calc, recv;
  const int ok = frame_crc_bytes(vb, n_bytes, crc, &calc, &recv);
  o[0] = n_failed, o[1] = n_err, o[2] = n_bit, o[3] = (int32_t)calc, o[4] = (int32_t)recv, o[5] = ok;
}

int rs_gcd(int a, int b) { return b ? rs_gcd(b, a % b) : a; }

// the checks the two launches share: the code, and every frame's row inside the tables and named once
int rs_check_args(const char* what, int32_t n_frame, const int32_t* row_host, const sy11_rs_code* code, int64_t n_rows) {
  const int rc = frame_rows_once(what, n_frame, row_host, n_rows);
  if (rc != SY11_OK) return rc;
  const sy11_rs_code& c = *code;
  SY11_REQUIRE(c.k >= 1 && c.k < c.n && c.n <= 255 && c.n - c.k <= RS_NROOTS_MAX, "%s: the code (n=%d, k=%d) is not 1 <= k < n <= 255 with n - k <= %d", what, c.n, c.k, RS_NROOTS_MAX);
  SY11_REQUIRE(c.fcr >= 0 && c.fcr <= 254, "%s: fcr %d is not in [0, 254]", what, c.fcr);
  SY11_REQUIRE(c.prim >= 1 && c.prim <= 254 && rs_gcd(c.prim, 255) == 1, "%s: prim %d is not in [1, 254] and coprime to 255", what, c.prim);
  SY11_REQUIRE(c.interleave >= 1 && c.interleave <= RS_I_MAX, "%s: interleave %d is not in [1, %d]", what, c.interleave, RS_I_MAX);
  SY11_REQUIRE(c.poly >= 0x100 && c.poly <= 0x1FF, "%s: the field polynomial 0x%x does not have 9 bits", what, c.poly);
  unsigned v = 1;
  int order = 0;
  do v = rs_mul_slow(v, 2, (unsigned)c.poly), ++order; while (v != 1 && order < 256);
  SY11_REQUIRE(order == 255, "%s: the field polynomial 0x%x is not primitive (x has order %d)", what, c.poly, order);
  return SY11_OK;
}

}  // namespace

extern "C" int sy11_rs_decode(int32_t n_frame, const int32_t* row_host, const int32_t* row, const sy11_rs_code* code, int32_t offset, int64_t n_rows,
                              int64_t stride_data, const uint8_t* data, int64_t stride_info, uint8_t* info, int32_t* cw, void* stream) {
  SY11_REQUIRE(row_host && row && code && data && info && cw, "rs_decode: null frame table / code / data / info / cw");
  SY11_REQUIRE((((uintptr_t)row | (uintptr_t)cw) & 3) == 0, "rs_decode: the frame table and cw must be 4-byte aligned");
  const int rc = rs_check_args("rs_decode", n_frame, row_host, code, n_rows);
  if (rc != SY11_OK) return rc;
  const int64_t block = (int64_t)code->interleave * code->n;
  SY11_REQUIRE(stride_data >= 1 && stride_data < (1LL << 31) && offset >= 0 && offset + block <= stride_data,
               "rs_decode: the %d x %d bytes at offset %d leave the %ld bytes of a data row", code->interleave, code->n, offset, (long)stride_data);
  SY11_REQUIRE(stride_info < (1LL << 31) && (int64_t)code->interleave * code->k <= stride_info, "rs_decode: the %d x %d information bytes leave the %ld bytes of an info row",
               code->interleave, code->k, (long)stride_info);
  const int per = code->interleave >= 4 ? 1 : 4 / code->interleave;
  hipLaunchKernelGGL(rs_decode_kernel, dim3((n_frame + per - 1) / per), dim3(RS_WAVE * per * code->interleave), 0, (hipStream_t)stream, row, (int)n_frame, *code, (int)offset, per,
                     stride_data, data, stride_info, info, cw);
  SY11_LAUNCH_CHECK("rs_decode");
  return SY11_OK;
}

extern "C" int sy11_rs_check(int32_t n_frame, const int32_t* row_host, const int32_t* row, const sy11_rs_code* code, const sy11_fec_crc* crc, int64_t n_rows,
                             int64_t stride_info, const uint8_t* info, const int32_t* cw, int32_t* rows, void* stream) {
  SY11_REQUIRE(row_host && row && code && crc && info && cw && rows, "rs_check: null frame table / code / crc / info / cw / rows");
  SY11_REQUIRE((((uintptr_t)row | (uintptr_t)cw | (uintptr_t)rows) & 3) == 0, "rs_check: the frame table, cw and rows must be 4-byte aligned");
  const int rc = rs_check_args("rs_check", n_frame, row_host, code, n_rows);
  if (rc != SY11_OK) return rc;
  const int n_bytes = code->interleave * code->k;
  SY11_REQUIRE(stride_info < (1LL << 31) && n_bytes <= stride_info, "rs_check: the %d x %d information bytes leave the %ld bytes of an info row", code->interleave, code->k,
               (long)stride_info);
  const int bad = frame_crc_refused("rs_check", crc, 8 * (int64_t)n_bytes, true);
  if (bad != SY11_OK) return bad;
  hipLaunchKernelGGL(rs_check_kernel, dim3(n_frame), dim3(RS_WAVE), 0, (hipStream_t)stream, row, (int)code->interleave, (int)code->k, *crc, stride_info, info, cw, rows);
  SY11_LAUNCH_CHECK("rs_check");
  return SY11_OK;
}
