// frame_check.h — what the check launches of the frame path share (sy11_fec_check, sy11_ldpc_check, sy11_rs_check; spec in DESIGN.md §4): the de-whitened,
// packed information bits of a frame, THE CRC (the Rocksoft model, in its bit-serial and its byte-serial form, side by side), the workgroup's sum of the
// channel counts with the five-int result row, and on the host the refusals of a CRC and of a table of rows.
//
//   crc    width W, poly (without the top bit), init, refin, refout, xorout:  reg = init;  per message bit b, the first first (with refin every group of 8
//          bits LSB first):  fb = top(reg) ^ b,  reg = (reg << 1) mod 2^W,  reg ^= poly if fb;  with refout reg is reversed over its W bits;
//          crc_calc = reg ^ xorout;  crc_recv = the W bits (W / 8 bytes) after the message, MSB first;  ok = crc_calc == crc_recv, -1 without a crc (W = 0)
//
//  * Every device function is __forceinline__ and takes its arrays as plain pointers: inlined, a caller's LDS array stays an LDS access and a global row a
//    global one, so a check kernel compiles to what it was with the loops written out.  Exact integer arithmetic, no atomics.
//  * The bit-serial form serves the two decoders, whose information need not be whole bytes; the byte-serial form serves the Reed-Solomon check, whose
//    information is whole bytes and up to 2040 of them, at an eighth of the steps.  Both run in ONE thread, behind the caller's barrier.
#pragma once
#include "common.h"

#include <vector>

namespace {

// byte b of `src`, the bits from n_bits on cleared and `whiten` (one 0 / 1 byte per bit, or null) XORed onto the others -> vb[b] and dst[b], b < ceil(n_bits / 8);
// zeros to dst up to stride_data.  All 256 threads of the workgroup, t = threadIdx.x; vb is read behind the caller's barrier.
__device__ __forceinline__ void frame_dewhiten_pack(const uint8_t* src, int n_bits, const uint8_t* whiten, int64_t stride_data, uint8_t* dst, uint8_t* vb, int t) {
  const int n_data = (n_bits + 7) / 8;
  for (int64_t b = t; b < stride_data; b += 256) {
    int byte = 0;
    if (b < n_data) {
      byte = src[b];
      for (int i = 0; i < 8; ++i) {
        const int at = (int)b * 8 + i;
        if (at >= n_bits) byte &= ~(0x80 >> i);
        else if (whiten) byte ^= (whiten[at] & 1) << (7 - i);
      }
      vb[b] = (uint8_t)byte;
    }
    dst[b] = (uint8_t)byte;
  }
}

// the CRC of the n_bits bits of vb (packed MSB first), bit by bit: the check field is the last crc.width of them
__device__ __forceinline__ int frame_crc_bits(const uint8_t* vb, int n_bits, const sy11_fec_crc& crc, uint32_t* calc, uint32_t* recv) {
  *calc = 0, *recv = 0;
  if (!crc.width) return -1;
  const int W = crc.width, n_msg = n_bits - W;
  const uint64_t top = 1ull << (W - 1), all = (top << 1) - 1ull;
  uint64_t reg = crc.init & all;
  for (int k = 0; k < n_msg; ++k) {
    const int at = crc.refin ? (k & ~7) | (7 - (k & 7)) : k;                // with refin each group of 8 bits is taken LSB first
    const uint64_t bit = (vb[at >> 3] >> (7 - (at & 7))) & 1;
    const uint64_t fb = ((reg >> (W - 1)) & 1ull) ^ bit;
    reg = (reg << 1) & all;
    if (fb) reg ^= crc.poly;
  }
  if (crc.refout) {
    uint64_t r = 0;
    for (int i = 0; i < W; ++i) r |= ((reg >> i) & 1ull) << (W - 1 - i);
    reg = r;
  }
  *calc = (uint32_t)((reg ^ crc.xorout) & all);
  uint64_t got = 0;
  for (int k = n_msg; k < n_bits; ++k) got = (got << 1) | ((vb[k >> 3] >> (7 - (k & 7))) & 1);
  *recv = (uint32_t)got;
  return *calc == *recv;
}

// the same CRC over the n_bytes whole bytes of vb, byte by byte (crc.width is 8, 16, 24 or 32): the register is kept at the top of 32 bits, a byte is XORed
// onto its top and shifted out in 8 steps
__device__ __forceinline__ int frame_crc_bytes(const uint8_t* vb, int n_bytes, const sy11_fec_crc& crc, uint32_t* calc, uint32_t* recv) {
  *calc = 0, *recv = 0;
  if (!crc.width) return -1;
  const int W = crc.width, n_msg = n_bytes - W / 8;
  const int up = 32 - W;
  const uint32_t poly = crc.poly << up;
  uint32_t top = crc.init << up;
  for (int b = 0; b < n_msg; ++b) {
    const uint32_t byte = vb[b];
    top ^= crc.refin ? __brev(byte) : byte << 24;                           // with refin a byte is taken LSB first
#pragma unroll
    for (int i = 0; i < 8; ++i) top = (top << 1) ^ ((top >> 31) ? poly : 0u);
  }
  uint32_t reg = top >> up;
  if (crc.refout) reg = __brev(reg) >> up;
  *calc = reg ^ crc.xorout;
  uint64_t got = 0;
  for (int b = n_msg; b < n_bytes; ++b) got = (got << 8) | vb[b];
  *recv = (uint32_t)got;
  return *calc == *recv;
}

// a thread's counts of received bits and of those that differ from the decision -> the sums of each of the four waves in sh; all 256 threads, read behind a barrier
__device__ __forceinline__ void frame_count_reduce(int n_ch, int n_err, int (*sh)[4], int t) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n_ch += __shfl_xor(n_ch, d), n_err += __shfl_xor(n_err, d);
  if ((t & 63) == 0) sh[0][t >> 6] = n_ch, sh[1][t >> 6] = n_err;
}

// the result row of a decoded frame: crc_calc, crc_recv, crc_ok, channel_errors, n_channel; one thread
__device__ __forceinline__ void frame_row_write(int32_t* o, uint32_t calc, uint32_t recv, int ok, const int (*sh)[4]) {
  o[0] = (int32_t)calc, o[1] = (int32_t)recv, o[2] = ok;
  o[3] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3], o[4] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
}

// a launch's CRC over n_bits information bits: none (width 0), or 8 .. 32 bits (8, 16, 24 or 32 where the check runs byte by byte) below the n_bits, with
// fields of that width and, with refin, whole bytes before the check field -> SY11_OK, or the refusal
inline int frame_crc_refused(const char* what, const sy11_fec_crc* crc, int64_t n_bits, bool whole_bytes) {
  SY11_REQUIRE(crc->width == 0 || (crc->width >= 8 && crc->width <= 32 && (!whole_bytes || crc->width % 8 == 0)), "%s: a CRC of %d bits is not 0 (none)%s", what, crc->width,
               whole_bytes ? ", 8, 16, 24 or 32" : " or 8 .. 32");
  if (!crc->width) return SY11_OK;
  const uint64_t all = (1ull << crc->width) - 1ull;
  SY11_REQUIRE(n_bits > crc->width, "%s: %ld information bits do not exceed the CRC's %d", what, (long)n_bits, crc->width);
  SY11_REQUIRE((crc->poly & ~all) == 0 && (crc->init & ~all) == 0 && (crc->xorout & ~all) == 0 && (crc->refin | crc->refout) >> 1 == 0,
               "%s: poly / init / xorout beyond the CRC's %d bits, or refin / refout not 0 or 1", what, crc->width);
  SY11_REQUIRE(!crc->refin || (n_bits - crc->width) % 8 == 0, "%s: refin needs whole bytes before the check field, not %ld bits", what, (long)(n_bits - crc->width));
  return SY11_OK;
}

// a launch's table of frames: every frame's row inside the tables of n_rows rows and named once -> SY11_OK, or the refusal
inline int frame_rows_once(const char* what, int32_t n_frame, const int32_t* row_host, int64_t n_rows) {
  SY11_REQUIRE(n_frame > 0 && n_rows > 0 && n_rows < (1LL << 31), "%s: need frames and rows below 2^31 (n_frame=%d n_rows=%ld)", what, n_frame, (long)n_rows);
  std::vector<bool> seen((size_t)n_rows, false);
  for (int i = 0; i < n_frame; ++i) {
    const int32_t r = row_host[i];
    SY11_REQUIRE(r >= 0 && r < n_rows, "%s: frame %d reads row %d of a table of %ld rows", what, i, r, (long)n_rows);
    SY11_REQUIRE(!seen[(size_t)r], "%s: frame %d reads row %d, which an earlier frame of this call reads", what, i, r);
    seen[(size_t)r] = true;
  }
  return SY11_OK;
}

}  // namespace
