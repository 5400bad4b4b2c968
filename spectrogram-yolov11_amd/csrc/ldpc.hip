// ldpc.hip — decode the frames of a quasi-cyclic LDPC code: the layered normalised min-sum decoder over the int8 soft bits that launch 1 of fec.hip
// (sy11_fec_soft with T = N / 2, tail 0, period 2, pattern 3; unchanged) wrote (launch 2, sy11_ldpc_decode), then the channel error count, the de-whitened
// information bits and their CRC (launch 3, sy11_ldpc_check), each over all frames at once.  No reference counterpart; spec in DESIGN.md §4, plan in
// sy11/data/ldpc.py.
//
//   code      base matrix mb x nb over circulants of size Z: entry (column j, shift s) of layer i joins check c = i Z + r to variable n = j Z + (r + s) mod Z, r in [0, Z)
//   state     Q[n] = y[n];  R[c, j] = 0
//   layer     for every check c of the layer (they share no variable):  T_j = Q[n_j] - R[c, j],  s_j = T_j < 0,  a_j = |T_j|;  m1 = min a_j at j1, m2 = min over j != j1,
//             S = XOR s_j;  R[c, j] = (S ^ s_j ? -1 : +1) min((scale (j == j1 ? m2 : m1)) >> 4, 127);  Q[n_j] = T_j + R[c, j]
//   stop      after the mb layers x[n] = Q[n] < 0, unsat = #{c : XOR_j x[n_j] = 1};  stop at unsat = 0 or after `iterations`
//
//  * Exact integer arithmetic: the results are the numpy definition's bit for bit and depend neither on the frame's place in the launch nor on the
//    other frames of it.  No atomics, no floating point.  NO CLAMP ON Q: Q[n] = y[n] + sum_c R[c, .] over the checks of n, a column has at most mb <= 64
//    entries and |R| <= 127, so |Q| <= 127 * 65 and |T| <= 127 * 65 + 127: int16 holds both.
//  * ONE WORKGROUP IS ONE FRAME, 64 lanes per started 64 checks of a layer, 256 at the most; thread r owns the checks r, r + W, ... of every layer for all
//    iterations.  Q lives in LDS as int16 (2 N bytes), loaded once with coalesced int8 reads.  R is kept COMPRESSED per check, 8 bytes in LDS: the two scaled
//    minima, j1 and a sign word of 32 bits (a row has at most 32 entries).  A check is two sweeps over its entries: the first forms T_j from Q and the old R
//    and finds m1, m2, j1 and the signs; the second forms T_j again (nobody else writes these Q in this layer) and writes Q.  No per-thread array, no scratch.
//  * The (column, shift) table and the layers' offsets are staged in LDS once (4 bytes an entry); all threads read the same entry at a time, a broadcast.
//  * ONE BARRIER PER LAYER, and one per iteration for the workgroup's count of unsatisfied checks: a wave sums by shuffles, lane 0 of each writes its sum,
//    after the barrier EVERY thread adds the same words, so the loop's exit is uniform over the workgroup.  The words are written again only behind the next
//    iteration's layer barriers.
//  * Dynamic LDS: 2 N + 8 M + 4 n_entry + 4 (mb + 1) + 16 bytes, each part rounded up to 16: 11.8 KiB for N = 1944 at rate 1/2, 160 KiB at the most (a code
//    beyond that is refused).  Launch 3 is bandwidth-trivial: one workgroup of 256 per frame; the CRC is a serial bit loop of one thread
//    (frame_check.h: what launch 3 shares with fec.hip and rs.hip).
#include "common.h"
#include "frame_check.h"

#include <vector>

namespace {

constexpr int LDPC_MB_MAX = 64, LDPC_NB_MAX = 128, LDPC_Z_MAX = 512, LDPC_DEG_MIN = 2, LDPC_DEG_MAX = 32;
constexpr int LDPC_NMAX = 16384;                // 2 sy11_fec_tmax(): what launch 1 can write
constexpr int LDPC_ITER_MAX = 100, LDPC_SCALE_MAX = 16;
constexpr int64_t LDPC_LDS_MAX = 160 * 1024;

__host__ __device__ inline int64_t ldpc_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
// the carve of the dynamic LDS: Q, R, the entries, the layers' offsets, the waves' counts
__host__ __device__ inline int64_t ldpc_off_r(int N) { return ldpc_up16(2 * (int64_t)N); }
__host__ __device__ inline int64_t ldpc_off_entry(int N, int M) { return ldpc_off_r(N) + 8 * (int64_t)M; }
__host__ __device__ inline int64_t ldpc_off_layer(int N, int M, int n_entry) { return ldpc_off_entry(N, M) + ldpc_up16(4 * (int64_t)n_entry); }
__host__ __device__ inline int64_t ldpc_off_red(int N, int M, int n_entry, int mb) { return ldpc_off_layer(N, M, n_entry) + ldpc_up16(4 * (int64_t)(mb + 1)); }
__host__ __device__ inline int64_t ldpc_lds_bytes(int N, int M, int n_entry, int mb) { return ldpc_off_red(N, M, n_entry, mb) + 16; }

__device__ __forceinline__ int ldpc_var(uint32_t e, int r, int Z) {      // the variable that entry e (column Z | shift << 16) joins to row r of its layer
  int s = r + (int)(e >> 16);
  s = s >= Z ? s - Z : s;
  return (int)(e & 0xffffu) + s;
}

__global__ __launch_bounds__(256) void ldpc_decode_kernel(const int32_t* __restrict__ frame_row, sy11_ldpc_code code, const int32_t* __restrict__ layer,
                                                          const sy11_ldpc_entry* __restrict__ entry, int iterations, int scale, int64_t stride_soft,
                                                          const int8_t* __restrict__ soft, int64_t stride_bits, uint8_t* __restrict__ bits, int32_t* __restrict__ out,
                                                          int64_t stride_post, int16_t* __restrict__ post) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_smem[];
  const int Z = code.Z, mb = code.mb, n_entry = code.n_entry, N = code.nb * Z, M = mb * Z;
  const int tid = threadIdx.x, W = blockDim.x, lane = tid & 63, wave = tid >> 6, n_wave = W >> 6;
  int16_t* Q = (int16_t*)ldpc_smem;
  uint2* Rc = (uint2*)(ldpc_smem + ldpc_off_r(N));                          // x: m1 | m2 << 8 | j1 << 16 (the minima scaled and clipped), y: bit j = R[c, j] < 0 (or -0)
  uint32_t* ent = (uint32_t*)(ldpc_smem + ldpc_off_entry(N, M));
  int* loff = (int*)(ldpc_smem + ldpc_off_layer(N, M, n_entry));
  int* red = (int*)(ldpc_smem + ldpc_off_red(N, M, n_entry, mb));
  const int row = frame_row[blockIdx.x];
  const int8_t* y = soft + (int64_t)row * stride_soft;
  for (int n = tid; n < N; n += W) Q[n] = (int16_t)y[n];
  for (int c = tid; c < M; c += W) Rc[c] = make_uint2(0u, 0u);
  for (int e = tid; e < n_entry; e += W) {
    const sy11_ldpc_entry v = entry[e];
    ent[e] = (uint32_t)(v.column * Z) | ((uint32_t)v.shift << 16);          // column Z < N <= 16384, shift < 512
  }
  for (int i = tid; i <= mb; i += W) loff[i] = layer[i];
  __syncthreads();
  int it = 1, unsat = 0;
  for (;; ++it) {
    for (int i = 0; i < mb; ++i) {
      const int e0 = loff[i], deg = loff[i + 1] - e0;
      const uint32_t live = deg == 32 ? ~0u : (1u << deg) - 1u;
      for (int r = tid; r < Z; r += W) {
        const int c = i * Z + r;
        const uint2 old = Rc[c];
        const int om1 = (int)(old.x & 0xffu), om2 = (int)((old.x >> 8) & 0xffu), oj1 = (int)(old.x >> 16);
        int m1 = 1 << 20, m2 = 1 << 20, j1 = 0;
        uint32_t sg = 0;
#pragma unroll 4
        for (int j = 0; j < deg; ++j) {
          const int n = ldpc_var(ent[e0 + j], r, Z);
          const int mag = j == oj1 ? om2 : om1;
          const int T = (int)Q[n] - (((old.y >> j) & 1u) ? -mag : mag);
          const int a = T < 0 ? -T : T;
          sg |= (uint32_t)(T < 0) << j;
          if (a < m1) m2 = m1, m1 = a, j1 = j;
          else if (a < m2) m2 = a;
        }
        const uint32_t ns = ((__popc(sg) & 1) ? ~sg : sg) & live;           // bit j = S ^ s_j
        int s1 = (scale * m1) >> 4, s2 = (scale * m2) >> 4;
        s1 = s1 > 127 ? 127 : s1, s2 = s2 > 127 ? 127 : s2;
#pragma unroll 4
        for (int j = 0; j < deg; ++j) {
          const int n = ldpc_var(ent[e0 + j], r, Z);
          const int mag = j == oj1 ? om2 : om1;
          const int T = (int)Q[n] - (((old.y >> j) & 1u) ? -mag : mag);
          const int nm = j == j1 ? s2 : s1;
          Q[n] = (int16_t)(T + (((ns >> j) & 1u) ? -nm : nm));
        }
        Rc[c] = make_uint2((uint32_t)s1 | ((uint32_t)s2 << 8) | ((uint32_t)j1 << 16), ns);
      }
      __syncthreads();
    }
    // the checks the hard decision leaves unsatisfied: every thread over its own, then the workgroup's sum, the same value in every thread
    int bad = 0;
    for (int i = 0; i < mb; ++i) {
      const int e0 = loff[i], deg = loff[i + 1] - e0;
      for (int r = tid; r < Z; r += W) {
        int p = 0;
#pragma unroll 4
        for (int j = 0; j < deg; ++j) p ^= (int)(Q[ldpc_var(ent[e0 + j], r, Z)] < 0);
        bad += p;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d);
    if (lane == 0) red[wave] = bad;
    __syncthreads();
    unsat = 0;
    for (int w = 0; w < n_wave; ++w) unsat += red[w];
    if (unsat == 0 || it == iterations) break;                              // uniform over the workgroup
  }
  uint8_t* dst = bits + (int64_t)row * stride_bits;
  const int n_bytes = (N + 7) / 8;
  for (int64_t b = tid; b < stride_bits; b += W) {
    int byte = 0;
    if (b < n_bytes) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int n = (int)b * 8 + k;
        if (n < N && Q[n] < 0) byte |= 0x80 >> k;
      }
    }
    dst[b] = (uint8_t)byte;
  }
  if (post) {
    int16_t* pq = post + (int64_t)row * stride_post;
    for (int n = tid; n < N; n += W) pq[n] = Q[n];
  }
  if (tid == 0) out[2 * (int64_t)row] = it, out[2 * (int64_t)row + 1] = unsat;
}

__global__ __launch_bounds__(256) void ldpc_check_kernel(const int32_t* __restrict__ frame_row, int N, int K, const uint8_t* __restrict__ whiten, sy11_fec_crc crc,
                                                         int64_t stride_soft, const int8_t* __restrict__ soft, int64_t stride_bits, const uint8_t* __restrict__ bits,
                                                         int64_t stride_data, uint8_t* __restrict__ data, int32_t* __restrict__ rows) {
  __shared__ uint8_t vb[LDPC_NMAX / 8];
  __shared__ int sh[2][4];
  const int row = frame_row[blockIdx.x], t = threadIdx.x;
  const uint8_t* src = bits + (int64_t)row * stride_bits;
  const int8_t* y = soft + (int64_t)row * stride_soft;
  int n_ch = 0, n_err = 0;
  for (int n = t; n < N; n += 256) {
    const int v = y[n], x = (src[n >> 3] >> (7 - (n & 7))) & 1;
    n_ch += v != 0;
    n_err += v != 0 && (v < 0) != x;
  }
  frame_count_reduce(n_ch, n_err, sh, t);
  frame_dewhiten_pack(src, K, whiten, stride_data, data + (int64_t)row * stride_data, vb, t);
  __syncthreads();
  if (t != 0) return;
  uint32_t calc, recv;
  const int ok = frame_crc_bits(vb, K, crc, &calc, &recv);
  frame_row_write(rows + (int64_t)row * 5, calc, recv, ok, sh);
}

}  // namespace

extern "C" int32_t sy11_ldpc_nmax(void) { return LDPC_NMAX; }

extern "C" int64_t sy11_ldpc_lds_bytes(int32_t Z, int32_t mb, int32_t nb, int32_t n_entry) {
  if (Z < 1 || Z > LDPC_Z_MAX || mb < 1 || mb > LDPC_MB_MAX || nb < 1 || nb > LDPC_NB_MAX || n_entry < 0 || n_entry > LDPC_MB_MAX * LDPC_DEG_MAX) return -1;
  return ldpc_lds_bytes(nb * Z, mb * Z, n_entry, mb);
}

extern "C" int sy11_ldpc_decode(int32_t n_frame, const int32_t* row_host, const int32_t* row, const sy11_ldpc_code* code, const int32_t* layer_host, const int32_t* layer,
                                const sy11_ldpc_entry* entry_host, const sy11_ldpc_entry* entry, int32_t iterations, int32_t scale, int64_t n_rows, int64_t stride_soft,
                                const int8_t* soft, int64_t stride_bits, uint8_t* bits, int32_t* out, int64_t stride_post, int16_t* post, void* stream) {
  SY11_REQUIRE(row_host && row && code && layer_host && layer && entry_host && entry && soft && bits && out,
               "ldpc_decode: null frame table / code / layer offsets / entries / soft / bits / out");
  SY11_REQUIRE((((uintptr_t)row | (uintptr_t)layer | (uintptr_t)entry | (uintptr_t)out) & 3) == 0 && ((uintptr_t)post & 1) == 0,
               "ldpc_decode: the frame table, the layer offsets, the entries and out must be 4-byte aligned, post 2-byte");
  const sy11_ldpc_code& c = *code;
  SY11_REQUIRE(c.Z >= 1 && c.Z <= LDPC_Z_MAX && c.mb >= 1 && c.mb <= LDPC_MB_MAX && c.nb > c.mb && c.nb <= LDPC_NB_MAX,
               "ldpc_decode: the code (Z=%d, mb=%d, nb=%d) is not 1 <= Z <= %d, 1 <= mb <= %d, mb < nb <= %d", c.Z, c.mb, c.nb, LDPC_Z_MAX, LDPC_MB_MAX, LDPC_NB_MAX);
  const int N = c.nb * c.Z, M = c.mb * c.Z;
  SY11_REQUIRE(N % 2 == 0 && N <= LDPC_NMAX, "ldpc_decode: N = nb Z = %d is not even and at most %d", N, LDPC_NMAX);
  SY11_REQUIRE(c.n_entry >= LDPC_DEG_MIN * c.mb && c.n_entry <= LDPC_DEG_MAX * c.mb, "ldpc_decode: %d entries are not %d .. %d for each of the %d layers", c.n_entry, LDPC_DEG_MIN,
               LDPC_DEG_MAX, c.mb);
  SY11_REQUIRE(iterations >= 1 && iterations <= LDPC_ITER_MAX, "ldpc_decode: iterations %d is not in [1, %d]", iterations, LDPC_ITER_MAX);
  SY11_REQUIRE(scale >= 1 && scale <= LDPC_SCALE_MAX, "ldpc_decode: scale %d (sixteenths) is not in [1, %d]", scale, LDPC_SCALE_MAX);
  SY11_REQUIRE(layer_host[0] == 0 && layer_host[c.mb] == c.n_entry, "ldpc_decode: the layer offsets run from %d to %d, not from 0 to the %d entries", layer_host[0], layer_host[c.mb],
               c.n_entry);
  std::vector<int> weight((size_t)c.nb, 0), last((size_t)c.nb, -1);
  for (int i = 0; i < c.mb; ++i) {
    const int64_t e0 = layer_host[i], e1 = layer_host[i + 1];
    SY11_REQUIRE(e0 >= 0 && e1 > e0 && e1 <= c.n_entry, "ldpc_decode: layer %d: the offsets %ld, %ld are not rising within the %d entries", i, (long)e0, (long)e1, c.n_entry);
    SY11_REQUIRE(e1 - e0 >= LDPC_DEG_MIN && e1 - e0 <= LDPC_DEG_MAX, "ldpc_decode: layer %d: a row weight of %ld is not in [%d, %d]", i, (long)(e1 - e0), LDPC_DEG_MIN, LDPC_DEG_MAX);
    for (int64_t e = e0; e < e1; ++e) {
      const sy11_ldpc_entry& v = entry_host[e];
      SY11_REQUIRE(v.column >= 0 && v.column < c.nb, "ldpc_decode: entry %ld of layer %d: column %d is not in [0, %d)", (long)(e - e0), i, v.column, c.nb);
      SY11_REQUIRE(v.shift >= 0 && v.shift < c.Z, "ldpc_decode: entry %ld of layer %d: shift %d is not in [0, %d)", (long)(e - e0), i, v.shift, c.Z);
      SY11_REQUIRE(last[(size_t)v.column] != i, "ldpc_decode: layer %d names column %d twice", i, v.column);
      last[(size_t)v.column] = i, ++weight[(size_t)v.column];
    }
  }
  for (int j = 0; j < c.nb; ++j) SY11_REQUIRE(weight[(size_t)j] >= 1, "ldpc_decode: column %d of the code has no entry", j);
  const int64_t lds = ldpc_lds_bytes(N, M, c.n_entry, c.mb);
  SY11_REQUIRE(lds <= LDPC_LDS_MAX, "ldpc_decode: the code needs %ld bytes of LDS (2 N + 8 M + 4 entries), more than the %ld of a compute unit", (long)lds, (long)LDPC_LDS_MAX);
  const int rc = frame_rows_once("ldpc_decode", n_frame, row_host, n_rows);
  if (rc != SY11_OK) return rc;
  SY11_REQUIRE(stride_soft >= N && stride_soft <= LDPC_NMAX, "ldpc_decode: the %d soft bits leave a row of %ld bytes (at most %d)", N, (long)stride_soft, LDPC_NMAX);
  SY11_REQUIRE(stride_bits >= (N + 7) / 8 && stride_bits <= LDPC_NMAX / 8, "ldpc_decode: the %d bits leave a row of %ld bytes (at most %d)", N, (long)stride_bits, LDPC_NMAX / 8);
  SY11_REQUIRE(!post || (stride_post >= N && stride_post <= LDPC_NMAX), "ldpc_decode: the %d posteriors leave a row of %ld int16 (at most %d)", N, (long)stride_post, LDPC_NMAX);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)ldpc_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) SY11_FAIL(SY11_ELAUNCH, "ldpc_decode: %ld bytes of dynamic LDS were refused: %s", (long)lds, hipGetErrorString(e));
  }
  const int W = c.Z > 192 ? 256 : 64 * ((c.Z + 63) / 64);
  hipLaunchKernelGGL(ldpc_decode_kernel, dim3(n_frame), dim3(W), (size_t)lds, (hipStream_t)stream, row, c, layer, entry, (int)iterations, (int)scale, stride_soft, soft, stride_bits,
                     bits, out, stride_post, post);
  SY11_LAUNCH_CHECK("ldpc_decode");
  return SY11_OK;
}

extern "C" int sy11_ldpc_check(int32_t n_frame, const int32_t* row_host, const int32_t* row, int32_t N, int32_t K, const uint8_t* whiten, const sy11_fec_crc* crc,
                               int64_t n_rows, int64_t stride_soft, const int8_t* soft, int64_t stride_bits, const uint8_t* bits, int64_t stride_data, uint8_t* data,
                               int32_t* rows, void* stream) {
  SY11_REQUIRE(row_host && row && crc && soft && bits && data && rows, "ldpc_check: null frame table / crc / soft / bits / data / rows");
  SY11_REQUIRE((((uintptr_t)row | (uintptr_t)rows) & 3) == 0, "ldpc_check: the frame table and the rows must be 4-byte aligned");
  SY11_REQUIRE(N >= 2 && N <= LDPC_NMAX && N % 2 == 0 && K >= 1 && K < N, "ldpc_check: N = %d is not even and in [2, %d], or K = %d not in [1, N)", N, LDPC_NMAX, K);
  SY11_REQUIRE(stride_soft >= N && stride_soft <= LDPC_NMAX && stride_bits >= (N + 7) / 8 && stride_bits <= LDPC_NMAX / 8 && stride_data >= (K + 7) / 8 &&
                   stride_data <= LDPC_NMAX / 8,
               "ldpc_check: the %d soft bits, %d bits or %d information bits leave a row of %ld / %ld / %ld bytes (at most %d / %d / %d)", N, N, K, (long)stride_soft,
               (long)stride_bits, (long)stride_data, LDPC_NMAX, LDPC_NMAX / 8, LDPC_NMAX / 8);
  int rc = frame_crc_refused("ldpc_check", crc, K, false);
  if (rc != SY11_OK) return rc;
  rc = frame_rows_once("ldpc_check", n_frame, row_host, n_rows);
  if (rc != SY11_OK) return rc;
  hipLaunchKernelGGL(ldpc_check_kernel, dim3(n_frame), dim3(256), 0, (hipStream_t)stream, row, (int)N, (int)K, whiten, *crc, stride_soft, soft, stride_bits, bits, stride_data, data,
                     rows);
  SY11_LAUNCH_CHECK("ldpc_check");
  return SY11_OK;
}
