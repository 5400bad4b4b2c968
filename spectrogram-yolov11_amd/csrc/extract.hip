// extract.hip — every detection of a scan as baseband IQ, in one launch: per clip mix -> low-pass -> decimate by D = 2^l -> cut in time
// (no reference counterpart; spec in DESIGN.md §4, plan in sy11/data/extract.py).
//
//   clip[m - m0] = sum_{j < T} taps_D[j] xm[m D + 16 D - j],   T = 32 D + 1,   xm[i] = x[i] e^{j 2 pi frac(i dphi / 2^32)},   x = 0 outside in[]
//
// which is ddc.hip with P = 1, Q = D, c = 16 D and the same table, bit for bit: the same mix() (iqmix.h), and per output ONE sequential
// float32 fmaf sum over j = 0 .. T-1.  D = 1 has no filter (out = xm, as ddc.hip's mixer).
//
//  * One launch serves every segment (a clip, or a piece of one) the host lists.  The host also lists, per workgroup, its segment and
//    its first output (the tile map): a workgroup looks itself up, so the grid has exactly as many blocks as there are tiles — no
//    (max tiles x detections) grid with idle blocks.
//  * A workgroup stages its table and the input span of its tile, already mixed, into LDS (pair loads, odd base and zeros outside in[]
//    as in ddc.hip), then each thread sums its outputs.
//  * LDS layout: consecutive lanes sum consecutive outputs, whose samples lie D slots apart; read as ds_read_b64 that is a stride of
//    2 D dwords over 64 banks, a min(D, 32)-way conflict.  Staged slot s is therefore stored at s + (s >> l): all lanes of a read
//    share (slot mod D), so consecutive lanes are D + 1 slots = 2 D + 2 dwords apart, gcd(2 D + 2, 64) = 2 for every D = 2 .. 64, and the
//    32 lanes of a half wave hit 32 different bank pairs.  The sum order is untouched.
#include "common.h"
#include "iqmix.h"

namespace {

constexpr int EXT_LDS_BUDGET = 64 * 1024;      // per workgroup, as ddc.hip
constexpr int EXT_MAX_LOG2D = 6;

// outputs of one tile: 64 at D = 64 (63 * 64 + 2049 staged samples), up to 1024
__host__ __device__ inline int tile_of(int l) { return l == 0 ? 1024 : (4096 >> l < 1024 ? 4096 >> l : 1024); }
// first float of table D = 2^l in the concatenated tap buffer: every table starts on a multiple of 4 floats
__host__ __device__ inline int taps_off(int l) { return l == 0 ? 0 : (32 << l) - 64 + 4 * l; }
// staged samples of a full tile (+ 1 for the alignment sample) and the LDS bytes of a workgroup: table, then the skewed samples
inline long span_of(int l) { return (long)(tile_of(l) - 1) * (1 << l) + (32 << l) + 2; }
inline long lds_of(int l) { return l == 0 ? 0 : ((32L << l) + 4) * 4 + (span_of(l) + (span_of(l) >> l) + 1) * 8; }

__global__ __launch_bounds__(256) void extract_kernel(const sy11_iq_segment* __restrict__ seg, const int2* __restrict__ tiles,
                                                      const float* __restrict__ taps, int64_t n0, int n_in, const float2* __restrict__ in,
                                                      float2* __restrict__ out) {
  extern __shared__ float4 lds_raw[];
  const int2 tl = tiles[blockIdx.x];                                      // (segment, first output of the tile relative to its m0)
  const sy11_iq_segment sg = seg[tl.x];
  const int l = sg.log2d, first = tl.y;
  const uint32_t dphi = sg.dphi;
  const int nt = min(tile_of(l), sg.M - first);
  const int64_t mf = sg.m0 + first;                                       // absolute index of the tile's first output
  float2* dst = out + sg.out_off + first;
  if (l == 0) {                                                           // no filter: output m is sample m
    for (int t = threadIdx.x; t < nt; t += blockDim.x) {
      const int64_t r = mf + t - n0;
      float2 v = make_float2(0.f, 0.f);
      if (r >= 0 && r < n_in) v = in[r];
      if (dphi != 0u) v = mix(v, (uint32_t)(uint64_t)(mf + t) * dphi);
      dst[t] = v;
    }
    return;
  }
  const int D = 1 << l, T = 32 * D + 1;
  float* hs = (float*)lds_raw;                                            // T taps in 32 D + 4 floats
  float2* xs = (float2*)(hs + 32 * D + 4);                                // staged slot s at s + (s >> l)
  // staged samples: absolute [lo, lo + len), lo = the oldest sample the first output reads (m D + 16 D - (T - 1)), moved one down where
  // that makes the first staged sample 16-byte aligned in in[]
  int64_t lo = (mf - 16) * D;
  const int len_needed = (nt - 1) * D + T;
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
    xs[s + (s >> l)] = a;
    if (s + 1 < len) xs[s + 1 + ((s + 1) >> l)] = b;
  }
  const float* h = taps + taps_off(l);
  for (int k = threadIdx.x; k < T; k += blockDim.x) hs[k] = h[k];
  __syncthreads();
  const int base = 32 * D + (odd ? 1 : 0);                                // slot of the first output's newest sample
  for (int t = threadIdx.x; t < nt; t += blockDim.x) {
    const float2* x = xs + t * (D + 1);                                   // slot base + t D - j sits at (base - j) + ((base - j) >> l) + t (D + 1)
    float re = 0.f, im = 0.f;
    for (int j = 0; j < T; ++j) {
      const int q = base - j;                                             // >= 0, uniform
      const float w = hs[j];
      const float2 v = x[q + (q >> l)];
      re = fmaf(w, v.x, re);
      im = fmaf(w, v.y, im);
    }
    dst[t] = make_float2(re, im);
  }
}

}  // namespace

extern "C" int32_t sy11_iq_extract_tile(int32_t log2d) { return log2d < 0 || log2d > EXT_MAX_LOG2D ? 0 : tile_of(log2d); }

extern "C" int sy11_iq_extract(int32_t n_seg, const sy11_iq_segment* seg_host, const sy11_iq_segment* seg, int32_t n_tile,
                               const int32_t* tile_host, const int32_t* tile, const float* taps, int64_t n_total, int64_t n0, int32_t n_in,
                               const float* in, int64_t out_len, float* out, void* stream) {
  SY11_REQUIRE(seg_host && seg && tile_host && tile && taps && in && out, "iq_extract: null segment table / tile map / tap table / input / output");
  SY11_REQUIRE(n_seg > 0 && n_tile > 0, "iq_extract: need at least one segment and one tile (n_seg=%d n_tile=%d)", n_seg, n_tile);
  SY11_REQUIRE(n_in > 0 && out_len > 0, "iq_extract: n_in and out_len must be positive (n_in=%d out_len=%ld)", n_in, (long)out_len);
  SY11_REQUIRE(n0 >= 0 && n_total > 0 && n0 + n_in <= n_total && n_total < (1LL << 48),
               "iq_extract: in[] = samples [%ld, %ld) must lie inside the capture's %ld (below 2^48)", (long)n0, (long)n0 + n_in, (long)n_total);
  SY11_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 7) == 0, "iq_extract: in / out must be 8-byte aligned (complex64 samples)");
  SY11_REQUIRE((((uintptr_t)seg | (uintptr_t)tile | (uintptr_t)taps) & 7) == 0, "iq_extract: segment table, tile map and tap table must be 8-byte aligned");
  long lds = 0;
  for (int i = 0; i < n_seg; ++i) {                                       // no segment reads outside in[] (clipped to the capture) or writes outside out
    const sy11_iq_segment& s = seg_host[i];
    SY11_REQUIRE(s.log2d >= 0 && s.log2d <= EXT_MAX_LOG2D, "iq_extract: segment %d: log2 D = %d is not in [0, %d]", i, s.log2d, EXT_MAX_LOG2D);
    const int64_t D = 1LL << s.log2d;
    SY11_REQUIRE(s.M > 0 && s.m0 >= 0 && s.m0 < (1LL << 48) && (s.m0 + s.M - 1) * D < n_total,
                 "iq_extract: segment %d: outputs [%ld, %ld) at D = %ld are not on the capture's %ld samples", i, (long)s.m0, (long)s.m0 + s.M,
                 (long)D, (long)n_total);
    SY11_REQUIRE(s.out_off >= 0 && s.out_off + s.M <= out_len, "iq_extract: segment %d writes [%ld, %ld) of an output of %ld samples", i,
                 (long)s.out_off, (long)s.out_off + s.M, (long)out_len);
    int64_t a = s.log2d ? (s.m0 - 16) * D : s.m0, b = s.log2d ? (s.m0 + s.M - 1 + 16) * D + 1 : s.m0 + s.M;
    a = a < 0 ? 0 : a;
    b = b > n_total ? n_total : b;
    SY11_REQUIRE(a >= n0 && b <= n0 + n_in, "iq_extract: segment %d reads samples [%ld, %ld); in[] holds [%ld, %ld)", i, (long)a, (long)b, (long)n0,
                 (long)n0 + n_in);
    if (lds_of(s.log2d) > lds) lds = lds_of(s.log2d);
  }
  SY11_REQUIRE(lds <= EXT_LDS_BUDGET, "iq_extract: a tile needs %ld bytes of LDS", lds);
  for (int i = 0; i < n_tile; ++i) {
    const int32_t sidx = tile_host[2 * i], first = tile_host[2 * i + 1];
    SY11_REQUIRE(sidx >= 0 && sidx < n_seg, "iq_extract: tile %d names segment %d of %d", i, sidx, n_seg);
    SY11_REQUIRE(first >= 0 && first < seg_host[sidx].M && first % tile_of(seg_host[sidx].log2d) == 0,
                 "iq_extract: tile %d starts at output %d of segment %d (M = %d, tiles of %d)", i, first, sidx, seg_host[sidx].M,
                 tile_of(seg_host[sidx].log2d));
  }
  hipLaunchKernelGGL(extract_kernel, dim3(n_tile), dim3(256), (size_t)lds, (hipStream_t)stream, seg, (const int2*)tile, taps, n0, n_in,
                     (const float2*)in, (float2*)out);
  SY11_LAUNCH_CHECK("iq_extract");
  return SY11_OK;
}
