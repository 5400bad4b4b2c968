// iqaug.hip — the IQ side of the training loader: gather one window per sample out of captures resident in HBM (or of a staged
// device copy) and apply the whole IQ-domain augmentation recipe in the same pass (no reference counterpart: the reference trains
// from rendered images; spec in DESIGN.md §4).  One launch per batch, pure streaming: 1-2 source streams in, one stream out.
//
//   out[b,n] = g rot(c(src[off+n]), phi0 + n dphi) + g2 rot(c2(src2[off2+n]), phi02 + n dphi2) + sigma w(seed, n)
//
//  * Phase is a 32-bit accumulator: dphi / phi0 are uint32 fractions of a cycle and phi0 + n dphi wraps in uint32 arithmetic, so the
//    phase is exact for every n; only the final int32 -> float angle (|angle| <= pi, one sincosf) rounds.  A float 2 pi f n would
//    have lost the phase by n ~ 1e5.
//  * w: unit-variance complex normal.  Philox4x32-10 keyed by the seed, counter (n / 2, 0, 0, 0): the four words give the two
//    samples 2k and 2k + 1 through Box-Muller on (x + 0.5) 2^-32, so a sample depends on (seed, n) alone, never on the launch shape.
//  * Every step that is switched off is SKIPPED, not multiplied by one / added as zero: with g = 1, dphi = phi0 = 0, no conjugate,
//    no partner, sigma = 0 the output is the source bit for bit.
//  * One thread owns the output pair (2i, 2i + 1).  src_off may be odd, so a 16-byte load is used only where base + offset is
//    16-byte aligned (uniform per block); otherwise two 8-byte loads.  The same rule picks the store width.
#include "common.h"

namespace {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1) {
  uint32_t c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

// Box-Muller, variance 1/2 per component: radius sqrt(-ln u1), u1 = (x + 0.5) 2^-32; angle 2 pi (y + 0.5) 2^-32.  -ln u1 is taken
// from the end of the interval where the float conversion keeps relative precision: ln(u1) for u1 < 1/2, log1p(-(1 - u1)) above
// (1 - u1 = (~x + 0.5) 2^-32 exactly), so neither a tiny u1 nor a u1 next to 1 is rounded away.
__device__ __forceinline__ float2 normal_pair(uint32_t x, uint32_t y) {
  const float t = (x & 0x80000000u) ? -log1pf(-(((float)(~x) + 0.5f) * 0x1p-32f)) : -logf(((float)x + 0.5f) * 0x1p-32f);
  const float r = sqrtf(t);
  float s, c;
  sincosf(((float)(int32_t)y + 0.5f) * 0x1.921fb6p-30f, &s, &c);          // pi / 2^31: y as a signed fraction of a cycle
  return make_float2(r * c, r * s);
}

__device__ __forceinline__ float2 rot_gain(float2 z, bool conj, bool rotate, uint32_t phase, float g) {
  if (conj) z.y = -z.y;
  if (rotate) {
    float s, c;
    sincosf((float)(int32_t)phase * 0x1.921fb6p-30f, &s, &c);
    z = make_float2(z.x * c - z.y * s, z.x * s + z.y * c);
  }
  if (g != 1.0f) { z.x *= g; z.y *= g; }
  return z;
}

__device__ __forceinline__ void load_pair(const float2* p, bool vec, bool two, float2& a, float2& b) {
  if (vec && two) {
    const float4 v = *(const float4*)p;
    a = make_float2(v.x, v.y);
    b = make_float2(v.z, v.w);
  } else {
    a = p[0];
    b = two ? p[1] : make_float2(0.f, 0.f);
  }
}

__global__ __launch_bounds__(256) void iq_gather_augment_kernel(int L, const uint64_t* __restrict__ src_ptr, const int64_t* __restrict__ src_off,
                                                                const sy11_iq_recipe* __restrict__ rec, float2* __restrict__ out) {
  const int b = blockIdx.y;
  const int n = (blockIdx.x * 256 + threadIdx.x) * 2;                     // this thread: samples n, n + 1
  if (n >= L) return;
  const bool two = n + 1 < L;
  const sy11_iq_recipe r = rec[b];
  const float2* s1 = (const float2*)src_ptr[b] + src_off[b];
  float2 a, c;
  load_pair(s1 + n, (((uintptr_t)s1) & 15) == 0, two, a, c);
  const bool rot1 = (r.dphi | r.phi0) != 0u;
  a = rot_gain(a, r.flags & SY11_IQ_CONJ, rot1, r.phi0 + (uint32_t)n * r.dphi, r.gain);
  c = rot_gain(c, r.flags & SY11_IQ_CONJ, rot1, r.phi0 + (uint32_t)(n + 1) * r.dphi, r.gain);
  if (r.src2) {
    const float2* s2 = (const float2*)r.src2 + r.off2;
    float2 p, q;
    load_pair(s2 + n, (((uintptr_t)s2) & 15) == 0, two, p, q);
    const bool rot2 = (r.dphi2 | r.phi02) != 0u;
    p = rot_gain(p, r.flags & SY11_IQ_CONJ2, rot2, r.phi02 + (uint32_t)n * r.dphi2, r.gain2);
    q = rot_gain(q, r.flags & SY11_IQ_CONJ2, rot2, r.phi02 + (uint32_t)(n + 1) * r.dphi2, r.gain2);
    a.x += p.x; a.y += p.y;
    c.x += q.x; c.y += q.y;
  }
  if (r.sigma != 0.0f) {
    const U4 w = philox4x32_10((uint32_t)(n >> 1), (uint32_t)r.seed, (uint32_t)(r.seed >> 32));
    const float2 w0 = normal_pair(w.x, w.y), w1 = normal_pair(w.z, w.w);
    a.x += r.sigma * w0.x; a.y += r.sigma * w0.y;
    c.x += r.sigma * w1.x; c.y += r.sigma * w1.y;
  }
  float2* o = out + (long)b * L + n;
  if (two && (((uintptr_t)o) & 15) == 0) {
    *(float4*)o = make_float4(a.x, a.y, c.x, c.y);
  } else {
    o[0] = a;
    if (two) o[1] = c;
  }
}

}  // namespace

extern "C" int sy11_iq_gather_augment(int32_t B, int32_t L, const uint64_t* src_ptr, const int64_t* src_off, const sy11_iq_recipe* r,
                                      float* out, void* stream) {
  SY11_REQUIRE(src_ptr && src_off && r, "iq_gather_augment: null source pointer table / offset table / recipe table");
  SY11_REQUIRE(out, "iq_gather_augment: null output");
  SY11_REQUIRE(B > 0 && L > 0, "iq_gather_augment: B and L must be positive (B=%d L=%d)", B, L);
  SY11_REQUIRE(B <= 65535, "iq_gather_augment: B=%d exceeds 65535", B);
  SY11_REQUIRE((long)B * L < (1L << 31), "iq_gather_augment: B*L = %ld exceeds the int32 index range", (long)B * L);
  const dim3 grid(cdiv(cdiv(L, 2), 256), B);
  hipLaunchKernelGGL(iq_gather_augment_kernel, grid, dim3(256), 0, (hipStream_t)stream, L, src_ptr, src_off, r, (float2*)out);
  SY11_LAUNCH_CHECK("iq_gather_augment");
  return SY11_OK;
}
