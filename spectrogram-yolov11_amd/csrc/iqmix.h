// iqmix.h — the one mixer rotation of the IQ front end (ddc.hip, extract.hip).  There is exactly one copy: extract.hip promises the
// bits of ddc.hip, and that holds only while both call this function.
#pragma once
#include "common.h"

// z e^{j 2 pi phase / 2^32}, rounded ONCE: the float angle of rot_gain (iqaug.hip) keeps 24 of the phase's 32 bits, which alone costs
// 2e-7 of |z| — more than everything else in this file together.  So the rotation is evaluated in float64: the top two bits of the
// phase (rounded) are a quarter turn, exact as swaps and signs; the rest is an angle |a| <= pi / 4 whose sine and cosine are the
// Taylor polynomials to a^11 / a^12 (next terms 7e-12 / 4e-13); products and sums in float64, one rounding to float32 per component.
__device__ __forceinline__ float2 mix(float2 z, uint32_t phase) {
  const uint32_t q = (phase + 0x20000000u) >> 30;
  const double a = (double)(int32_t)(phase - (q << 30)) * 0x1.921fb54442d18p-30;      // pi / 2^31
  const double a2 = a * a;
  double s = a * (1.0 + a2 * (-1.0 / 6 + a2 * (1.0 / 120 + a2 * (-1.0 / 5040 + a2 * (1.0 / 362880 + a2 * (-1.0 / 39916800))))));
  double c = 1.0 + a2 * (-1.0 / 2 + a2 * (1.0 / 24 + a2 * (-1.0 / 720 + a2 * (1.0 / 40320 + a2 * (-1.0 / 3628800 + a2 * (1.0 / 479001600))))));
  if (q & 1u) { const double t = c; c = -s; s = t; }                      // + a quarter turn
  if (q & 2u) { c = -c; s = -s; }                                         // + half a turn
  const double x = z.x, y = z.y;
  return make_float2((float)(x * c - y * s), (float)(x * s + y * c));
}
