// link.hip — link the boxes of one emission into tracks (gfx950): connected components of the link relation of DESIGN.md §4
// over a scan's rows, in seconds / Hz, float64 throughout.
//
// Rows i != j are linked when their classes agree (any classes: agnostic) and
//   along time       ov_t >= -gap_t  and  ov_f >= align * min(bw_i, bw_j),   or
//   along frequency  ov_f >= -gap_f  and  ov_t >= align * min(dur_i, dur_j)          (only with use_f)
// with ov_t = min(t1) - max(t0), ov_f = min(f_hi) - max(f_lo), dur = t1 - t0, bw = f_hi - f_lo: subtract, min, max, one multiply
// that feeds a compare and nothing else — there is nothing to contract, so the host's numpy decides every pair identically.
//
// n reaches millions, so there is no n x n mask and no edge list: pairs are recomputed per pass, as in the seam merge (detect.hip).
// Rows arrive sorted by t0, hence the later partners of row i are the contiguous rows (i, hi[i]) with t0_j <= t1_i + gap_t (both
// branches need it: the frequency branch asks ov_t >= 0).  hi[i] comes from one binary search per row over a bound widened by an
// explicit relative slack; it is a superset and never decides a pair.
//
// Components by hook-and-compress.  label[i] starts as i and only ever decreases; label[i] <= i and label[i] is a row of i's
// component at all times.  A HOOK pass (one wave per row, 64 lanes striding its range) takes, per linked pair, the two labels —
// roots, because every pass starts fully compressed — and atomicMin's the smaller into the larger root's slot (the smaller root's
// slot already holds it).  COMPRESS is pointer jumping, eight hops per row per launch, so ceil(log8 n) launches flatten any forest
// of n rows and no flag has to be read for it.  A hook pass that meets no pair with two different labels wrote nothing, therefore
// read the true labels: they are constant on every component, and a compressed constant label that is a member and <= every member
// is the component's smallest row.  Integer atomicMin commutes, so this fixed point does not depend on scheduling; only the number
// of passes may.  Hooking ROOTS is what makes that number logarithmic: a long chain is one tree after the first pass.
// A label read inside a pass may be older than the newest store (another CU's L1): every value ever stored is a root of the pass's
// start and a member of the component, so an old one costs at most a further pass.
#include "common.h"

#include <float.h>

typedef double f64x2 __attribute__((ext_vector_type(2)));

enum { LINK_ROWS_PER_WG = 4, LINK_HOPS = 8, LINK_BATCH = 2 };

__device__ __forceinline__ int link_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void link_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// label[i] = i; hi[i] = one past the last later row that can be linked to row i
__global__ __launch_bounds__(256) void scan_link_ranges_kernel(int n, const f64x2* __restrict__ rect, double gap_t, int* __restrict__ label,
                                                               int* __restrict__ hi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double t1 = rect[2 * (size_t)i + 1][0];
  // ov_t >= -gap_t rounds once: a pair passes with t0_j at most half an ulp of the difference above t1 + gap_t.  1e-12 relative
  // is some 10^4 times that, and DBL_MIN covers an all-zero row.
  const double bound = (t1 + gap_t) + (1e-12 * (fabs(t1) + gap_t) + DBL_MIN);
  int a = i + 1, b = n;                                      // first row in [i + 1, n) with t0 > bound
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (rect[2 * (size_t)mid][0] <= bound) a = mid + 1; else b = mid;
  }
  label[i] = i;
  hi[i] = a;
}

__global__ __launch_bounds__(256) void scan_link_hook_kernel(int n, const f64x2* __restrict__ rect, const int* __restrict__ cls,
                                                             const int* __restrict__ hi, double gap_t, double gap_f, int use_f,
                                                             double align, int agnostic, int* label, int* changed) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * LINK_ROWS_PER_WG + (threadIdx.x >> 6);
  if (i >= n) return;                                        // wave-uniform from here on
  const int end = min(max(hi[i], i + 1), n);
  if (end <= i + 1) return;
  const f64x2 lo_i = rect[2 * (size_t)i], hi_i = rect[2 * (size_t)i + 1];
  const double t0i = lo_i[0], f0i = lo_i[1], t1i = hi_i[0], f1i = hi_i[1];
  const double dur_i = t1i - t0i, bw_i = f1i - f0i;
  const int ci = cls[i];
  const int a = link_load(label + i);
  bool any = false;
  for (int j = i + 1 + lane; j < end; j += 64) {
    if (!agnostic && cls[j] != ci) continue;
    const f64x2 lo_j = rect[2 * (size_t)j], hi_j = rect[2 * (size_t)j + 1];
    const double t0j = lo_j[0], f0j = lo_j[1], t1j = hi_j[0], f1j = hi_j[1];
    const double ov_t = fmin(t1i, t1j) - fmax(t0i, t0j);
    const double ov_f = fmin(f1i, f1j) - fmax(f0i, f0j);
    const double need_f = align * fmin(bw_i, f1j - f0j);
    bool linked = ov_t >= -gap_t && ov_f >= need_f;
    if (!linked && use_f) {
      const double need_t = align * fmin(dur_i, t1j - t0j);
      linked = ov_f >= -gap_f && ov_t >= need_t;
    }
    if (!linked) continue;
    const int b = link_load(label + j);
    if (a == b) continue;
    atomicMin(label + max(a, b), min(a, b));                 // both are rows below n: labels never leave [0, n)
    any = true;
  }
  if (__ballot(any) != 0 && lane == 0) *changed = 1;         // same value from every writer
}

// LINK_HOPS hops towards the root per row: a forest of depth d leaves this launch with depth <= ceil(d / LINK_HOPS)
__global__ __launch_bounds__(256) void scan_link_compress_kernel(int n, int* label) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int first = link_load(label + i);
  int r = first;
  for (int k = 1; k < LINK_HOPS; ++k) {
    const int up = link_load(label + r);
    if (up == r) break;
    r = up;
  }
  if (r != first) link_store(label + i, r);
}

static inline size_t link_align16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" size_t sy11_scan_link_workspace_bytes(int32_t n) {
  if (n <= 0) return 0;
  return 16 + link_align16((size_t)n * 4);                   // the changed flags of a batch of passes, then hi (n)
}

extern "C" int sy11_scan_link(int32_t n, const double* rect, const int32_t* cls, double gap_t, double gap_f, int32_t use_f, double align,
                              int32_t agnostic, void* workspace, int32_t* label, int32_t* passes, void* stream) {
  SY11_REQUIRE(n >= 0, "scan_link: n must not be negative");
  SY11_REQUIRE(gap_t >= 0 && gap_t <= DBL_MAX, "scan_link: gap_t must be finite and >= 0");
  SY11_REQUIRE(!use_f || (gap_f >= 0 && gap_f <= DBL_MAX), "scan_link: gap_f must be finite and >= 0");
  SY11_REQUIRE(align > 0 && align <= 1, "scan_link: align must lie in (0, 1]");
  if (passes) *passes = 0;
  if (n == 0) return SY11_OK;
  SY11_REQUIRE(rect && cls && workspace && label, "scan_link: null pointer");
  SY11_REQUIRE(((uintptr_t)rect & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "scan_link: rect and workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int* flags = (int*)workspace;
  int* hi = (int*)((char*)workspace + 16);
  if (!use_f) gap_f = 0.0;
  int jumps = 1;                                             // LINK_HOPS ^ jumps >= n: enough launches for the deepest forest of n rows
  for (long reach = LINK_HOPS; reach < n; reach *= LINK_HOPS) ++jumps;
  hipLaunchKernelGGL(scan_link_ranges_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, (const f64x2*)rect, gap_t, label, hi);
  SY11_LAUNCH_CHECK("scan_link (ranges)");
  // Every pass that changes something hooks at least one root under another, so n passes always suffice.  One host read per batch.
  for (long pass = 0; pass < (long)n + LINK_BATCH; pass += LINK_BATCH) {
    if (hipMemsetAsync(flags, 0, 16, st) != hipSuccess) SY11_FAIL(SY11_ELAUNCH, "scan_link: memset failed");
    for (int k = 0; k < LINK_BATCH; ++k) {
      hipLaunchKernelGGL(scan_link_hook_kernel, dim3(cdiv(n, LINK_ROWS_PER_WG)), dim3(256), 0, st, n, (const f64x2*)rect, cls, hi, gap_t, gap_f,
                         use_f ? 1 : 0, align, agnostic ? 1 : 0, label, flags + k);
      SY11_LAUNCH_CHECK("scan_link (hook)");
      for (int c = 0; c < jumps; ++c) {
        hipLaunchKernelGGL(scan_link_compress_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, label);
        SY11_LAUNCH_CHECK("scan_link (compress)");
      }
    }
    int changed[LINK_BATCH] = {0};
    if (hipMemcpyAsync(changed, flags, sizeof(changed), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      SY11_FAIL(SY11_ELAUNCH, "scan_link: reading the changed flags failed: %s", hipGetErrorString(hipGetLastError()));
    if (passes) *passes = (int32_t)(pass + LINK_BATCH);
    if (!changed[LINK_BATCH - 1]) return SY11_OK;            // a later pass of the batch changes nothing once an earlier one did not
  }
  SY11_FAIL(SY11_ELAUNCH, "scan_link: no fixed point after n passes");
}
