// detect.hip — Detect._inference decode (DFL expectation + dist2bbox + sigmoid) and greedy NMS for gfx950.
//
// decode: replaces nn/modules/head.py:100-131 (+ block.py:80 DFL, utils/tal.py:349-358 dist2bbox): one thread per
// (image, anchor); reads the NHWC f32 head maps, writes the reference's (B, 4+nc, A) layout coalesced over anchors.
// nms: replaces torchvision.ops.nms as called from utils/ops.py:312.  Candidates arrive sorted (score desc, index asc);
// kernel 1 builds the n x n/64 suppression bit matrix (IoU > thr, strict) with one wave ballot per 64 columns,
// kernel 2 is the serial greedy sweep held by ONE wave (removed-mask words in LDS), so the kept set is exactly the
// sequential algorithm's: bit-exact indices.  IoU arithmetic is plain f32 without contraction so it matches the oracle.
#include "common.h"

struct DecodeArgs {
  const float* maps[8];
  int hs[8], ws[8], a0[8], c0[8];     // c0 = first 64-anchor chunk of the level inside one image
  float strides[8];
  int B, nc, nl, A, chunks;           // chunks = 64-anchor chunks per image
  float* out;
};

// One workgroup = 64 consecutive anchors of one (image, level).  Their rows (64 x (64 + nc) f32, contiguous in the NHWC map)
// are staged through LDS with coalesced 16-byte loads — a thread per anchor walking its own 576-byte row touched 64 cache
// lines per load instruction — then thread (anchor, side) does one DFL expectation and the class sigmoids are written
// anchor-fastest, which is the reference's (B, 4+nc, A) layout.  Arithmetic and its order are those of the scalar form.
__global__ __launch_bounds__(256) void detect_decode_kernel(const DecodeArgs a) {
  extern __shared__ float rows[];                        // [64][no + 1]
  __shared__ float dist[64][4];
  const int b = blockIdx.x / a.chunks, ch = blockIdx.x - b * a.chunks;
  int l = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i)
    if (i < a.nl && ch >= a.c0[i]) l = i;
  const int W = a.ws[l], HW = a.hs[l] * W;
  const int loc0 = (ch - a.c0[l]) * 64;
  const int n_an = min(64, HW - loc0);
  const int no = 64 + a.nc, ld = no + 1;
  const float* src = a.maps[l] + ((long)b * HW + loc0) * no;
  const int total = n_an * no;
  if ((no & 3) == 0 && (((uintptr_t)src) & 15) == 0) {
    for (int i = threadIdx.x * 4; i < total; i += 1024) {
      const float4 v = *(const float4*)(src + i);
      const int r = i / no, c = i - r * no;                // no % 4 == 0: the four values stay in one row
      float* d = rows + r * ld + c;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    for (int i = threadIdx.x; i < total; i += 256) { const int r = i / no; rows[r * ld + (i - r * no)] = src[i]; }
  }
  __syncthreads();
  const int an = threadIdx.x & 63, side = threadIdx.x >> 6;
  if (an < n_an) {
    const float* v0 = rows + an * ld + side * 16;
    float v[16], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 16; ++k) { v[k] = v0[k]; mx = fmaxf(mx, v[k]); }
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const float e = expf(v[k] - mx); den += e; num += e * (float)k; }
    dist[an][side] = num / den;
  }
  __syncthreads();
  if (an >= n_an) return;
  const int loc = loc0 + an;
  float* o = a.out + (long)b * (4 + a.nc) * a.A + a.a0[l] + loc;
  if (side == 0) {
    const int gy = loc / W, gx = loc - gy * W;
    const float ax = gx + 0.5f, ay = gy + 0.5f, st = a.strides[l];
    const float x1 = ax - dist[an][0], y1 = ay - dist[an][1], x2 = ax + dist[an][2], y2 = ay + dist[an][3];
    o[0] = (x1 + x2) * 0.5f * st;
    o[(long)a.A] = (y1 + y2) * 0.5f * st;
    o[2L * a.A] = (x2 - x1) * st;
    o[3L * a.A] = (y2 - y1) * st;
  }
  const float* cls = rows + an * ld + 64;
  for (int c = side; c < a.nc; c += 4) o[(long)(4 + c) * a.A] = 1.f / (1.f + expf(-cls[c]));
}

extern "C" int sy11_detect_decode(int32_t B, int32_t nc, int32_t nl, const float* const* maps, const int32_t* hs,
                                  const int32_t* ws, const float* strides, float* out, void* stream) {
  SY11_REQUIRE(B > 0 && nc > 0 && nl > 0 && nl <= 8 && maps && hs && ws && strides && out, "detect_decode: bad argument");
  DecodeArgs a{};
  int A = 0, chunks = 0;
  for (int i = 0; i < nl; ++i) {
    SY11_REQUIRE(maps[i] && hs[i] > 0 && ws[i] > 0, "detect_decode: bad level %d", i);
    a.maps[i] = maps[i]; a.hs[i] = hs[i]; a.ws[i] = ws[i]; a.strides[i] = strides[i]; a.a0[i] = A; a.c0[i] = chunks;
    A += hs[i] * ws[i];
    chunks += cdiv(hs[i] * ws[i], 64);
  }
  SY11_REQUIRE((long)B * A < (1L << 31) && (long)B * chunks < (1L << 31), "detect_decode: too many anchors");
  const size_t lds = (size_t)64 * (64 + nc + 1) * sizeof(float);
  SY11_REQUIRE(lds <= 60 * 1024, "detect_decode: nc=%d needs %zu bytes of LDS per workgroup (max 61440)", nc, lds);
  a.B = B; a.nc = nc; a.nl = nl; a.A = A; a.chunks = chunks; a.out = out;
  hipLaunchKernelGGL(detect_decode_kernel, dim3((unsigned)(B * chunks)), dim3(256), lds, (hipStream_t)stream, a);
  SY11_LAUNCH_CHECK("detect_decode");
  return SY11_OK;
}

// ------------------------------------------------------------------------------------------------ NMS
__global__ __launch_bounds__(64) void nms_mask_kernel(int n, int nw, const float* __restrict__ boxes, float thr, uint64_t* __restrict__ mask) {
#pragma clang fp contract(off)
  // block (cb, rb): rows rb*64..+63 (one per lane), column word cb
  const int cb = blockIdx.x, rb = blockIdx.y;
  if (cb < rb) return;   // only j > i can be suppressed by i; words left of the diagonal stay zero (pre-cleared)
  __shared__ float cbx[64][4];
  const int lane = threadIdx.x;
  const int cj = cb * 64 + lane;
  if (cj < n) { cbx[lane][0] = boxes[cj * 4]; cbx[lane][1] = boxes[cj * 4 + 1]; cbx[lane][2] = boxes[cj * 4 + 2]; cbx[lane][3] = boxes[cj * 4 + 3]; }
  __syncthreads();
  const int i = rb * 64 + lane;
  if (i >= n) return;
  const float x1 = boxes[i * 4], y1 = boxes[i * 4 + 1], x2 = boxes[i * 4 + 2], y2 = boxes[i * 4 + 3];
  const float ai = (x2 - x1) * (y2 - y1);
  uint64_t bits = 0;
  const int jmax = min(64, n - cb * 64);
  for (int j = 0; j < jmax; ++j) {
    const int gj = cb * 64 + j;
    if (gj <= i) continue;
    const float xx1 = fmaxf(x1, cbx[j][0]), yy1 = fmaxf(y1, cbx[j][1]);
    const float xx2 = fminf(x2, cbx[j][2]), yy2 = fminf(y2, cbx[j][3]);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    const float aj = (cbx[j][2] - cbx[j][0]) * (cbx[j][3] - cbx[j][1]);
    const float iou = inter / (ai + aj - inter);
    if (iou > thr) bits |= (1ull << j);
  }
  mask[(long)i * nw + cb] = bits;
}

__global__ __launch_bounds__(64) void nms_sweep_kernel(int n, int nw, const uint64_t* __restrict__ mask, uint8_t* __restrict__ keep) {
  extern __shared__ uint64_t removed[];
  const int lane = threadIdx.x;
  for (int w = lane; w < nw; w += 64) removed[w] = 0;
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const uint64_t r = removed[i >> 6];            // wave-uniform read
    const bool dead = (r >> (i & 63)) & 1;
    if (lane == 0) keep[i] = dead ? 0 : 1;
    if (!dead) {
      const uint64_t* row = mask + (long)i * nw;
      for (int w = (i >> 6) + lane; w < nw; w += 64) removed[w] |= row[w];
    }
    __syncthreads();
  }
}

extern "C" size_t sy11_nms_workspace_bytes(int32_t n) { return n <= 0 ? 0 : (size_t)n * ((n + 63) / 64) * sizeof(uint64_t); }

extern "C" int sy11_nms_sorted(int32_t n, const float* boxes, float iou_thres, uint64_t* workspace, uint8_t* keep, void* stream) {
  SY11_REQUIRE(n >= 0, "nms_sorted: negative n");
  if (n == 0) return SY11_OK;
  SY11_REQUIRE(boxes && workspace && keep, "nms_sorted: null pointer");
  SY11_REQUIRE(n <= 65535 * 64, "nms_sorted: n too large");
  const int nw = (n + 63) / 64;
  SY11_REQUIRE((size_t)nw * 8 <= 64 * 1024, "nms_sorted: n=%d exceeds the LDS removed-mask", n);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, sy11_nms_workspace_bytes(n), st) != hipSuccess) SY11_FAIL(SY11_ELAUNCH, "nms_sorted: memset failed");
  hipLaunchKernelGGL(nms_mask_kernel, dim3(nw, nw), dim3(64), 0, st, n, nw, boxes, iou_thres, workspace);
  hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(64), (size_t)nw * 8, st, n, nw, (const uint64_t*)workspace, keep);
  SY11_LAUNCH_CHECK("nms_sorted");
  return SY11_OK;
}

// ---- batched form: up to NMS_SEGS images per launch, each a contiguous run of rows of `boxes` (score-descending inside the run).
// The per-image work is unchanged (same IoU arithmetic, same greedy order => the same kept set, bit for bit); what changes is that
// the images run side by side — the greedy sweep is ONE wave per image and latency-bound (a dependent global row read per
// surviving box), so 64 images in one launch take the time of the slowest instead of the sum — and that the sweep stops after
// `max_keep` survivors (the callers keep at most max_det rows per image: ops.py:322), the rest of `keep` is cleared.
#define NMS_SEGS 128
struct NmsSegs {
  int start[NMS_SEGS];          // first row of the segment in boxes / keep
  int n[NMS_SEGS];              // rows
  long ws[NMS_SEGS];            // first mask word of the segment in the workspace
  int count;
};
__global__ __launch_bounds__(64) void nms_mask_batched_kernel(const NmsSegs sg, const float* __restrict__ boxes_all, float thr, uint64_t* __restrict__ mask_all) {
#pragma clang fp contract(off)
  const int seg = blockIdx.z, n = sg.n[seg], nw = (n + 63) >> 6;
  const int cb = blockIdx.x, rb = blockIdx.y;
  if (cb >= nw || rb >= nw) return;
  const float* boxes = boxes_all + (long)sg.start[seg] * 4;
  uint64_t* mask = mask_all + sg.ws[seg];
  const int lane = threadIdx.x;
  const int i = rb * 64 + lane;
  if (cb < rb) {                                   // left of the diagonal: j <= i never suppressed by i; written, so no memset pass is needed
    if (i < n) mask[(long)i * nw + cb] = 0;
    return;
  }
  __shared__ float cbx[64][4];
  const int cj = cb * 64 + lane;
  if (cj < n) { cbx[lane][0] = boxes[cj * 4]; cbx[lane][1] = boxes[cj * 4 + 1]; cbx[lane][2] = boxes[cj * 4 + 2]; cbx[lane][3] = boxes[cj * 4 + 3]; }
  __syncthreads();
  if (i >= n) return;
  const float x1 = boxes[i * 4], y1 = boxes[i * 4 + 1], x2 = boxes[i * 4 + 2], y2 = boxes[i * 4 + 3];
  const float ai = (x2 - x1) * (y2 - y1);
  uint64_t bits = 0;
  const int jmax = min(64, n - cb * 64);
  for (int j = 0; j < jmax; ++j) {
    const int gj = cb * 64 + j;
    if (gj <= i) continue;
    const float xx1 = fmaxf(x1, cbx[j][0]), yy1 = fmaxf(y1, cbx[j][1]);
    const float xx2 = fminf(x2, cbx[j][2]), yy2 = fminf(y2, cbx[j][3]);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    const float aj = (cbx[j][2] - cbx[j][0]) * (cbx[j][3] - cbx[j][1]);
    const float iou = inter / (ai + aj - inter);
    if (iou > thr) bits |= (1ull << j);
  }
  mask[(long)i * nw + cb] = bits;
}

__global__ __launch_bounds__(64) void nms_sweep_batched_kernel(const NmsSegs sg, const uint64_t* __restrict__ mask_all, uint8_t* __restrict__ keep_all, int max_keep) {
  extern __shared__ uint64_t removed[];
  const int seg = blockIdx.x, n = sg.n[seg], nw = (n + 63) >> 6;
  const uint64_t* mask = mask_all + sg.ws[seg];
  uint8_t* keep = keep_all + sg.start[seg];
  const int lane = threadIdx.x;
  for (int w = lane; w < nw; w += 64) removed[w] = 0;
  __syncthreads();
  int kept = 0, i = 0;
  for (; i < n && kept < max_keep; ++i) {
    const uint64_t r = removed[i >> 6];            // wave-uniform read
    const bool dead = (r >> (i & 63)) & 1;
    if (lane == 0) keep[i] = dead ? 0 : 1;
    if (!dead) {
      ++kept;
      const uint64_t* row = mask + (long)i * nw;
      for (int w = (i >> 6) + lane; w < nw; w += 64) removed[w] |= row[w];
    }
    __syncthreads();
  }
  for (int j = i + lane; j < n; j += 64) keep[j] = 0;            // past the max_keep-th survivor: never reported
}

extern "C" size_t sy11_nms_batched_workspace_bytes(int32_t nseg, const int32_t* counts) {
  size_t words = 0;
  for (int i = 0; i < nseg; ++i) words += counts[i] > 0 ? (size_t)counts[i] * ((counts[i] + 63) / 64) : 0;
  return words * sizeof(uint64_t);
}

extern "C" int sy11_nms_sorted_batched(int32_t nseg, const int32_t* counts, const float* boxes, float iou_thres, int32_t max_keep, uint64_t* workspace,
                                       uint8_t* keep, void* stream) {
  SY11_REQUIRE(nseg >= 0 && (nseg == 0 || counts), "nms_sorted_batched: bad segment list");
  SY11_REQUIRE(max_keep > 0, "nms_sorted_batched: max_keep must be positive");
  hipStream_t st = (hipStream_t)stream;
  long row = 0, word = 0;
  for (int s0 = 0; s0 < nseg; s0 += NMS_SEGS) {
    NmsSegs sg{};
    int max_nw = 0;
    for (int s = s0; s < nseg && s < s0 + NMS_SEGS; ++s) {
      const int n = counts[s];
      SY11_REQUIRE(n >= 0 && n <= 65535 * 64, "nms_sorted_batched: segment %d has %d rows", s, n);
      const int nw = (n + 63) / 64;
      SY11_REQUIRE((size_t)nw * 8 <= 64 * 1024, "nms_sorted_batched: n=%d exceeds the LDS removed-mask", n);
      sg.start[sg.count] = (int)row; sg.n[sg.count] = n; sg.ws[sg.count] = word;
      row += n; word += (long)n * nw;
      SY11_REQUIRE(row < (1L << 31), "nms_sorted_batched: too many rows");
      if (nw > max_nw) max_nw = nw;
      ++sg.count;
    }
    if (max_nw == 0) continue;
    SY11_REQUIRE(boxes && workspace && keep, "nms_sorted_batched: null pointer");
    hipLaunchKernelGGL(nms_mask_batched_kernel, dim3(max_nw, max_nw, sg.count), dim3(64), 0, st, sg, boxes, iou_thres, workspace);
    hipLaunchKernelGGL(nms_sweep_batched_kernel, dim3(sg.count), dim3(64), (size_t)max_nw * 8, st, sg, (const uint64_t*)workspace, keep, max_keep);
  }
  SY11_LAUNCH_CHECK("nms_sorted_batched");
  return SY11_OK;
}


// ---- segments given by DEVICE arrays (r04): seg_start[s] .. seg_start[s + 1] are the rows of segment s (score-descending), seg_ws[s] its first
// mask word.  Used with one segment per (image, CLASS): the reference suppresses all classes of an image in one torchvision.ops.nms call
// by shifting every box by class * max_wh (utils/ops.py:307-312), so boxes of different classes never intersect and the greedy sweep
// over the whole image keeps exactly what independent sweeps per class keep — but the image-wide bit matrix tests n^2 / 2 pairs
// (6 723 candidates per image at conf 0.001: 1.4 G pairs per 64 images, 1.1 ms) where the per-class matrices test n^2 / (2 nc).
// The IoU arithmetic is unchanged (the SHIFTED boxes, same operation order): the kept set is bit-identical.
__global__ __launch_bounds__(64) void nms_mask_seg_kernel(const int* __restrict__ seg_start, const long long* __restrict__ seg_ws,
                                                          const float* __restrict__ boxes_all, float thr, uint64_t* __restrict__ mask_all) {
#pragma clang fp contract(off)
  const int seg = blockIdx.z, r0 = seg_start[seg], n = seg_start[seg + 1] - r0, nw = (n + 63) >> 6;
  const int cb = blockIdx.x, rb = blockIdx.y;
  if (cb >= nw || rb >= nw) return;
  const float* boxes = boxes_all + (long)r0 * 4;
  uint64_t* mask = mask_all + seg_ws[seg];
  const int lane = threadIdx.x;
  const int i = rb * 64 + lane;
  if (cb < rb) {
    if (i < n) mask[(long)i * nw + cb] = 0;
    return;
  }
  __shared__ float cbx[64][4];
  const int cj = cb * 64 + lane;
  if (cj < n) { cbx[lane][0] = boxes[cj * 4]; cbx[lane][1] = boxes[cj * 4 + 1]; cbx[lane][2] = boxes[cj * 4 + 2]; cbx[lane][3] = boxes[cj * 4 + 3]; }
  __syncthreads();
  if (i >= n) return;
  const float x1 = boxes[i * 4], y1 = boxes[i * 4 + 1], x2 = boxes[i * 4 + 2], y2 = boxes[i * 4 + 3];
  const float ai = (x2 - x1) * (y2 - y1);
  uint64_t bits = 0;
  const int jmax = min(64, n - cb * 64);
  for (int j = 0; j < jmax; ++j) {
    const int gj = cb * 64 + j;
    if (gj <= i) continue;
    const float xx1 = fmaxf(x1, cbx[j][0]), yy1 = fmaxf(y1, cbx[j][1]);
    const float xx2 = fminf(x2, cbx[j][2]), yy2 = fminf(y2, cbx[j][3]);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    const float aj = (cbx[j][2] - cbx[j][0]) * (cbx[j][3] - cbx[j][1]);
    const float iou = inter / (ai + aj - inter);
    if (iou > thr) bits |= (1ull << j);
  }
  mask[(long)i * nw + cb] = bits;
}

__global__ __launch_bounds__(64) void nms_sweep_seg_kernel(const int* __restrict__ seg_start, const long long* __restrict__ seg_ws,
                                                           const uint64_t* __restrict__ mask_all, uint8_t* __restrict__ keep_all, int max_keep) {
  extern __shared__ uint64_t removed[];
  const int seg = blockIdx.x, r0 = seg_start[seg], n = seg_start[seg + 1] - r0, nw = (n + 63) >> 6;
  if (n <= 0) return;
  const uint64_t* mask = mask_all + seg_ws[seg];
  uint8_t* keep = keep_all + r0;
  const int lane = threadIdx.x;
  for (int w = lane; w < nw; w += 64) removed[w] = 0;
  __syncthreads();
  int kept = 0, i = 0;
  for (; i < n && kept < max_keep; ++i) {
    const uint64_t r = removed[i >> 6];
    const bool dead = (r >> (i & 63)) & 1;
    if (lane == 0) keep[i] = dead ? 0 : 1;
    if (!dead) {
      ++kept;
      const uint64_t* row = mask + (long)i * nw;
      for (int w = (i >> 6) + lane; w < nw; w += 64) removed[w] |= row[w];
    }
    __syncthreads();
  }
  for (int j = i + lane; j < n; j += 64) keep[j] = 0;
}

extern "C" int sy11_nms_sorted_segments(int32_t nseg, const int32_t* seg_start, const int64_t* seg_ws, int32_t max_n, const float* boxes,
                                        float iou_thres, int32_t max_keep, uint64_t* workspace, uint8_t* keep, void* stream) {
  SY11_REQUIRE(nseg >= 0 && max_n >= 0 && max_keep > 0, "nms_sorted_segments: bad argument");
  if (nseg == 0 || max_n == 0) return SY11_OK;
  SY11_REQUIRE(seg_start && seg_ws && boxes && workspace && keep, "nms_sorted_segments: null pointer");
  const int max_nw = (max_n + 63) / 64;
  SY11_REQUIRE((size_t)max_nw * 8 <= 64 * 1024, "nms_sorted_segments: a segment of %d rows exceeds the LDS removed-mask", max_n);
  SY11_REQUIRE(max_nw <= 65535, "nms_sorted_segments: segment too long");
  hipStream_t st = (hipStream_t)stream;
  for (int s0 = 0; s0 < nseg; s0 += 65535) {                   // grid.z limit
    const int ns = nseg - s0 < 65535 ? nseg - s0 : 65535;
    hipLaunchKernelGGL(nms_mask_seg_kernel, dim3(max_nw, max_nw, ns), dim3(64), 0, st, seg_start + s0, (const long long*)seg_ws + s0, boxes, iou_thres, workspace);
    hipLaunchKernelGGL(nms_sweep_seg_kernel, dim3(ns), dim3(64), (size_t)max_nw * 8, st, seg_start + s0, (const long long*)seg_ws + s0,
                       (const uint64_t*)workspace, keep, max_keep);
  }
  SY11_LAUNCH_CHECK("nms_sorted_segments");
  return SY11_OK;
}


// ------------------------------------------------------------------------------------------------ NMS candidates (r04)
// non_max_suppression's candidate selection (utils/ops.py:246-292) on the prediction tensor AS Detect returns it, (B, 4 + nc + nm, A)
// with the anchors contiguous: a thread owns one anchor and walks its class scores (coalesced across the workgroup), so the
// (B, A, 4 + nc) transposed copy, the boolean mask, torch.nonzero and the score gather of the r03 wrapper are never materialised.
// Candidates come out in the reference's order — image, then anchor, then class — which is what makes the later STABLE sort by
// (image, score descending) reproduce torchvision's tie order: two passes (count per 256-anchor block; exclusive scan on the host
// side of the call as one torch.cumsum; write at the scanned offsets).  key = segment << 32 | ~bits(score): scores above a threshold
// >= 0 are positive floats, whose bit patterns order like the values; segment = image, or image * nc + class (see the segment kernels).
template <bool WRITE>
__global__ __launch_bounds__(256) void nms_candidates_kernel(int D, int A, int nc, float thr, int multi, const float* __restrict__ pred,
                                                             const int* __restrict__ blk_offset, int* __restrict__ blk_count,
                                                             long long* __restrict__ key, int* __restrict__ anchor, int* __restrict__ cls, int seg_nc) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, a0 = blockIdx.x * 256, a = a0 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = a < A;
  const float* sc = pred + ((long)b * D + 4) * A + (live ? a : 0);
  int cnt = 0, arg = 0;
  float best = -INFINITY;
  if (live) {
    if (multi) {
      for (int c = 0; c < nc; ++c) cnt += sc[(long)c * A] > thr ? 1 : 0;
    } else {
      for (int c = 0; c < nc; ++c) {
        const float v = sc[(long)c * A];
        if (v > best) { best = v; arg = c; }           // strict: the first maximum wins
      }
      cnt = best > thr ? 1 : 0;
    }
  }
  // inclusive scan of the per-thread counts inside the wave, then across the four waves
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wsum[w];
  if (!WRITE) {
    if (threadIdx.x == 255) blk_count[b * gridDim.x + blockIdx.x] = before + incl;
    return;
  }
  long o = (long)blk_offset[b * gridDim.x + blockIdx.x] + before + incl - cnt;
  if (!live || cnt == 0) return;
  if (multi) {
    for (int c = 0; c < nc; ++c) {
      const float v = sc[(long)c * A];
      if (v > thr) {
        key[o] = ((long long)(seg_nc ? b * seg_nc + c : b) << 32) | (long long)(unsigned)(~__float_as_uint(v));
        anchor[o] = a; cls[o] = c;
        ++o;
      }
    }
  } else {
    key[o] = ((long long)(seg_nc ? b * seg_nc + arg : b) << 32) | (long long)(unsigned)(~__float_as_uint(best));
    anchor[o] = a; cls[o] = arg;
  }
}

extern "C" int sy11_nms_candidates(int32_t B, int32_t D, int32_t A, int32_t nc, float conf_thres, int32_t multi_label, int32_t segment_by_class,
                                   const float* pred, const int32_t* blk_offset, int32_t* blk_count, int64_t* key, int32_t* anchor, int32_t* cls,
                                   void* stream) {
  SY11_REQUIRE(B > 0 && B <= 65535 && A > 0 && nc > 0 && D >= 4 + nc, "nms_candidates: bad dims (B %d, D %d, A %d, nc %d)", B, D, A, nc);
  SY11_REQUIRE(conf_thres >= 0.f, "nms_candidates: the threshold must be >= 0 (score bits are ordered as integers)");
  SY11_REQUIRE(pred != nullptr, "nms_candidates: null prediction");
  SY11_REQUIRE(!segment_by_class || (long)B * nc < (1L << 31), "nms_candidates: B * nc overflows the segment id");
  const int seg_nc = segment_by_class ? nc : 0;
  const dim3 grid(cdiv(A, 256), B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (blk_offset == nullptr) {                       // pass 1: candidates per (image, 256-anchor block), image-major
    SY11_REQUIRE(blk_count != nullptr, "nms_candidates: count pass without blk_count");
    hipLaunchKernelGGL((nms_candidates_kernel<false>), grid, block, 0, st, D, A, nc, conf_thres, multi_label, pred, nullptr, blk_count, nullptr, nullptr, nullptr, seg_nc);
  } else {                                           // pass 2: write at the exclusive prefix of those counts
    SY11_REQUIRE(key && anchor && cls, "nms_candidates: write pass without outputs");
    hipLaunchKernelGGL((nms_candidates_kernel<true>), grid, block, 0, st, D, A, nc, conf_thres, multi_label, pred, blk_offset, nullptr, (long long*)key, anchor, cls, seg_nc);
  }
  SY11_LAUNCH_CHECK("nms_candidates");
  return SY11_OK;
}


// ------------------------------------------------------------------------------------------------ pairwise IoU
// box_iou of the validator (utils/metrics.py:52-72): out[i][j] = inter / (area_a[i] + area_b[j] - inter + eps), every
// operation a separate f32 rounding in the reference's order (contraction is off for this file region) so the matrix —
// and with it the TP assignment at the 10 IoU thresholds — is bit-identical to the ATen element-wise evaluation.
__global__ __launch_bounds__(256) void box_iou_kernel(int n, int m, const float* __restrict__ a, const float* __restrict__ b, float eps,
                                                      float* __restrict__ out) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * m) return;
  const int i = (int)(idx / m), j = (int)(idx - (long)i * m);
  const float ax1 = a[i * 4], ay1 = a[i * 4 + 1], ax2 = a[i * 4 + 2], ay2 = a[i * 4 + 3];
  const float bx1 = b[j * 4], by1 = b[j * 4 + 1], bx2 = b[j * 4 + 2], by2 = b[j * 4 + 3];
  // every product goes through an empty asm so the backend cannot fuse it into the following add (-ffp-contract=fast
  // fuses at instruction selection whatever the source-level pragma says; the reference rounds each step)
  const float w = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
  const float h = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  float inter = w * h, area_a = (ax2 - ax1) * (ay2 - ay1), area_b = (bx2 - bx1) * (by2 - by1);
  asm volatile("" : "+v"(inter), "+v"(area_a), "+v"(area_b));
  out[idx] = inter / (((area_a + area_b) - inter) + eps);
}

extern "C" int sy11_box_iou(int32_t n, int32_t m, const float* a, const float* b, float eps, float* out, void* stream) {
  SY11_REQUIRE(n >= 0 && m >= 0, "box_iou: negative count");
  if (n == 0 || m == 0) return SY11_OK;
  SY11_REQUIRE(a && b && out, "box_iou: null pointer");
  const long tot = (long)n * m;
  hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, m, a, b, eps, out);
  SY11_LAUNCH_CHECK("box_iou");
  return SY11_OK;
}

// ---- seam merge of a long-capture scan ------------------------------------------------------------------------------------------
// The per-window NMS survivors of every window of a scan, greedily suppressed across windows in STRIP coordinates (X = start[w] + x):
// visit boxes by (score descending, row ascending); a box is dropped when an already-kept box of its class (any class: agnostic)
// has metric > thres with it.  n reaches millions, so there is no n x n mask.  Rows are grouped by window and windows are ordered
// by start, hence the possible partners of a box (windows whose start is less than n_frames away) are ONE contiguous row range,
// found once per window.  The greedy result is reached as a fixed point: per pass, one wave per undecided box walks its range and
// tests the better-ranked partners — KEPT once none of them that is over the threshold is kept or undecided, DROPPED once one is
// kept.  A decision, once made, is the greedy one (induction over the rank), the best-ranked undecided box is decided in every
// pass, and a pass reads the states of the previous pass only (two state arrays), so neither the result nor the number of passes
// depends on scheduling.  Pairs are recomputed per pass instead of stored: memory is O(n).
// start reaches 1e7 frames and beyond, where f32 loses the sub-pixel part: a pair is evaluated relative to the window of the box
// being decided (the integer frame delta, |delta| < n_frames, added to the local x) in f64, which makes both exact.
enum { SCAN_UNDECIDED = 0, SCAN_KEPT = 1, SCAN_DROPPED = 2 };

__global__ __launch_bounds__(256) void scan_row_offsets_kernel(int n, int W, const int* __restrict__ win, int* __restrict__ off) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cur = min(max(win[i], -1), W - 1);
  const int prev = i == 0 ? -1 : min(max(win[i - 1], -1), W - 1);
  for (int w = prev + 1; w <= cur; ++w) off[w] = i;          // first row of every window in (prev, cur]
  if (i == n - 1) for (int w = cur + 1; w <= W; ++w) off[w] = n;
}

__global__ __launch_bounds__(256) void scan_row_ranges_kernel(int n, int W, int n_frames, const long long* __restrict__ start,
                                                              const int* __restrict__ off, int* __restrict__ rlo, int* __restrict__ rhi) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const long long s = start[w];
  int a = w, b = w;
  while (a > 0 && s - start[a - 1] < n_frames) --a;
  while (b + 1 < W && start[b + 1] - s < n_frames) ++b;
  rlo[w] = min(max(off[a], 0), n);
  rhi[w] = min(max(off[b + 1], 0), n);
}

__global__ __launch_bounds__(256) void scan_merge_pass_kernel(int n, int W, int n_frames, const int* __restrict__ win, const f32x4* __restrict__ boxes,
                                                              const float* __restrict__ score, const int* __restrict__ cls,
                                                              const long long* __restrict__ start, const int* __restrict__ rlo,
                                                              const int* __restrict__ rhi, int use_ios, double thres, int agnostic,
                                                              const uint8_t* __restrict__ sin, uint8_t* __restrict__ sout,
                                                              uint8_t* __restrict__ keep, int* __restrict__ pending) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                        // wave-uniform from here on
  const uint8_t s0 = sin[i];
  if (s0 != SCAN_UNDECIDED) { if (lane == 0) sout[i] = s0; return; }
  const int w = win[i];
  if (w < 0 || w >= W) { if (lane == 0) { sout[i] = SCAN_DROPPED; keep[i] = 0; } return; }
  const f32x4 bi = boxes[i];
  const float si = score[i];
  const int ci = cls[i];
  const long long sw = start[w];
  const double ix1 = bi[0], iy1 = bi[1], ix2 = bi[2], iy2 = bi[3];
  const double ai = (ix2 - ix1) * (iy2 - iy1);
  bool drop = false, pend = false;
  const int lo = rlo[w], hi = rhi[w];
  for (int j = lo + lane; j < hi; j += 64) {
    if (j == i) continue;
    const float sj = score[j];
    if (!(sj > si || (sj == si && j < i))) continue;         // only better-ranked boxes can suppress
    if (!agnostic && cls[j] != ci) continue;
    const uint8_t stj = sin[j];
    if (stj == SCAN_DROPPED) continue;
    const int wj = win[j];
    if (wj < 0 || wj >= W) continue;
    const long long d = start[wj] - sw;
    if (d <= -(long long)n_frames || d >= (long long)n_frames) continue;
    const f32x4 bj = boxes[j];
    const double jx1 = (double)bj[0] + (double)d, jx2 = (double)bj[2] + (double)d, jy1 = bj[1], jy2 = bj[3];
    const double iw = fmax(0.0, fmin(ix2, jx2) - fmax(ix1, jx1)), ih = fmax(0.0, fmin(iy2, jy2) - fmax(iy1, jy1));
    const double inter = iw * ih;
    const double aj = (jx2 - jx1) * (jy2 - jy1);
    const double metric = use_ios ? inter / fmin(ai, aj) : inter / (ai + aj - inter);
    if (!(metric > thres)) continue;
    if (stj == SCAN_KEPT) drop = true; else pend = true;
  }
  const bool any_drop = __ballot(drop) != 0, any_pend = __ballot(pend) != 0;
  if (lane == 0) {
    if (any_drop) { sout[i] = SCAN_DROPPED; keep[i] = 0; }
    else if (!any_pend) { sout[i] = SCAN_KEPT; keep[i] = 1; }
    else { sout[i] = SCAN_UNDECIDED; *pending = 1; }          // same value from every writer
  }
}

static inline size_t scan_align16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" size_t sy11_scan_merge_workspace_bytes(int32_t n, int32_t W) {
  if (n <= 0 || W <= 0) return 0;
  // row offsets (W + 1), first / last partner row per window (W each), two state arrays (n each), the pending flags of a batch of passes
  return scan_align16((size_t)(W + 1) * 4) + 2 * scan_align16((size_t)W * 4) + 2 * scan_align16((size_t)n) + 16;
}

extern "C" int sy11_scan_merge(int32_t n, int32_t W, int32_t n_frames, const int32_t* window, const float* boxes, const float* score,
                               const int32_t* cls, const int64_t* start, int32_t metric, float thres, int32_t agnostic, void* workspace,
                               uint8_t* keep, void* stream) {
  SY11_REQUIRE(n >= 0 && W > 0 && n_frames > 0, "scan_merge: bad dims");
  SY11_REQUIRE(metric == 0 || metric == 1, "scan_merge: metric must be 0 (iou) or 1 (ios)");
  if (n == 0) return SY11_OK;
  SY11_REQUIRE(window && boxes && score && cls && start && workspace && keep, "scan_merge: null pointer");
  SY11_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "scan_merge: boxes and workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)workspace;
  int* off = (int*)p;        p += scan_align16((size_t)(W + 1) * 4);
  int* rlo = (int*)p;        p += scan_align16((size_t)W * 4);
  int* rhi = (int*)p;        p += scan_align16((size_t)W * 4);
  uint8_t* sa = (uint8_t*)p; p += scan_align16((size_t)n);
  uint8_t* sb = (uint8_t*)p; p += scan_align16((size_t)n);
  int* flags = (int*)p;
  if (hipMemsetAsync(sa, 0, (size_t)n, st) != hipSuccess) SY11_FAIL(SY11_ELAUNCH, "scan_merge: memset failed");
  hipLaunchKernelGGL(scan_row_offsets_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, W, window, off);
  SY11_LAUNCH_CHECK("scan_merge (row offsets)");
  hipLaunchKernelGGL(scan_row_ranges_kernel, dim3(cdiv(W, 256)), dim3(256), 0, st, n, W, n_frames, (const long long*)start, off, rlo, rhi);
  SY11_LAUNCH_CHECK("scan_merge (row ranges)");
  // passes in batches of four (an even count: the current states are in `sa` after every batch); one host read per batch.  Every
  // pass decides at least the best-ranked undecided box, so n passes always suffice.
  for (long pass = 0; pass < (long)n + 4; pass += 4) {
    if (hipMemsetAsync(flags, 0, 16, st) != hipSuccess) SY11_FAIL(SY11_ELAUNCH, "scan_merge: memset failed");
    for (int k = 0; k < 4; ++k) {
      hipLaunchKernelGGL(scan_merge_pass_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, n, W, n_frames, window, (const f32x4*)boxes, score, cls,
                         (const long long*)start, rlo, rhi, metric, (double)thres, agnostic, (k & 1) ? sb : sa, (k & 1) ? sa : sb, keep, flags + k);
      SY11_LAUNCH_CHECK("scan_merge (pass)");
    }
    int left = 0;
    if (hipMemcpyAsync(&left, flags + 3, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      SY11_FAIL(SY11_ELAUNCH, "scan_merge: reading the pending flag failed: %s", hipGetErrorString(hipGetLastError()));
    if (!left) return SY11_OK;
  }
  SY11_FAIL(SY11_ELAUNCH, "scan_merge: no fixed point after n passes");
}
