// dwgrad1x1.hip — input gradient AND filter gradient of a dense 1x1 / stride-1 convolution in one pass over dy (gfx950).
//
//   dx[m][c]  = sum_n dy[m][n] * w[n][c]          (m = pixel; the conv's input gradient, optionally added into dx)
//   dW[n][c] += sum_m dy[m][n] * x[m][c]          (f32, atomics — the filter gradient)
//
// Run as the pair sy11_conv2d_dgrad + sy11_conv2d_wgrad, dy travels from HBM into LDS twice.  Here a PERSISTENT workgroup of eight
// waves walks a contiguous run of 128-pixel tiles; per tile it stages dy[128 x N] and x[128 x C] once (register staging, the next
// tile's loads in flight under this tile's math), computes the dx tile from the staged dy and the LDS-resident transposed filter
// wT[c][n] (row reads, ds_read_b128), adds dy^T * x into dW accumulators that stay in registers over all of its tiles (the
// hardware-transposing fragment read of wgrad16_kernel, ds_read_b64_tr_b16), and stores the dx tile through LDS with 16-byte
// stores.  After the last tile the dW block goes into the f32 gradient with atomics, exactly as wgrad16_kernel ends.
//
// One LDS image serves both kinds of read: plain [row][chunk] rows with the 16-byte chunk index XORed by
// ((row & 3) << 2) | ((row >> 2) & 3) — sixteen consecutive rows of one chunk (the ds_read_b128 lane groups) land on sixteen
// different 16-byte slots, and the four rows x 64 bytes a 32-lane half of the transposing read touches land on four disjoint
// 64-byte windows.
//
// NP x CP = N and the workgroup's share of C rounded up to 64 / 128 / 256 (columns past N / past the share are zero-filled by
// the out-of-range buffer loads and masked on the way out).  NP * CP <= 32768: 64 dW accumulator registers per lane.  A filter
// too large for that, or for the LDS beside the two tiles, is cut into COLUMN blocks of C (gridDim.y): block j owns
// dW[:, block j] and dx[:, block j]; both need all of dy (re-read per block; the blocks of one tile run side by side on one
// XCD and meet in its L2) and only block j of x and of the filter.
#include "common.h"
#include "tune.h"
#include "det.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

template <typename T> struct Mma;
template <> struct Mma<_Float16> {
  static __device__ __forceinline__ f32x16 run(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mma<__bf16> {
  static __device__ __forceinline__ f32x16 run(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

struct DW1Args {
  const void* dy;
  const void* x;
  const void* wt;         // [C][N]: the tap-transposed filter of sy11_weight_transpose
  void* dx;
  float* dw;              // [N][C] f32
  int M, C, N;
  int dy_ld, x_ld, dx_ld;
  int cb;                 // input channels per column block (multiple of 8)
  int tiles_m;
  unsigned dy_bytes, x_bytes, wt_bytes;
  int accumulate;
};

// byte offset of 16-byte chunk `ch` of row `row` in an image of CH chunks per row (CH a power of two >= 8)
template <int CH>
__device__ __forceinline__ int img_off(int row, int ch) {
  return row * (CH * 16) + ((ch ^ ((((row & 3) << 2) | ((row >> 2) & 3)) & (CH - 1))) << 4);
}

// 32 columns (first: col0, a multiple of 32) x 16 rows (k-step ks) of an image, as the MFMA operand "8 consecutive rows of one column
// per lane": lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3 of the group's 4 x 16 block
template <int CH>
__device__ __forceinline__ s16x8 tr_frag(const unsigned char* img, int ks, int col0, int lane) {
  const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int r = ks * 16 + (grp >> 1) * 8 + q;
  const int ch = (col0 >> 3) + (grp & 1) * 2 + (p >> 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + img_off<CH>(r, ch) + 8 * (p & 1)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + img_off<CH>(r + 4, ch) + 8 * (p & 1)));
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

constexpr int DW1_BM = 128;
constexpr size_t dw1_lds(int np, int cp) { return (size_t)DW1_BM * 2 * (np + cp) + (size_t)cp * np * 2; }

template <typename T, int NP, int CP>
__global__ __launch_bounds__(512) void dgrad_wgrad1x1_kernel(const DW1Args a) {
  constexpr int BM = DW1_BM;
  constexpr int DCH = NP / 8, XCH = CP / 8;                 // 16-byte chunks per dy / x row
  constexpr int SD = BM * NP * 2, SX = BM * CP * 2;
  constexpr int PD = BM * DCH / 512, PX = BM * XCH / 512;   // staging passes: 512 threads cover 512 / DCH (512 / XCH) rows at a time
  constexpr int PW = CP * DCH / 512;
  // dW: NP x CP in 32 x 32 blocks over the eight waves, WR x WC waves of FI x FJ blocks; with fewer than eight blocks KH waves share
  // one and split the tile's eight k-steps (their partial sums meet in the atomics at the end)
  constexpr int NBN = NP / 32, NBC = CP / 32;
  constexpr int WR = NBN < 4 ? NBN : 4, WC = NBC < 8 / WR ? NBC : 8 / WR, KH = 8 / (WR * WC);
  constexpr int FI = NBN / WR, FJ = NBC / WC;
  constexpr int KPW = (BM / 16) / KH;
  // dx: 128 x CP over 4 x 2 waves, one row block and FJX column blocks each
  constexpr int FJX = CP / 64, JX = FJX < 2 ? FJX : 2;
  static_assert(NP >= 64 && CP >= 64 && NP * CP <= 32768, "tile sizes");
  static_assert(WR * WC * KH == 8 && FI * WR == NBN && FJ * WC == NBC, "wave layout");
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const sD = smem;                           // [BM][NP]  dy tile
  unsigned char* const sX = sD + SD;                        // [BM][CP]  x tile; after the math the dx tile, plain rows
  unsigned char* const sW = sX + SX;                        // [CP][NP]  filter block, rows = input channels

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.y * a.cb, c_end = min(a.C, c0 + a.cb);
  // this workgroup's run of tiles
  const int G = gridDim.x, g = blockIdx.x;
  const int base = a.tiles_m / G, rem = a.tiles_m - base * G;
  const int t0 = g * base + min(g, rem), t1 = t0 + base + (g < rem ? 1 : 0);
  if (t0 >= t1) return;

  const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr_ = __builtin_amdgcn_make_buffer_rsrc((void*)a.wt, 0, a.wt_bytes, 0x00020000);

  // ---- the filter block, once: sW[c - c0][n]
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int idx = tid + 512 * i, row = idx / DCH, ch = idx - row * DCH;
    const bool ok = c0 + row < c_end && ch * 8 < a.N;
    const u4 v = __builtin_amdgcn_raw_buffer_load_b128(wr_, ok ? (unsigned)(((c0 + row) * a.N + ch * 8) * 2) : OOB, 0, 0);
    *(uint4*)(sW + img_off<DCH>(row, ch)) = make_uint4(v[0], v[1], v[2], v[3]);
  }

  // ---- staging roles: one fixed 16-byte chunk of PD dy rows and of PX x rows per tile
  const int d_ch = tid % DCH, d_row = tid / DCH;
  const int x_ch = tid % XCH, x_row = tid / XCH;
  const int d_col = d_ch * 8 < a.N ? d_ch * 16 : -1;
  const int x_col = c0 + x_ch * 8 < c_end ? (c0 + x_ch * 8) * 2 : -1;
  const int dy_rowb = a.dy_ld * 2, x_rowb = a.x_ld * 2;
  uint4 rd[PD], rx[PX];
  auto load_tile = [&](int tile) {
    const int m0 = tile * BM;
#pragma unroll
    for (int p = 0; p < PD; ++p) {
      const int m = m0 + d_row + p * (512 / DCH);
      const u4 v = __builtin_amdgcn_raw_buffer_load_b128(dr, (m < a.M && d_col >= 0) ? (unsigned)m * (unsigned)dy_rowb + (unsigned)d_col : OOB, 0, 0);
      rd[p] = make_uint4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int p = 0; p < PX; ++p) {
      const int m = m0 + x_row + p * (512 / XCH);
      const u4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, (m < a.M && x_col >= 0) ? (unsigned)m * (unsigned)x_rowb + (unsigned)x_col : OOB, 0, 0);
      rx[p] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int p = 0; p < PD; ++p) *(uint4*)(sD + img_off<DCH>(d_row + p * (512 / DCH), d_ch)) = rd[p];
#pragma unroll
    for (int p = 0; p < PX; ++p) *(uint4*)(sX + img_off<XCH>(x_row + p * (512 / XCH), x_ch)) = rx[p];
  };

  const int frow = lane & 31, fh = lane >> 5;
  // dW roles
  const int kh = wave / (WR * WC), wrc = wave - kh * (WR * WC), wr = wrc / WC, wc = wrc - wr * WC;
  f32x16 acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // dx roles
  const int wrx = wave >> 1, wcx = wave & 1;

  load_tile(t0);
  for (int tile = t0; tile < t1; ++tile) {
    store_tile();
    __syncthreads();                                         // the tile (and, first time, the filter) is in LDS
    if (tile + 1 < t1) load_tile(tile + 1);                  // in flight under the math and the epilogue below
    // ---- dW += dy^T * x
#pragma unroll
    for (int kq = 0; kq < KPW; ++kq) {
      const int ks = kh * KPW + kq;
      s16x8 fa[FI], fb[FJ];
#pragma unroll
      for (int i = 0; i < FI; ++i) fa[i] = tr_frag<DCH>(sD, ks, (wr * FI + i) * 32, lane);
#pragma unroll
      for (int j = 0; j < FJ; ++j) fb[j] = tr_frag<XCH>(sX, ks, (wc * FJ + j) * 32, lane);
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = Mma<T>::run(fa[i], fb[j], acc[i][j]);
    }
    __syncthreads();                                         // every wave is done with the x tile: its LDS becomes the dx tile
    // ---- dx tile = dy * wT^T, JX column blocks of 32 at a time (their accumulators are live beside the dW block's), written as
    // plain 16-bit rows.  D map: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int j0 = 0; j0 < FJX; j0 += JX) {
      f32x16 ax[JX];
#pragma unroll
      for (int j = 0; j < JX; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) ax[j][e] = 0.f;
#pragma unroll 4
      for (int ks = 0; ks < NP / 16; ++ks) {
        const uint4 fa = *(const uint4*)(sD + img_off<DCH>(wrx * 32 + frow, 2 * ks + fh));
        uint4 fb[JX];
#pragma unroll
        for (int j = 0; j < JX; ++j) fb[j] = *(const uint4*)(sW + img_off<DCH>(wcx * (CP / 2) + (j0 + j) * 32 + frow, 2 * ks + fh));
#pragma unroll
        for (int j = 0; j < JX; ++j) ax[j] = Mma<T>::run(__builtin_bit_cast(s16x8, fa), __builtin_bit_cast(s16x8, fb[j]), ax[j]);
      }
#pragma unroll
      for (int j = 0; j < JX; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rl = wrx * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
          const int cl = wcx * (CP / 2) + (j0 + j) * 32 + frow;
          *(T*)(sX + (rl * CP + cl) * 2) = ElemTraits<T>::from_f(ax[j][e]);
        }
    }
    __syncthreads();
    const int m0 = tile * BM;
#pragma unroll
    for (int k = 0; k < BM * XCH / 512; ++k) {
      const int idx = tid + k * 512, rl = idx / XCH, ch = idx - rl * XCH;
      const int m = m0 + rl, c = c0 + ch * 8;
      if (m < a.M && c < c_end) {
        uint4 v = *(const uint4*)(sX + (rl * CP + ch * 8) * 2);
        T* gp = (T*)a.dx + (long)m * a.dx_ld + c;
        if (a.accumulate) {
          typedef T vt8 __attribute__((ext_vector_type(8)));
          vt8 s = __builtin_bit_cast(vt8, v), o = *(const vt8*)gp;
#pragma unroll
          for (int q = 0; q < 8; ++q) s[q] = ElemTraits<T>::from_f(ElemTraits<T>::to_f(s[q]) + ElemTraits<T>::to_f(o[q]));
          v = __builtin_bit_cast(uint4, s);
        }
        *(uint4*)gp = v;
      }
    }
    __syncthreads();                                         // the dx tile has left LDS before the next x tile lands there
  }
  // ---- the dW block: 32 lanes = 32 consecutive input channels = 128 contiguous bytes per atomic instruction
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = (wr * FI + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
        const int c = c0 + (wc * FJ + j) * 32 + frow;
        if (n < a.N && c < c_end) atomicAdd(a.dw + (long)n * a.C + c, acc[i][j][e]);
      }
}

int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t p;
    n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
  }
  return n;
}
size_t lds_limit() {
  static size_t n = 0;
  if (!n) {
    int dev = 0, v = 0;
    n = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0) ? (size_t)v : (size_t)64 * 1024;
    (void)hipGetLastError();
  }
  return n;
}

// resident workgroups per CU of one instantiation (occupancy API, asked once), 0 = the kernel cannot be launched with this much LDS
template <typename T, int NP, int CP>
int dw1_resident() {
  static int n = -1;
  if (n < 0) {
    const int lds = (int)dw1_lds(NP, CP);
    int nb = 0;
    if (hipFuncSetAttribute((const void*)dgrad_wgrad1x1_kernel<T, NP, CP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)dgrad_wgrad1x1_kernel<T, NP, CP>, 512, lds) != hipSuccess) {
      (void)hipGetLastError();
      nb = 0;
    }
    n = nb > 0 ? nb : 0;
  }
  return n;
}

template <typename T, int NP, int CP>
int dw1_launch(DW1Args a, int blocks_c, hipStream_t st) {
  const int per_cu = dw1_resident<T, NP, CP>();
  if (per_cu <= 0) SY11_FAIL(SY11_ELAUNCH, "conv2d_dgrad_wgrad_1x1: the %d x %d tile (%zu bytes of LDS) cannot be launched", NP, CP, dw1_lds(NP, CP));
  // one resident round, shared by the column blocks; a whole number of XCD rounds (8) so that the column blocks of one tile run share an XCD
  int G = per_cu * cu_count() / blocks_c;
  const int forced = sy11_opt(OPT_DWGRAD_WG);
  if (forced > 0) G = forced;
  else if (G >= 8) G &= ~7;
  if (G > a.tiles_m) G = a.tiles_m;
  if (G < 1) G = 1;
  hipLaunchKernelGGL((dgrad_wgrad1x1_kernel<T, NP, CP>), dim3(G, blocks_c), dim3(512), dw1_lds(NP, CP), st, a);
  SY11_LAUNCH_CHECK("conv2d_dgrad_wgrad_1x1");
  return SY11_OK;
}

}  // namespace

// The column split, host arithmetic (exported so that it can be checked without a GPU): NP = N rounded up to 64 / 128 / 256; the widest
// column block CP of 256 / 128 / 64 with NP * CP <= 32768 whose LDS fits `lds_bytes`; blocks = ceil(C / CP), cb = ceil(C / blocks)
// rounded up to 16, CP = cb rounded up to 64 / 128 / 256.  Returns SY11_EUNSUPPORTED when nothing fits.
extern "C" int sy11_dgrad_wgrad_1x1_plan(int32_t C, int32_t N, int64_t lds_bytes, int32_t* np, int32_t* cp, int32_t* cb, int32_t* blocks) {
  SY11_REQUIRE(np && cp && cb && blocks, "dgrad_wgrad_1x1_plan: null argument");
  if (C < 16 || N < 16 || C > 256 || N > 256 || C % 16 || N % 16)
    SY11_FAIL(SY11_EUNSUPPORTED, "conv2d_dgrad_wgrad_1x1: C = %d, N = %d (multiples of 16 in 16..256)", C, N);
  auto pad = [](int v) { return v <= 64 ? 64 : v <= 128 ? 128 : 256; };
  const int NPv = pad(N);
  int cpmax = 0;
  for (int c = 256; c >= 64; c >>= 1)
    if (NPv * c <= 32768 && (int64_t)dw1_lds(NPv, c) <= lds_bytes) { cpmax = c; break; }
  if (!cpmax) SY11_FAIL(SY11_EUNSUPPORTED, "conv2d_dgrad_wgrad_1x1: no tile for N = %d fits %lld bytes of LDS", N, (long long)lds_bytes);
  const int nb = cdiv(C, cpmax), per = cdiv(cdiv(C, nb), 16) * 16;
  *np = NPv; *cp = pad(per); *cb = per; *blocks = cdiv(C, per);
  return SY11_OK;
}

extern "C" int sy11_conv2d_dgrad_wgrad_1x1(int32_t dtype, int32_t M, int32_t C, int32_t N, const void* dy, int32_t dy_ld, const void* x,
                                           int32_t x_ld, const void* wt, void* dx, int32_t dx_ld, int32_t accumulate, float* dw,
                                           void* stream) {
  SY11_REQUIRE(dy && x && wt && dx && dw, "conv2d_dgrad_wgrad_1x1: null argument");
  SY11_REQUIRE(dtype_ok(dtype), "conv2d_dgrad_wgrad_1x1: bad dtype");
  if (dtype == SY11_F32) SY11_FAIL(SY11_EUNSUPPORTED, "conv2d_dgrad_wgrad_1x1: 16-bit dtypes only");
  SY11_REQUIRE(M > 0 && C > 0 && N > 0, "conv2d_dgrad_wgrad_1x1: non-positive dims");
  SY11_REQUIRE(dy_ld % 8 == 0 && x_ld % 8 == 0 && dx_ld % 8 == 0 && dy_ld >= N && x_ld >= C && dx_ld >= C, "conv2d_dgrad_wgrad_1x1: bad pixel strides");
  SY11_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)wt | (uintptr_t)dx) & 15) == 0 && ((uintptr_t)dw & 3) == 0, "conv2d_dgrad_wgrad_1x1: misaligned pointer");
  // ordered mode keeps one partial dW per pixel split and folds them in order: that is the pair's job
  if (sy11_det(8)) SY11_FAIL(SY11_EUNSUPPORTED, "conv2d_dgrad_wgrad_1x1: ordered reductions are on (use conv2d_dgrad + conv2d_wgrad)");
  int np, cp, cb, blocks;
  const int rc = sy11_dgrad_wgrad_1x1_plan(C, N, (int64_t)lds_limit(), &np, &cp, &cb, &blocks);
  if (rc) return rc;
  const long db = ((long)M - 1) * dy_ld * 2 + (long)N * 2, xb = ((long)M - 1) * x_ld * 2 + (long)C * 2, gb = ((long)M - 1) * dx_ld * 2 + (long)C * 2;
  SY11_REQUIRE(db < (1L << 31) && xb < (1L << 31) && gb < (1L << 31), "conv2d_dgrad_wgrad_1x1: operand view larger than 2 GiB");
  DW1Args a{};
  a.dy = dy; a.x = x; a.wt = wt; a.dx = dx; a.dw = dw;
  a.M = M; a.C = C; a.N = N;
  a.dy_ld = dy_ld; a.x_ld = x_ld; a.dx_ld = dx_ld;
  a.cb = cb;
  a.tiles_m = cdiv(M, DW1_BM);
  a.dy_bytes = (unsigned)db; a.x_bytes = (unsigned)xb; a.wt_bytes = (unsigned)((long)C * N * 2);
  a.accumulate = accumulate != 0;
  sy11_note_cfg(1, SY11_CFG_DWGRAD_1X1);
  hipStream_t st = (hipStream_t)stream;
#define SY11_DW1(TT)                                                                  \
  do {                                                                                \
    if (np == 64 && cp == 64) return dw1_launch<TT, 64, 64>(a, blocks, st);           \
    if (np == 64 && cp == 128) return dw1_launch<TT, 64, 128>(a, blocks, st);         \
    if (np == 64 && cp == 256) return dw1_launch<TT, 64, 256>(a, blocks, st);         \
    if (np == 128 && cp == 64) return dw1_launch<TT, 128, 64>(a, blocks, st);         \
    if (np == 128 && cp == 128) return dw1_launch<TT, 128, 128>(a, blocks, st);       \
    if (np == 128 && cp == 256) return dw1_launch<TT, 128, 256>(a, blocks, st);       \
    if (np == 256 && cp == 64) return dw1_launch<TT, 256, 64>(a, blocks, st);         \
    if (np == 256 && cp == 128) return dw1_launch<TT, 256, 128>(a, blocks, st);       \
  } while (0)
  if (dtype == SY11_F16) SY11_DW1(_Float16); else SY11_DW1(__bf16);
#undef SY11_DW1
  SY11_FAIL(SY11_EUNSUPPORTED, "conv2d_dgrad_wgrad_1x1: no kernel for the %d x %d tile", np, cp);
}
