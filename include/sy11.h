/* sy11.h — C-ABI of libsy11.so: the MI355X (gfx950) kernels behind the Spectrogram-YOLOv11 hot path.
 *
 * The reference (a fork of Ultralytics 8.3.70) has NO native code and NO FFI on this path: every op is a
 * stock ATen call issued from Python modules.  Each entry point below therefore names the reference
 * *Python call site* whose arithmetic it replaces (file:line under /root/reference/ultralytics), which is
 * what a maintainer would re-bind (see INTEGRATION.md for the ctypes stub).
 *
 * Conventions
 *   - all pointers are DEVICE pointers borrowed from the caller (torch tensors); the library allocates
 *     nothing persistent and keeps no global state; every call is asynchronous on `stream`
 *     (a hipStream_t passed as void*), re-entrant per stream, and never synchronises the host;
 *   - activations are NHWC; a tensor view is (pointer to first used channel, `ld` = elements between
 *     consecutive pixels), so channel slices of a wider buffer ("concat by pointer") need no copy;
 *   - conv weights are [Cout][KH][KW][Cin/groups] (= torch OIHW tensor in channels_last memory format);
 *   - dtype codes: 0 = f32, 1 = f16, 2 = bf16.  Accumulation is always f32;
 *   - return value: 0 on success, negative sy11_status on error; sy11_last_error() gives the message
 *     (thread-local).  Shapes/strides are validated on the host BEFORE any launch.
 */
#ifndef SY11_H
#define SY11_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SY11_VERSION 100

enum sy11_status { SY11_OK = 0, SY11_EINVAL = -1, SY11_EUNSUPPORTED = -2, SY11_ELAUNCH = -3 };
enum sy11_dtype { SY11_F32 = 0, SY11_F16 = 1, SY11_BF16 = 2, SY11_U8 = 3 /* image entries only */ };

/* epilogue / behaviour flags for the conv entry points */
#define SY11_EPI_SILU 1u       /* y = silu(acc + bias)                                   */
#define SY11_EPI_ACCUM 2u      /* y += acc (gradient accumulation into an existing view)  */
#define SY11_EPI_OUT_F32 4u    /* y is f32 whatever desc.dtype says (Detect logits)       */

typedef struct sy11_conv_desc {
  int32_t dtype;               /* element type of x, w, (y)                                  */
  int32_t B, IH, IW, C;        /* input: batch, height, width, channels CONSUMED              */
  int32_t x_ld;                /* input pixel stride (elements), >= C                          */
  int32_t OH, OW, N;           /* output: height, width, channels PRODUCED                     */
  int32_t y_ld;                /* output pixel stride (elements), >= N                         */
  int32_t KH, KW, SH, SW, PH, PW, DH, DW;
  int32_t groups;              /* 1, or == C == N (depthwise)                                  */
  uint32_t flags;              /* SY11_EPI_*                                                   */
  int32_t stat_slots;          /* stat_sum / stat_sq are [stat_slots][N]; workgroup i adds into slot i % stat_slots
                                  (same-address f32 atomics retire at ~25 ns each: spreading them keeps the BN
                                  statistics off the critical path).  0 or 1 = a single [N] row.               */
} sy11_conv_desc;

int sy11_version(void);
const char* sy11_last_error(void);

/* ---- run-time options (no reference counterpart; "tune" stands where the reference has torch.backends.cudnn.benchmark,
 *      utils/torch_utils.py:488):
 *   "tune" 0|1            first-call tile autotuner (0: no NEW measurements; recorded / imported picks are still honoured)
 *   "tune_log" 0|1, "igemm_cfg" / "wgrad_cfg" (-1 = automatic, else force one tile configuration), "igemm_korder" 0|1,
 *   "igemm_deep" 0|1|2 (deeper LDS rings), "igemm_bpol" 0|1|2 (cache policy of the filter-row copies),
 *   "dgrad_s2_halo" 0|1 (3x3 stride-2 input gradient: four igemm launches, one per output parity / ONE fused-parity pass),
 *   "row_map" 0|1 (row walk of the BatchNorm and copy kernels: strided grid of r01 / contiguous chunk per workgroup),
 *   "maxpool_sep" 0|1 (5x5 max-pool of 16-bit tensors with 16-byte channel vectors: 25-way kernels / separable forward and column-walk backward),
 *   "dwgrad_fused" 0|1 (large-map dense 1x1 layers: input + filter gradient as the pair / as sy11_conv2d_dgrad_wgrad_1x1, read by the engine),
 *   "dwgrad_wg" n (workgroups per column block of sy11_conv2d_dgrad_wgrad_1x1; 0 = one resident round),
 *   "deterministic" 0|1   ordered reductions (cfg/default.yaml:29 `deterministic: True`, utils/torch_utils.py:474-492): every sum
 *                         across workgroups — BatchNorm statistics and backward sums, filter / bias gradients, loss partials —
 *                         goes through one partial row per workgroup and a fixed-shape fold instead of f32 atomics; bit-identical
 *                         results run to run when the tile choice is pinned ("tune" 0 or an imported pick table).  The partial
 *                         rows live in a per-stream workspace the LIBRARY allocates (grown during eager warm-up, never under capture).
 *                         Cost on the headline workload: +3.8 ... +4.9 % per training step (r04).
 * Defaults come from the environment (SY11_TUNE, SY11_TUNE_LOG, SY11_IGEMM_CFG, SY11_WGRAD_CFG, SY11_IGEMM_KORDER,
 * SY11_IGEMM_DEEP, SY11_IGEMM_BPOL, SY11_DGRAD_S2_HALO, SY11_ROW_MAP, SY11_DETERMINISTIC, SY11_MAXPOOL_SEP,
 * SY11_DWGRAD_FUSED, SY11_DWGRAD_WG).  Process-wide; set them between
 * launches, not concurrently with them.                                                                                */
int sy11_set_option(const char* name, int32_t value);
int sy11_get_option(const char* name, int32_t* value);
/* Two more names are READ-ONLY (sy11_get_option answers, sy11_set_option fails with a message): igemm_last_cfg and wgrad_last_cfg,
 * the tile configuration of the most recent forward / input-gradient launch and of the most recent filter-gradient launch
 * (csrc/igemm.hip 0..25, csrc/wgrad.hip 0..19; 100 = the fused-parity stride-2 input gradient, which is no entry of the igemm
 * table, and in wgrad_last_cfg the grouped launch of sy11_conv2d_wgrad_group, which is no entry of the wgrad table, 101 there the fused 1x1 launch of
 * sy11_conv2d_dgrad_wgrad_1x1; -1 before the first launch).  The tuner's candidate launches record themselves too: read them with "tune" 0.
 * Likewise stem_fwd_last and stem_wgrad_last: which first-layer kernel (csrc/direct.hip) the most recent sy11_stem_conv_fwd[_bn] /
 * sy11_stem_conv_wgrad launched — 1 gather, 2 MFMA gather, 3 LDS-tiled with 16-byte image loads, 4 LDS-tiled with element-wise
 * fill; -1 before the first launch.
 * pool_fwd_last and pool_bwd_last: which 5x5 max-pool kernel the most recent sy11_maxpool5_fwd / sy11_maxpool5_bwd launched —
 * 1 25-way with one element per thread, 2 25-way with 16-byte channel vectors, 3 the separable forward / column-walk backward.
 * ew_vec_last: the channel-vector width in elements (1, 4 or 8) of the most recent sy11_copy2d / sy11_upsample2x_fwd /
 * sy11_upsample2x_bwd launch.  Both -1 before the first launch.                                                              */
/* The autotuner's pick tables as a flat array of 16-byte records {u64 problem hash, i32 kind, i32 pick}: export on one
 * rank, broadcast, import on the others, so every rank of a data-parallel job (engine/trainer.py:217-228) runs the same
 * kernels.  sy11_tune_export returns the number of bytes needed (pass buf = NULL to size the buffer).                 */
int64_t sy11_tune_export(void* buf, int64_t capacity_bytes);
int sy11_tune_import(const void* buf, int64_t bytes);
int sy11_tune_clear(void);
/* Measurement helper (bench.py `peaks`): a pure-MFMA loop, `iters` x 8 v_mfma_f32_32x32x16_f16 per wave, 4 waves per
 * workgroup, no memory traffic.  FLOPs per launch = workgroups * 4 * iters * 8 * 32768; out: workgroups * 4 floats.     */
int sy11_peak_mfma_f16(int32_t workgroups, int32_t iters, float* out, void* stream);
/* Diagnostic (tools/igemm8_stamps.py, never on the product path): with SY11_IGEMM_DEBUG=9 the 8-wave convolution pipeline
 * (csrc/igemm8.hip) sums per-section s_memtime deltas in waves 0 / 4 of workgroup 0; this copies the 2 x 8 counters of the
 * last such launch to the HOST array out16 (synchronous).  With out16[0] == 1 on entry the array must hold 16 + 8 * 2048
 * elements: the per-workgroup records {entry, exit (100 MHz ticks), XCC id, cycles of the four kernel sections, 0} of the first 2048
 * workgroups follow.                                                                                                      */
int sy11_debug_stamps(uint64_t* out16);
/* ... and of its persistent form (csrc/igemm8p.hip): per workgroup (256) {cycles waiting for the first stages, main loops, next-tile
 * addresses + first copies, epilogues, tiles, 100 MHz ticks from start to end, 0, 0} -> 2048 values on the host.                  */
int sy11_debug_stamps_persistent(uint64_t* out2048);

/* ---- convolution (replaces nn.Conv2d inside Conv.forward / forward_fuse, nn/modules/conv.py:79-83,
 *      and the bare nn.Conv2d heads of Detect, nn/modules/head.py:44-55) -------------------------------- */

/* y[b,oy,ox,n] = sum_{r,s,c} x[b, oy*SH-PH+r*DH, ox*SW-PW+s*DW, c] * w[n,r,s,c]  (+bias[n]) (silu)
 * groups==1: implicit-GEMM on MFMA.  groups==C==N: direct depthwise kernel.
 * stat_sum/stat_sq (f32[N], may be NULL): per-channel sum and sum of squares of the f32 accumulators are
 * atomically ADDED (BatchNorm batch statistics of F.batch_norm(training=True), conv.py:81).               */
int sy11_conv2d_fwd(const sy11_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                    float* stat_sum, float* stat_sq, void* stream);

/* Conv.forward in train mode (conv.py:81: bn(conv(x)) with batch statistics): the convolution above with its BatchNorm
 * statistics FINALISED in the kernel tail — the last workgroup to finish folds the statistic slots and writes mean / rstd
 * (saved for backward), scale = gamma*rstd, shift = beta - mean*scale, and the running-stat update, exactly what
 * sy11_bn_finalize computes.  ticket: zero-initialised int32 words (one per group for grouped convs), returned at zero.   */
typedef struct sy11_bn_tail {
  const float* gamma;
  const float* beta;
  float* running_mean;         /* both NULL: no running-stat update */
  float* running_var;
  float* mean;                 /* outputs, [N] each */
  float* rstd;
  float* scale;
  float* shift;
  int32_t* ticket;
  float eps, momentum;
  double count;                /* pixels per channel: B*OH*OW */
} sy11_bn_tail;
int sy11_conv2d_fwd_bn(const sy11_conv_desc* d, const void* x, const void* w, void* y, float* stat_sum, float* stat_sq,
                       const sy11_bn_tail* bn, void* stream);

/* dx = conv_transpose(dy, w): gradient wrt the input of the conv described by `d`
 * (autograd of nn.Conv2d, fired by loss.backward() at engine/trainer.py:388).
 * `dy` has pixel stride dy_ld, `dx` pixel stride d->x_ld.  wt is the tap-transposed filter made by
 * sy11_weight_transpose: [C][KH*KW][N] for groups==1 (ignored for depthwise: pass w).
 * SY11_EPI_ACCUM in d->flags adds into dx instead of overwriting it.                                      */
int sy11_conv2d_dgrad(const sy11_conv_desc* d, const void* dy, int32_t dy_ld, const void* wt, void* dx, void* stream);

/* dw[n,r,s,c] += sum_{b,oy,ox} dy[b,oy,ox,n] * x[b, oy*SH-PH+r*DH, ox*SW-PW+s*DW, c]   (dw is ALWAYS f32 and is
 * accumulated into: zero it for a fresh gradient).                                                         */
int sy11_conv2d_wgrad(const sy11_conv_desc* d, const void* x, const void* dy, int32_t dy_ld, float* dw, void* stream);

/* Several dense 16-bit filter gradients in ONE launch (the small-map layers of a backward pass: each alone has too few dW tiles
 * to fill the chip without many pixel splits).  Per problem exactly the sum above, dw += x (*) dy, with the arguments and the
 * checks of sy11_conv2d_wgrad; in addition: dtype F16 or BF16 (the same for every problem), groups == 1, 1 <= count <=
 * SY11_WGRAD_GROUP_MAX.  All checks run before anything is launched.  The problems travel by value in the kernel's argument block:
 * nothing is copied to the device or allocated, and `problems` may be freed as soon as the call returns.
 * target_workgroups: how many workgroups the group is cut into (0 = one resident round of the chip); the split is the pure function
 * below.  Partial sums meet in dw through f32 atomics: with the "deterministic" option on the call returns SY11_EUNSUPPORTED and
 * launches nothing (the caller runs the problems through sy11_conv2d_wgrad, which has the ordered path).
 * "wgrad_last_cfg" reads 100 after a grouped launch.                                                                          */
#define SY11_WGRAD_GROUP_MAX 32
typedef struct sy11_wgrad_problem {
  sy11_conv_desc desc;
  const void* x;
  const void* dy;
  float* dw;
  int32_t dy_ld;
  int32_t reserved;
} sy11_wgrad_problem;
int sy11_conv2d_wgrad_group(int32_t dtype, int32_t count, const sy11_wgrad_problem* problems, int32_t target_workgroups,
                            void* stream);
/* The work split of a grouped launch, host arithmetic only.  Problem i (M = B*OH*OW pixels, N filters, K = KH*KW*C columns) has
 * tiles_i = ceil(N/128) * ceil(K/128) tiles and stages_i = ceil(M/64) stages.  chunk = max(8, ceil(sum tiles_i * stages_i /
 * target_workgroups)); splits_i = ceil(stages_i / chunk); pix_per_split[i] = 64 * ceil(stages_i / splits_i); problem i owns the
 * workgroups wg_start[i] .. wg_start[i+1] (count + 1 entries), tiles_i * ceil(M / pix_per_split[i]) of them, split-major.       */
int sy11_wgrad_group_plan(int32_t count, const int32_t* M, const int32_t* N, const int32_t* K, int32_t target_workgroups,
                          int32_t* pix_per_split, int32_t* wg_start);

/* Input gradient and filter gradient of a DENSE 1x1 / stride-1 / unpadded convolution in one launch: dy is read once instead of
 * once per gradient (csrc/dwgrad1x1.hip).  M = B*H*W pixels, C input and N output channels;
 *     dx[m][c]  = sum_n dy[m][n] * wt[c][n]   (dx += ... when accumulate != 0; dx has the dtype of dy)
 *     dw[n][c] += sum_m dy[m][n] * x[m][c]    (f32, f32 atomics: zero it for a fresh gradient)
 * — what sy11_conv2d_dgrad followed by sy11_conv2d_wgrad compute for that layer, up to summation order.  dtype F16 or BF16 (F32:
 * SY11_EUNSUPPORTED); C and N multiples of 16 in 16..256 (else SY11_EUNSUPPORTED); dy, x, dx are pixel-major views with pixel strides
 * dy_ld >= N, x_ld >= C, dx_ld >= C (multiples of 8, 16-byte aligned bases, each view below 2 GiB): channel slices of wider tensors
 * work, the channels outside a slice are not touched.  wt: the [C][N] filter of sy11_weight_transpose.  With the "deterministic"
 * option on the call returns SY11_EUNSUPPORTED and launches nothing (the caller runs the pair, which has the ordered path).
 * Persistent workgroups, one resident round by the occupancy API ("dwgrad_wg" n > 0 forces n workgroups per column block);
 * "wgrad_last_cfg" reads 101 after the launch.  "dwgrad_fused" (SY11_DWGRAD_FUSED, default 1) is the ENGINE's switch between this
 * entry point and the pair; the entry point does not look at it.                                                              */
int sy11_conv2d_dgrad_wgrad_1x1(int32_t dtype, int32_t M, int32_t C, int32_t N, const void* dy, int32_t dy_ld, const void* x,
                                int32_t x_ld, const void* wt, void* dx, int32_t dx_ld, int32_t accumulate, float* dw, void* stream);
/* The tile choice of that launch, host arithmetic only: np = N rounded up to 64 / 128 / 256; the widest column block of 256 / 128 /
 * 64 input channels with np * block <= 32768 whose LDS image, 256 * (np + block) + 2 * np * block bytes, fits lds_bytes;
 * blocks = ceil(C / that), cb = ceil(C / blocks) rounded up to 16, cp = cb rounded up to 64 / 128 / 256; finally blocks = ceil(C / cb).
 * A workgroup of column block j owns input channels j * cb .. min(C, (j + 1) * cb).                                           */
int sy11_dgrad_wgrad_1x1_plan(int32_t C, int32_t N, int64_t lds_bytes, int32_t* np, int32_t* cp, int32_t* cb, int32_t* blocks);

/* wt[c][t][n] = w[n][t][c]  (t = r*KW+s), same dtype; feeds sy11_conv2d_dgrad                               */
int sy11_weight_transpose(int32_t dtype, int32_t N, int32_t T, int32_t C, const void* w, void* wt, void* stream);

/* every dgrad filter of a model in one launch.  desc: device array of nlayers records
 * {int32 N, T, C, pad; int64 src_off, dst_off (elements into src / dst); int32 first_tile, tiles_c, tiles_n, pad}
 * sorted by first_tile; a layer owns T * tiles_n * tiles_c tiles of 32x32 (tiles_x = ceil(x/32)).                */
int sy11_weight_transpose_multi(int32_t dtype, int32_t nlayers, int32_t total_tiles, const void* desc, const void* src,
                                void* dst, void* stream);

/* first layer: x is the caller's NCHW f32 image (B,3,H,W) in [0,1] (detect/train.py:59 output); y NHWC.
 * stat_sum / stat_sq receive the per-channel sum and sum of squares of the RAW convolution — the f32 accumulator before bias,
 * activation and the rounding to the output type — in every kernel behind these entry points (what BatchNorm normalises).   */
int sy11_stem_conv_fwd(const sy11_conv_desc* d, const float* x_nchw, const void* w, const float* bias, void* y,
                       float* stat_sum, float* stat_sq, void* stream);
int sy11_stem_conv_fwd_bn(const sy11_conv_desc* d, const float* x_nchw, const void* w, void* y, float* stat_sum,
                          float* stat_sq, const sy11_bn_tail* bn, void* stream);
int sy11_stem_conv_wgrad(const sy11_conv_desc* d, const float* x_nchw, const void* dy, int32_t dy_ld, float* dw,
                         void* stream);

/* ---- BatchNorm (+SiLU, + residual) around the conv: nn.BatchNorm2d + nn.SiLU in Conv.forward
 *      (nn/modules/conv.py:81), eps/momentum from utils/torch_utils.py:417-418, residual of Bottleneck
 *      (nn/modules/block.py:725) ------------------------------------------------------------------------- */

/* from sum/sumsq (summed over stat_slots rows of C) over `count` pixels: mean, rstd (saved for backward), scale = gamma*rstd,
 * shift = beta - mean*scale, and the running-stat update (unbiased var, momentum).                          */
int sy11_bn_finalize(int32_t C, int32_t stat_slots, double count, const float* stat_sum, const float* stat_sq, const float* gamma,
                     const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                     float* mean, float* rstd, float* scale, float* shift, void* stream);

/* z = act(y*scale[c] + shift[c]) (+ res);  y,z,res: M pixels x C channels with their own pixel strides      */
int sy11_bn_act_fwd(int32_t dtype, int64_t M, int32_t C, const void* y, int32_t y_ld, const float* scale,
                    const float* shift, int32_t silu, const void* res, int32_t res_ld, void* z, int32_t z_ld,
                    void* stream);

/* backward, pass 1: g = dz * act'(y*scale+shift);  sum_g[c] += sum g;  sum_gx[c] += sum g * xhat.
 * sum_g / sum_gx are [sum_slots][C] (workgroup i adds into slot i % sum_slots; pass 2 folds the slots).          */
int sy11_bn_act_bwd_reduce(int32_t dtype, int64_t M, int32_t C, const void* y, int32_t y_ld, const void* dz,
                           int32_t dz_ld, const float* mean, const float* rstd, const float* scale,
                           const float* shift, int32_t silu, float* sum_g, float* sum_gx, int32_t sum_slots,
                           void* stream);
/* backward, pass 2: dy = gamma*rstd*(g - sum_g/M - xhat*sum_gx/M); also dgamma += sum_gx, dbeta += sum_g     */
int sy11_bn_act_bwd_apply(int32_t dtype, int64_t M, int32_t C, const void* y, int32_t y_ld, const void* dz,
                          int32_t dz_ld, const float* mean, const float* rstd, const float* scale,
                          const float* shift, const float* gamma, int32_t silu, const float* sum_g,
                          const float* sum_gx, int32_t sum_slots, void* dy, int32_t dy_ld, float* dgamma, float* dbeta,
                          void* stream);

/* pass 2 with the gradient of a RESIDUAL operand folded in (Bottleneck shortcut, nn/modules/block.py:725: z = x + act(bn(conv))):
 * res_grad[m, 0:C] (= | +=, f32 add and one rounding as sy11_copy2d) dz[m, 0:C], from the dz values the pass holds anyway —
 * instead of a separate three-pass copy launch.  res_grad == NULL: exactly sy11_bn_act_bwd_apply.                              */
int sy11_bn_act_bwd_apply_res(int32_t dtype, int64_t M, int32_t C, const void* y, int32_t y_ld, const void* dz,
                              int32_t dz_ld, const float* mean, const float* rstd, const float* scale,
                              const float* shift, const float* gamma, int32_t silu, const float* sum_g,
                              const float* sum_gx, int32_t sum_slots, void* dy, int32_t dy_ld, float* dgamma, float* dbeta,
                              void* res_grad, int32_t res_ld, int32_t res_accumulate, void* stream);

/* ---- data movement inside the graph --------------------------------------------------------------------- */
/* dst[m, 0:C] (= | +=) src[m, 0:C] with independent pixel strides: torch.cat / chunk (conv.py:1821,
 * block.py:466-468) and residual-gradient accumulation.                                                     */
int sy11_copy2d(int32_t dtype, int64_t M, int32_t C, const void* src, int32_t src_ld, void* dst, int32_t dst_ld,
                int32_t accumulate, void* stream);
/* nn.Upsample(None, 2, "nearest") (cfg/models/11/yolo11.yaml:34,38) written straight into a concat slice    */
int sy11_upsample2x_fwd(int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, const void* x, int32_t x_ld,
                        void* y, int32_t y_ld, void* stream);
int sy11_upsample2x_bwd(int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, const void* dy, int32_t dy_ld,
                        void* dx, int32_t dx_ld, int32_t accumulate, void* stream);
/* pairwise IoU of the validator's _process_batch (utils/metrics.py:52-72; models/yolo/detect/val.py:205-232):
 * a (n,4), b (m,4) xyxy f32 -> out (n,m) f32, bit-identical to the reference's element-wise evaluation order      */
int sy11_box_iou(int32_t n, int32_t m, const float* a, const float* b, float eps, float* out, void* stream);

/* ---- Fusion('ESChannel') of the fusion model variant (cfg yolo11_fusion_sand3_new.yaml) ----------------------
 * Replaces Fusion.forward (nn/modules/conv.py:2087-2127) = GCT (conv.py:2284-2301) on the channel concat plus
 * WeightedSpatialAttention(3) (conv.py:1839-1852) per input:  out = sum_i x_i * (gate[b, i*C + c] + S_i[b, h, w]).
 * All views NHWC (pointer + pixel stride); C * sizeof(elem) / 16 must be a power of two <= 64 (C = 128 in the model). */
/* per input: mm[pix] = (mean_c x, max_c x), amax[pix] = first argmax channel, sq[b*sq_ld + c] += sum_hw x^2        */
int sy11_fusion_stats(int32_t dtype, int32_t B, int32_t HW, int32_t C, const void* x, int32_t x_ld, float* mm,
                      uint16_t* amax, float* sq, int32_t sq_ld, void* stream);
/* S = sigmoid(conv3x3(mm; w)), pad 1, no bias; w = cv1.weight[0] in [KH][KW][2] memory (18 floats)                 */
int sy11_sab_map_fwd(int32_t B, int32_t H, int32_t W, const float* mm, const float* w, float* S, void* stream);
int sy11_sab_map_bwd(int32_t B, int32_t H, int32_t W, const float* dS, const float* S, const float* mm, const float* w,
                     float* dmm, float* dw /* [18] accumulated */, void* stream);
/* gate[b][c] = 1 + tanh(e * gamma / sqrt(mean_c(e^2) + eps) + beta), e = sqrt(sq + eps) * alpha, c in [0, Ct)     */
int sy11_gct_gate_fwd(int32_t B, int32_t Ct, const float* sq, const float* alpha, const float* gamma, const float* beta,
                      float eps, float* G, void* stream);
/* from dG = dL/dgate: q[b][c] with dx += x * q, and dalpha / dgamma / dbeta accumulated over the batch             */
int sy11_gct_gate_bwd(int32_t B, int32_t Ct, const float* sq, const float* alpha, const float* gamma, const float* beta,
                      float eps, const float* dG, float* q, float* dalpha, float* dgamma, float* dbeta, void* stream);
int sy11_fusion_combine(int32_t dtype, int32_t B, int32_t HW, int32_t C, int32_t n_in, const void* x0, int32_t ld0,
                        const float* S0, const void* x1, int32_t ld1, const float* S1, const void* x2, int32_t ld2,
                        const float* S2, const float* G, void* out, int32_t out_ld, void* stream);
/* per input: dG[b*dg_ld + c] += sum_pix dout * x ; dS[pix] = sum_c dout * x                                        */
int sy11_fusion_bwd_reduce(int32_t dtype, int32_t B, int32_t HW, int32_t C, const void* dout, int32_t dout_ld,
                           const void* x, int32_t x_ld, float* dG, int32_t dg_ld, float* dS, void* stream);
/* per input: dx (= | +=) dout * (G + S) + x * q + dmm[.,0] / C + [c == amax] dmm[.,1]                              */
int sy11_fusion_bwd_apply(int32_t dtype, int32_t B, int32_t HW, int32_t C, const void* dout, int32_t dout_ld,
                          const void* x, int32_t x_ld, const float* G, const float* q, int32_t g_ld, const float* S,
                          const float* dmm, const uint16_t* amax, void* dx, int32_t dx_ld, int32_t accumulate,
                          void* stream);

/* nn.MaxPool2d(5, 1, 2) (SPPF, nn/modules/block.py:192,197); idx[m,c] = window position (0..24) of the
 * first maximum in row-major scan order (ATen max_pool2d_with_indices tie rule).                            */
int sy11_maxpool5_fwd(int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, const void* x, int32_t x_ld,
                      void* y, int32_t y_ld, uint8_t* idx, void* stream);
int sy11_maxpool5_bwd(int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, const void* dy, int32_t dy_ld,
                      const uint8_t* idx, void* dx, int32_t dx_ld, int32_t accumulate, void* stream);
/* flat dtype cast (f32 <-> f16 / bf16), n elements                                                          */
/* backward of a bias conv with f32 output (Detect's last 1x1 convs, nn/modules/head.py:44-55; autograd of nn.Conv2d bias +
 * autocast's cast of the incoming gradient): dz f32 (M x N, pixel stride dz_ld) -> dy (dtype, M x npad contiguous, channels >= N
 * zero) and dbias[c] += sum_m dz[m][c] (dbias may be NULL).  partials != NULL ([partial_rows][N] scratch): ordered reduction —
 * one partial row per workgroup, folded in row order by a second launch (bit-reproducible).                             */
int sy11_bias_grad_cast(int32_t dtype, int64_t M, int32_t N, int32_t npad, const float* dz, int32_t dz_ld, void* dy, float* dbias,
                        float* partials, int32_t partial_rows, void* stream);
int sy11_cast(int32_t src_dtype, int32_t dst_dtype, int64_t n, const void* src, void* dst, void* stream);

/* ---- C2PSA attention core: softmax(q^T k * scale) applied to v (nn/modules/block.py:1925-1931) ---------- */
/* qkv: (B, N, heads*(2*kd+hd)) NHWC pixels, per head [q(kd) k(kd) v(hd)];  o: (B, N, heads*hd);
 * p (f32, B*heads*N*N) receives the attention probabilities (kept for backward).                            */
int sy11_attention_fwd(int32_t dtype, int32_t B, int32_t N, int32_t heads, int32_t kd, int32_t hd, const void* qkv,
                       int32_t qkv_ld, void* o, int32_t o_ld, float* p, void* stream);
/* workspace: caller-allocated, sy11_attention_workspace_bytes(B, N, heads) bytes (f32 B*heads*N*N: the generic kernels
 * stage dS there; the MFMA path only uses its first B*heads*N floats for the per-query row sums).                    */
int sy11_attention_bwd(int32_t dtype, int32_t B, int32_t N, int32_t heads, int32_t kd, int32_t hd, const void* qkv,
                       int32_t qkv_ld, const float* p, const void* d_o, int32_t do_ld, void* dqkv, int32_t dqkv_ld,
                       float* workspace, void* stream);
/* the same with the forward output o (B, N, heads*hd) at hand: the per-query row sums of softmax's backward are dO . o, so the MFMA path
 * reads P once instead of twice (o == NULL: identical to sy11_attention_bwd).  autograd's SoftmaxBackward of
 * `attn.softmax(dim=-1)` (nn/modules/block.py:1928) — same sums, taken from the product instead of the factors.            */
int sy11_attention_bwd_o(int32_t dtype, int32_t B, int32_t N, int32_t heads, int32_t kd, int32_t hd, const void* qkv,
                         int32_t qkv_ld, const float* p, const void* o, int32_t o_ld, const void* d_o, int32_t do_ld, void* dqkv,
                         int32_t dqkv_ld, float* workspace, void* stream);
size_t sy11_attention_workspace_bytes(int32_t B, int32_t N, int32_t heads);

/* ---- Detect decode + NMS (nn/modules/head.py:100-131; utils/ops.py:181-332 + torchvision.ops.nms) ------- */
/* maps: 3 NHWC f32 maps (B,H_l,W_l,64+nc); out: (B, 4+nc, A) f32 exactly as Detect._inference returns it.   */
int sy11_detect_decode(int32_t B, int32_t nc, int32_t nl, const float* const* maps, const int32_t* hs,
                       const int32_t* ws, const float* strides, float* out, void* stream);
/* greedy NMS over n candidate boxes ALREADY sorted by (score desc, index asc): keep[i] in {0,1}.
 * boxes: (n,4) xyxy f32 (class offset already added).  workspace: n*ceil(n/64) uint64 words.               */
int sy11_nms_sorted(int32_t n, const float* boxes, float iou_thres, uint64_t* workspace, uint8_t* keep,
                    void* stream);
size_t sy11_nms_workspace_bytes(int32_t n);
/* The same for `nseg` images at once: image i owns counts[i] consecutive rows of boxes / keep (HOST array; rows of an image in
 * score-descending order).  Images run side by side; each sweep stops after `max_keep` survivors (ops.py:322 keeps at most max_det
 * rows per image) and clears the rest of its keep flags.  workspace: as many bytes as the ..._workspace_bytes query below returns.  */
int sy11_nms_sorted_batched(int32_t nseg, const int32_t* counts, const float* boxes, float iou_thres, int32_t max_keep,
                            uint64_t* workspace, uint8_t* keep, void* stream);
size_t sy11_nms_batched_workspace_bytes(int32_t nseg, const int32_t* counts);
/* Candidate selection of non_max_suppression (utils/ops.py:246-292: `x[xc]`, the multi-label `where(cls > conf_thres)` / the
 * best-class `max`, in the reference's candidate order image -> anchor -> class) straight from the (B, D = 4 + nc + nm, A) tensor
 * Detect returns.  Two calls: with blk_offset = NULL it COUNTS, blk_count[b * ceil(A / 256) + k] = candidates of anchors
 * [256 k, 256 k + 256) of image b; with blk_offset = the exclusive prefix sum of those counts it WRITES, per candidate,
 * key = segment << 32 | ~bits(score) (a stable ascending sort of the keys = per segment, score descending, ties in candidate order),
 * its anchor and its class; segment = image, or image * nc + class with segment_by_class.  conf_thres >= 0.          */
int sy11_nms_candidates(int32_t B, int32_t D, int32_t A, int32_t nc, float conf_thres, int32_t multi_label, int32_t segment_by_class,
                        const float* pred, const int32_t* blk_offset, int32_t* blk_count, int64_t* key, int32_t* anchor, int32_t* cls,
                        void* stream);
/* sy11_nms_sorted_batched with the segment list on the DEVICE: rows seg_start[s] .. seg_start[s + 1] (nseg + 1 entries) and first
 * mask word seg_ws[s] of segment s; max_n = the longest segment (host).  One segment per (image, class) is the reference's batched
 * NMS (boxes shifted by class * max_wh never intersect across classes, utils/ops.py:307-312) with n^2 / (2 nc) pair tests.      */
int sy11_nms_sorted_segments(int32_t nseg, const int32_t* seg_start, const int64_t* seg_ws, int32_t max_n, const float* boxes,
                             float iou_thres, int32_t max_keep, uint64_t* workspace, uint8_t* keep, void* stream);
/* Seam merge of a long-capture scan (no reference counterpart): the per-window NMS survivors of all W windows — n rows of
 * {window index, (x1, y1, x2, y2) window-local f32 pixels (16-byte aligned array), score, class}, rows grouped by window in
 * ascending window order, start[w] (int64 frames, DEVICE array, non-decreasing) the first strip frame of window w — are suppressed
 * greedily and class-aware (agnostic != 0: across classes) in strip coordinates X = start[w] + x: boxes are visited by (score
 * descending, row ascending) and a box is dropped when an already-kept one has metric > thres with it (strict), metric 0 = IoU
 * inter / (a_i + a_j - inter), 1 = IoS inter / min(a_i, a_j).  Pairs are evaluated in f64 relative to one of the two windows, so
 * starts of 1e9 frames and beyond keep their sub-pixel part.  keep[i] in {0, 1}.  workspace: caller-allocated, 16-byte aligned,
 * as many bytes as the ..._workspace_bytes query below returns (O(n): no pair matrix).  Synchronises the stream (one host read
 * per four passes).                                                                                                          */
int sy11_scan_merge(int32_t n, int32_t W, int32_t n_frames, const int32_t* window, const float* boxes, const float* score,
                    const int32_t* cls, const int64_t* start, int32_t metric, float thres, int32_t agnostic, void* workspace,
                    uint8_t* keep, void* stream);
size_t sy11_scan_merge_workspace_bytes(int32_t n, int32_t W);
/* Link the boxes of one emission into tracks (no reference counterpart): n rows of rect = [t0_s, f_lo_hz, t1_s, f_hi_hz] f64
 * (16-byte aligned array, finite, t1 >= t0, f_hi >= f_lo, rows SORTED by t0 ascending) and their classes.  Rows i != j of one class
 * (agnostic != 0: of any classes) are linked when ov_t >= -gap_t and ov_f >= align * min(bw_i, bw_j), or, with use_f != 0, when
 * ov_f >= -gap_f and ov_t >= align * min(dur_i, dur_j); ov_t = min(t1) - max(t0), ov_f = min(f_hi) - max(f_lo), dur = t1 - t0,
 * bw = f_hi - f_lo, all in f64 with no contraction, so a host evaluation decides every pair identically.  label[i] = the smallest
 * row of i's connected component: unique, whatever the scheduling.  gap_t >= 0, gap_f >= 0 (ignored without use_f), 0 < align <= 1.
 * Hook-and-compress on the labels with integer atomicMin; pairs are recomputed per pass over the contiguous candidate range of
 * each row.  workspace: caller-allocated, 16-byte aligned, as many bytes as the ..._workspace_bytes query below returns (O(n): no
 * pair matrix, no edge list).  *passes (HOST, may be NULL): hook passes run — a few, not O(chain length).  Synchronises the stream
 * (one host read per two passes).                                                                                              */
int sy11_scan_link(int32_t n, const double* rect, const int32_t* cls, double gap_t, double gap_f, int32_t use_f, double align,
                   int32_t agnostic, void* workspace, int32_t* label, int32_t* passes, void* stream);
size_t sy11_scan_link_workspace_bytes(int32_t n);

/* ---- fused detection criterion (v8DetectionLoss.__call__, utils/loss.py:221-275; TaskAlignedAssigner, utils/tal.py:40-296;
 *      bbox_iou CIoU, utils/metrics.py:171-234).  maps: nl NHWC f32 head maps (B, H_l*W_l, 64+nc); gt: (B, G, 5) rows
 *      [cls, x1, y1, x2, y2] in pixels, all-zero rows are padding.  Workspaces are caller-allocated:
 *      pbox (B,A,4) f32, align/overlap (B,G,A) f32, topk (B,G,10) i32, assign (B,A) i32, pos (2,B,G) f32 zeroed,
 *      norm (B,A) f32, sums (64,4) f32 zeroed: per-slot partials of {sum(target_scores), box, cls, dfl}.            */
int sy11_det_loss_assign(int32_t B, int32_t nc, int32_t nl, const float* const* maps, const int32_t* hs, const int32_t* ws,
                         const float* strides, int32_t G, const float* gt, float* pbox, float* align, float* overlap,
                         int32_t* topk, int32_t* assign, float* pos, float* norm, float* sums, void* stream);
/* un-normalised loss sums: sums[.][1..3] += sum (1-CIoU)*w, sum BCE, sum DFL*w                                      */
int sy11_det_loss_terms(int32_t B, int32_t nc, int32_t nl, const float* const* maps, const int32_t* hs, const int32_t* ws,
                        const float* strides, int32_t G, const float* gt, const int32_t* assign, const float* norm,
                        float* sums, void* stream);
/* dmaps[l] = d(B * (gb*box + gc*cls + gd*dfl) / tss) / d maps[l], scaled by the DEVICE scalar *upstream and, when given, by the
 * second device scalar *inv_tss (out[4] of sy11_det_loss_finish); with inv_tss = NULL `upstream` must already carry
 * 1 / max(tss, 1).  No host synchronisation.                                                                       */
int sy11_det_loss_bwd(int32_t B, int32_t nc, int32_t nl, const float* const* maps, float* const* dmaps, const int32_t* hs,
                      const int32_t* ws, const float* strides, int32_t G, const float* gt, const int32_t* assign,
                      const float* norm, const float* upstream, const float* inv_tss, float gain_box, float gain_cls,
                      float gain_dfl, void* stream);
/* v8DetectionLoss.preprocess (utils/loss.py:194-207): n targets given as three strided f32 columns (image index, class, xywh
 * normalised; strides in elements) -> gt (B, G, 5) [cls, x1, y1, x2, y2] in pixels (scale_w / scale_h = image width / height),
 * an image's targets in their original order, the rest of its G rows zero.  G = the largest target count of one image.  */
int sy11_det_loss_pack_targets(int32_t n, int32_t B, int32_t G, const float* batch_idx, int32_t idx_stride, const float* cls,
                               int32_t cls_stride, const float* bboxes, int32_t box_stride, float scale_w, float scale_h, float* gt,
                               void* stream);
/* loss.py:268-275: out[0] = batch_size * sum_i gain_i * term_i / max(tss, 1), out[1..3] = the gained items, out[4] = 1 / max(tss, 1);
 * the 64 slots of `sums` are folded in index order.                                                                  */
int sy11_det_loss_finish(const float* sums, int32_t B, float gain_box, float gain_cls, float gain_dfl, float* out, void* stream);

/* ---- trainer step over flat buffers (engine/trainer.py:585-593 optimizer_step: GradScaler.unscale_ -> clip_grad_norm_(10.0) ->
 *      optimizer.step -> GradScaler.update -> zero_grad -> ModelEMA.update, utils/torch_utils.py:495-531; the optimizers are
 *      torch.optim.SGD(nesterov=True) / AdamW as built by build_optimizer, trainer.py:758-819).  Two launches:
 *      sy11_opt_grad_norm writes `nparts` ordered partial sums of (grad / scale)^2 plus snapshots of 1/scale and of the Adam
 *      step counter into ws (sy11_opt_workspace_floats(nparts) floats); sy11_opt_step folds them in a fixed order (bit-
 *      reproducible clip factor), applies the update to param / mom (/ sq), averages the UPDATED parameters and the float
 *      buffers into the EMA, zeroes grad, and updates the loss scale like GradScaler.update.  A non-finite norm with amp = 1
 *      skips the parameter update (GradScaler.step) but not the EMA.  Flat buffers: three consecutive groups ending at
 *      group_end[0..2] (multiples of 4), all 16-byte aligned.                                                            */
typedef struct sy11_opt_desc {
  int64_t n;                   /* elements of param / grad / mom / sq / ema                                      */
  int64_t n_buf;               /* elements of buf / ema_buf (BatchNorm running statistics), may be 0             */
  int64_t group_end[3];        /* end of each parameter group inside the flat buffers                            */
  float lr[3], momentum[3], weight_decay[3];    /* AdamW: momentum = beta1                                      */
  int32_t kind;                /* 0 SGD nesterov (dampening 0), 1 AdamW (decoupled decay), 2 Adam (L2 in the gradient) */
  float beta2, eps;            /* AdamW                                                                          */
  float max_norm;              /* clip_grad_norm_ threshold (10.0)                                               */
  float ema_decay;             /* d of this update: ema = d * ema + (1 - d) * value                              */
  int32_t amp;                 /* 1: gradients carry the loss scale; overflow skips the update                   */
  float growth_factor, backoff_factor; int32_t growth_interval;      /* GradScaler: 2.0, 0.5, 2000              */
  int32_t nparts;              /* partial sums written by sy11_opt_grad_norm (<= 4096)                           */
} sy11_opt_desc;
int sy11_opt_workspace_floats(int32_t nparts);
int sy11_opt_grad_norm(int64_t n, const float* grad, const float* scale, const float* adam_step, float* ws, int32_t nparts,
                       void* stream);
/* scale / growth_tracker: GradScaler's device scalars (updated in place; NULL with amp = 0); adam_step: device f32 count of
 * applied AdamW steps (updated in place; NULL for SGD); norm_out: optional [2] = {total gradient norm, update skipped}.  */
int sy11_opt_step(const sy11_opt_desc* d, float* param, float* grad, float* mom, float* sq, float* ema, const float* buf,
                  float* ema_buf, const float* ws, float* scale, int32_t* growth_tracker, float* adam_step, float* norm_out,
                  void* stream);

/* ---- IQ -> STFT -> power -> mel -> log producer (no reference code: README.md:7; spec in DESIGN.md) ------ */
/* iq: (B, L) interleaved complex64; db: (B, n_frames, n_mel) f32 dB (frame-major: coalesced stores);
 * minmax: (B,2) f32 [min,max] per image
 * (must be pre-filled with +inf/-inf by the caller or by sy11_stft_minmax_init).
 * n_fft: a power of two in [64, 8192].  window: n_fft f32 taps; mel_start: n_mel int32 first bins (0 <= start < n_fft);
 * mel_w: (n_mel, mel_taps) f32, a tap at bin >= n_fft does not exist (zero padding may follow the last real tap); with n_fft = 1024 and
 * mel_taps = 8 mel_w must be 16-byte aligned.                                                                  */
int sy11_stft_logmel(int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t n_frames, int32_t n_mel,
                     const float* iq, const float* window, const int32_t* mel_start, const float* mel_w,
                     int32_t mel_taps, float* db, float* minmax, void* stream);
int sy11_stft_minmax_init(int32_t B, float* minmax, void* stream);
/* img[b,c,f,t] = (db[b,t,f]-min)/(max-min), c = 0..2, NCHW f32 (what preprocess_batch hands the model)        */
int sy11_stft_normalize(int32_t B, int32_t n_mel, int32_t n_frames, const float* db, const float* minmax,
                        float* img_nchw, void* stream);
/* Windows from one strip (long-capture scan): db_strip is the (F, n_mel) dB output of sy11_stft_logmel called with B = 1 and
 * n_frames = F; window w is the n_frames consecutive frames from start[w] (DEVICE array, relative to the strip's first frame,
 * 0 <= start[w] <= F - n_frames; frames outside the strip read as nothing).  minmax (W, 2): min / max over exactly the window's
 * n_frames x n_mel rectangle; img (W, 3, n_mel, n_frames) = sy11_stft_normalize's arithmetic per window.  frame_minmax: caller-
 * allocated scratch of 2 F floats (the per-frame partials: overlapping windows do not re-read the strip).  W <= 65535.        */
int sy11_stft_windows(int32_t F, int32_t n_mel, int32_t n_frames, int32_t W, const int32_t* start, const float* db_strip,
                      float* minmax, float* frame_minmax, float* img_nchw, void* stream);

/* ---- image side of preprocess --------------------------------------------------------------
 * batch["img"].float() / 255 of DetectionTrainer.preprocess_batch (models/yolo/detect/train.py:59): n uint8 values
 * -> dtype (true division by 255.0f then rounding to dtype)                                                        */
int sy11_image_u8_to_float(int32_t dtype, int64_t n, const uint8_t* x, void* y, void* stream);
/* the multi_scale branch of preprocess_batch (models/yolo/detect/train.py:60-73): F.interpolate(imgs size=ns
 * mode="bilinear" align_corners=False) on `planes` = B*C planes of IH x IW -> OH x OW.  x_dtype may be SY11_U8:
 * the taps are then divided by 255 first (uint8 batch resized in the same pass)                                    */
int sy11_image_resize_bilinear(int32_t x_dtype, int32_t y_dtype, int32_t planes, int32_t IH, int32_t IW, int32_t OH,
                               int32_t OW, const void* x, void* y, void* stream);
/* LetterBox.__call__ (data/augment.py:1544-1591) fused with BasePredictor.preprocess (engine/predictor.py:118-136):
 * src (sh x sw x 3) uint8 HWC -> cv2.resize(INTER_LINEAR) to new_h x new_w placed at (top left) on an H x W canvas
 * filled with `fill` (114); reverse_c swaps channel 0 and 2 (BGR->RGB); chw=1 writes (3 H W) planes else (H W 3);
 * dtype SY11_U8 keeps bytes (the dataset stage) otherwise value / 255 in dtype (the predictor stage).
 * The 8-bit bilinear follows OpenCV imgproc/src/resize.cpp (opencv-python is a reference dependency and is not
 * vendored): 11-bit coefficients; the ((b*(S>>4))>>16 + ... + 2)>>2 vertical pass; exact 2x shrink = 2x2 box mean */
int sy11_image_letterbox(int32_t dtype, int32_t sh, int32_t sw, int32_t H, int32_t W, int32_t new_h, int32_t new_w,
                         int32_t top, int32_t left, int32_t fill, int32_t reverse_c, int32_t chw,
                         const uint8_t* src, void* dst, void* stream);
/* One training sample of the augmentation pipeline in a single launch (data/augment.py: Mosaic._mosaic4 :660-715 then
 * RandomPerspective.affine_transform :1000-1078 then RandomHSV :1303-1390 then RandomFlip :1393-1474 then the
 * transpose / channel flip of Format._format_img :2070-2107).  The mosaic canvas (canvas_h x canvas_w filled with
 * `fill`) is virtual: tile t (tile_src[t] = device pointer to an (h w 3) uint8 image) covers canvas
 * [x1 x2) x [y1 y2) and canvas pixel (x y) reads source pixel (x - padw  y - padh); tile_geom holds 8 int32 per
 * tile in the order h w x1 y1 x2 y2 padw padh.  minv = the 6 doubles of the INVERTED 2x3 map exactly as
 * cv::warpAffine computes them (NULL: no warp and the output is the canvas); hsv_lut = 768 bytes hue|sat|val
 * tables (NULL: no HSV step).  tile_src / tile_geom / minv / hsv_lut are HOST arrays (copied into the launch).
 * Output H x W written as with sy11_image_letterbox (dtype SY11_U8 or float / 255; chw; reverse_c).
 * cv2.warpAffine and cv2.cvtColor are restated from OpenCV 4.x (imgwarp.cpp fixed-point INTER_LINEAR path;
 * color_hsv.simd.hpp RGB2HSV_b / HSV2RGB_b): opencv-python is an un-vendored reference dependency              */
int sy11_image_mosaic_warp(int32_t dtype, int32_t n_tiles, const uint8_t* const* tile_src, const int32_t* tile_geom,
                           int32_t canvas_h, int32_t canvas_w, const double* minv, int32_t H, int32_t W,
                           const uint8_t* hsv_lut, int32_t flip_ud, int32_t flip_lr, int32_t fill,
                           int32_t reverse_c, int32_t chw, void* dst, void* stream);

/* MixUp (data/augment.py: BaseMixTransform.__call__ :386-407, MixUp.get_indexes :919, MixUp._mix_transform :944-949,
 * placed by v8_transforms :2310-2342 after Mosaic + RandomPerspective and before RandomHSV / RandomFlip) folded into
 * the same single launch: TWO geometry recipes, each as in sy11_image_mosaic_warp (n_tiles, tile_src, tile_geom,
 * canvas_h/w, minv or NULL), both producing H x W.  Every output pixel samples recipe a (the sample) and recipe b (the
 * partner) and blends per channel as numpy does in (img * r + img2 * (1 - r)).astype(np.uint8): two float64 products
 * and one float64 sum, each rounded on its own (never an fma), then truncation.  r and one_minus_r are BOTH passed,
 * formed by the host in float64, finite and in [0 1].  Then the shared tail of sy11_image_mosaic_warp: hsv_lut, the
 * two flips (of the blended image), fill (the border of both canvases and warps), reverse_c, chw, dtype.
 * Every argument check of sy11_image_mosaic_warp applies to each recipe; nothing is launched on an error.          */
int sy11_image_mixup_warp(int32_t dtype, int32_t n_tiles_a, const uint8_t* const* tile_src_a, const int32_t* tile_geom_a,
                          int32_t canvas_h_a, int32_t canvas_w_a, const double* minv_a, int32_t n_tiles_b,
                          const uint8_t* const* tile_src_b, const int32_t* tile_geom_b, int32_t canvas_h_b,
                          int32_t canvas_w_b, const double* minv_b, double r, double one_minus_r, int32_t H, int32_t W,
                          const uint8_t* hsv_lut, int32_t flip_ud, int32_t flip_lr, int32_t fill,
                          int32_t reverse_c, int32_t chw, void* dst, void* stream);

/* ---- IQ side of the training loader (no reference code: the reference trains from rendered images; spec in DESIGN.md §4) ----
 * One launch gathers a window of L samples per batch row out of captures resident in device memory and applies the IQ-domain
 * augmentation recipe of that row:
 *   out[b n] = gain rot(c(src[off + n])  phi0 + n dphi) + gain2 rot(c2(src2[off2 + n])  phi02 + n dphi2) + sigma w(seed  n)
 * src = (const complex64*) src_ptr[b], off = src_off[b] in SAMPLES (may be odd); c / c2 = optional conjugate (flags).
 * dphi / phi0: uint32 fractions of a cycle; phi0 + n dphi is taken in wrapping uint32 arithmetic (exact for every n) and becomes
 * an angle in [-pi pi) for one sincos.  w: unit-variance complex normal from Philox4x32-10 with key = seed and counter
 * (n / 2  0  0  0): words 0 1 give sample 2k, words 2 3 sample 2k + 1, each by Box-Muller on (x + 0.5) 2^-32 (radius sqrt(-ln u1),
 * angle 2 pi u2), so a sample depends on (seed n) only.  src2 = 0: no partner.  Steps that are off are skipped: gain 1, dphi =
 * phi0 = 0, no conjugate, no partner, sigma 0 copies the source bit for bit.
 * src_ptr / src_off / r are DEVICE arrays of B entries; out (B L) interleaved complex64.  The caller guarantees that
 * [off  off + L) and [off2  off2 + L) lie inside their captures.  B <= 65535 and B * L < 2^31.                          */
enum { SY11_IQ_CONJ = 1, SY11_IQ_CONJ2 = 2 };
typedef struct sy11_iq_recipe {
  uint32_t dphi, phi0;         /* phase step per sample and phase of sample 0, in 2^-32 cycles                    */
  float gain, sigma;           /* linear gain of the sample's own window; noise standard deviation (complex)      */
  uint64_t seed;               /* Philox key                                                                      */
  uint64_t src2;               /* partner capture (device address of complex64 samples) or 0                      */
  int64_t off2;                /* partner's first sample                                                          */
  uint32_t dphi2, phi02;
  float gain2;
  uint32_t flags;              /* SY11_IQ_CONJ | SY11_IQ_CONJ2                                                    */
} sy11_iq_recipe;
int sy11_iq_gather_augment(int32_t B, int32_t L, const uint64_t* src_ptr, const int64_t* src_off, const sy11_iq_recipe* r,
                           float* out, void* stream);

/* ---- digital down-converter at the front of a scan: mix -> low-pass -> rational resample (spec in DESIGN.md §4) ----
 *   y[m] = sum_{j < T} taps[phi  j] xm[i0 - j]    i0 = floor((m Q + c) / P)    phi = (m Q + c) mod P
 *   xm[i] = x[i] e^{j 2 pi frac(i dphi / 2^32)}   x = 0 outside in[]
 * for the outputs m0 <= m < m0 + M of a capture resampled by P / Q.  taps: DEVICE (P T) f32 polyphase table of a low-pass with
 * centre tap c at the P-times up-sampled rate (entry [phi j] = h[phi + j P]; sy11/data/resample.py builds it).  in: complex64
 * samples n0 <= i < n0 + n_in (absolute indices of the capture); the caller guarantees that they cover every sample of the capture
 * the outputs read - [floor((m0 Q + c) / P) - T + 1   floor(((m0 + M - 1) Q + c) / P)] - and everything outside in[] reads as zero.
 * The mixer phase (uint32) i * dphi wraps in uint32 arithmetic (exact for every i); the rotation is evaluated in float64 and rounded
 * to float32 once, per INPUT sample; dphi = 0 skips the mixer.  Every output is one sequential f32 sum over j = 0 .. T - 1, so a value depends on
 * (m  capture) only, never on the launch shape or on how the caller cut the capture into calls.  P == Q: no filter, out[m] = xm[m]
 * (in[] must hold the samples m0 .. m0 + M - 1).  P Q <= 4096, 1/64 <= P/Q <= 64, c < P T, M and n_in below 2^31; in / out 8-byte
 * aligned (in may start at an odd sample of its allocation).  Nothing is launched on an error.                            */
int sy11_iq_resample(int32_t P, int32_t Q, int32_t T, int32_t c, const float* taps, int64_t n0, int32_t n_in, const float* in,
                     uint32_t dphi, int64_t m0, int32_t M, float* out, void* stream);

/* ---- polyphase analysis filter bank: all K bands of a capture from one read of its samples (spec in DESIGN.md §4) ----
 *   y_k[m] = sum_n h[n] x[m D + c - n] e^{-j 2 pi k (m D + c - n) / K}    x = 0 outside in[]
 *          = sum_{r < K} e^{-j 2 pi k r / K} v_m[r]    v_m[r] = sum_{i = r (mod K)} h[m D + c - i] x[i]
 * for the time steps m0 <= m < m0 + M and every channel 0 <= k < K: channel k is sy11_iq_resample with P = 1, Q = D and
 * dphi = (-k 2^32 / K) mod 2^32.  K a power of two in [2, 64]; D = K (critically sampled) or K / 2 (2x oversampled); taps: DEVICE N =
 * 32 D + 1 f32 of the low-pass of the DDC for 1 / D, centre c = 16 D; twiddle: DEVICE K / 2 complex64 e^{-j 2 pi t / K} (built on the
 * host in float64, rounded once).  in: complex64 samples n0 <= i < n0 + n_in (absolute indices i of the capture, which also fix the
 * residue r = i mod K: a chunk cut anywhere gives the same values); the caller guarantees that they cover every sample of the
 * capture the outputs read - [m0 D + c - N + 1   (m0 + M - 1) D + c] - and everything outside in[] reads as zero.
 * out[k out_stride + (m - m0)]: complex64, channel-major, out_stride >= M complex samples between channels.  Every v_m[r] is one
 * sequential f32 sum in ascending tap index and the K-point FFT runs in one fixed order (radix-2 decimation in frequency), so a value
 * depends on (k  m  capture) only, never on the tile, the launch shape or on how the caller cut the capture into calls.  n0, m0 >= 0,
 * m0 < 2^48, M and n_in positive and below 2^31; in / out 8-byte aligned (in may start at an odd sample of its allocation).
 * Nothing is launched on an error.                                                                                        */
int sy11_iq_channelize(int32_t K, int32_t D, int32_t N, int32_t c, const float* taps, const float* twiddle, int64_t n0, int32_t n_in,
                       const float* in, int64_t m0, int32_t M, int64_t out_stride, float* out, void* stream);

/* ---- extraction: every detection of a scan as baseband IQ, all of them in one launch (spec in DESIGN.md §4) ----
 *   out[out_off + (m - m0)] = sum_{j < T} taps_D[j] xm[m D + 16 D - j]    T = 32 D + 1    D = 2^log2d
 *   xm[i] = x[i] e^{j 2 pi frac(i dphi / 2^32)}                             x = 0 outside in[]
 * for the outputs m0 <= m < m0 + M of every segment: sy11_iq_resample with P = 1, Q = D, c = 16 D, the same table and the same mixer,
 * bit for bit (one sequential f32 sum over j = 0 .. T - 1 per output).  log2d = 0: no filter, out = xm (the DDC's mixer).  A segment is a
 * clip or a piece of one; output m of a segment sits on capture sample m D.
 * taps: DEVICE f32, the tables of D = 1, 2 .. 64 one after the other, each padded to a multiple of 4 floats: D = 1 is the single tap
 * 1.0 at float 0, D = 2^l >= 2 is the low-pass of the DDC for 1 / D (32 D + 1 taps) at float 32 D - 64 + 4 l; 4060 floats in all
 * (sy11/data/extract.py builds it).  seg: DEVICE n_seg segments; tile: DEVICE n_tile pairs (segment, first output relative to its m0),
 * one per workgroup, first a multiple of sy11_iq_extract_tile(log2d) - every output belongs to the tile that starts at or before it.
 * seg_host / tile_host: HOST copies of the two tables; they are checked entry by entry before anything is launched: no segment may
 * read samples outside in[] - [(m0 - 16) D   (m0 + M + 15) D] clipped to the capture [0  n_total), or [m0  m0 + M) for D = 1 - or write
 * outside out[0  out_len), and every output must lie on the capture ((m0 + M - 1) D < n_total).  in: complex64 samples n0 <= i < n0 +
 * n_in (absolute indices of the capture; in may start at an odd sample of its allocation); out: out_len complex64 samples.  A value
 * depends on (m  D  dphi  capture) only, never on the tile, the segment or how the caller cut the capture into calls.
 * Nothing is launched on an error.                                                                                      */
typedef struct sy11_iq_segment {
  int64_t m0;                  /* first output (absolute index on the grid of decimation D: capture sample m0 D)   */
  int64_t out_off;             /* first complex64 sample of the segment in out                                     */
  int32_t M;                   /* number of outputs                                                                */
  int32_t log2d;               /* log2 of the decimation, 0 .. 6                                                   */
  uint32_t dphi;               /* mixer step per input sample, in 2^-32 cycles                                     */
  int32_t reserved;            /* 0                                                                                */
} sy11_iq_segment;
int32_t sy11_iq_extract_tile(int32_t log2d);      /* outputs per workgroup at decimation 2^log2d (0: log2d out of range) */
int sy11_iq_extract(int32_t n_seg, const sy11_iq_segment* seg_host, const sy11_iq_segment* seg, int32_t n_tile,
                    const int32_t* tile_host, const int32_t* tile, const float* taps, int64_t n_total, int64_t n0, int32_t n_in,
                    const float* in, int64_t out_len, float* out, void* stream);

/* ---- measurement: Welch power spectrum, noise, bandwidth and centroid of every detection of a scan (spec in DESIGN.md §4) ----
 * N = n_fft in {64 128 256 512 1024}, H = N / 2.  Frame j is the capture's samples [j H  j H + N), anchored at sample 0;
 *   X_j[k] = sum_{i < N} window[i] x[j H + i] e^{-2 pi i k i / N}     k = 0 .. N - 1 (bin k >= N / 2 is the signed bin k - N)
 * Frames are grouped on their absolute index, G = the value of sy11_iq_psd_group frames per group.
 *
 * Stage 1, sy11_iq_psd.  An item is the frames [j0  j0 + nf) of one box, all of ONE group (1 <= nf <= G).  Per item
 *   partial[row N + k]     = f32(sum_j |X_j[k]|^2)                          frames ascending, one after the other
 *   env[env_off + (j - j0)] = f32((sum_{k_lo <= k <= k_hi} |X_j[k]|^2) / nw2)   signed bins; only when env != NULL
 * computed in float64 (the product window[i] x is exact there) and rounded once, to the f32 that is stored.
 * window: DEVICE N f32; twiddle: DEVICE N / 2 complex128, e^{-2 pi i m / N}, 16-byte aligned; nw2 = N sum window^2 in float64.  item: DEVICE n_item
 * items; item_host: a HOST copy, checked entry by entry before anything is launched: no item may read samples outside in[] -
 * [j0 H  (j0 + nf - 1) H + N), which must also lie on the capture [0  n_total) - or write outside partial[0  n_rows N) or
 * env[0  env_len), every row is written by one item of the call, and -N/2 <= k_lo <= k_hi < N/2.  in: complex64 samples
 * n0 <= i < n0 + n_in (absolute indices of the capture; in may start at an odd sample of its allocation).  The FFT runs in one fixed
 * order (radix-2 decimation in frequency) and so does every sum, so a value depends on (box  frames  capture) only, never on the
 * launch shape, the item's place in the table or on how the caller cut the capture into calls.  No atomics.
 * Nothing is launched on an error.
 *
 * Stage 2, sy11_psd_measure: one launch after the last stage-1 call, float64 throughout, every product and sum rounded on its own.
 * Per box, with the rows row0 .. row0 + n_rows - 1 of partial (its groups, ascending):
 *   P[k]         = (sum over the rows of partial[row N + (k mod N)], ascending, one after the other) scale      -N/2 <= k < N/2
 *   noise_median = the median (mean of the two middle values for an even count) of P over the noise bins: -noise_l <= k <= noise_l - 1
 *                  and k outside [s_lo  s_hi];   NaN when there are none;    nd = noise_median corr
 *   p_in         = sum of P[k], k_lo <= k <= k_hi, ascending
 *   c[k]         = max(P[k] - nd  0), or P[k] when there are no noise bins;   sum_c = sum of c[k], sum_kc = sum of k c[k] over
 *                  s_lo <= k <= s_hi, ascending
 *   k_dn, k_up   = the first k at which the running sum of c reaches frac_lo sum_c and frac_hi sum_c
 * psd: n_box N float64, psd[b N + k + N/2] = P[k]; out_f: n_box 4 float64 (p_in  noise_median  sum_c  sum_kc); out_i: n_box 4 int32
 * (k_dn  k_up  n_in  n_noise).  box: DEVICE table, box_host: its HOST copy, checked before the launch (rows inside partial[0  n_rows N),
 * -N/2 <= s_lo <= k_lo <= k_hi <= s_hi < N/2, 0 <= noise_l <= N/2, scale and corr positive and finite).
 * Nothing is launched on an error.                                                                                      */
typedef struct sy11_psd_item {
  int64_t j0;                  /* first frame (absolute index: capture sample j0 H)                                */
  int64_t env_off;             /* first f32 of the item's frames in env (ignored when env is NULL)                 */
  int32_t nf;                  /* number of frames, 1 .. G, all with the same j / G                                */
  int32_t row;                 /* row of the partial table the item writes                                         */
  int32_t k_lo, k_hi;          /* the box's signed bins, for the envelope                                          */
} sy11_psd_item;
typedef struct sy11_psd_box {
  int64_t row0;                /* first row of the box in the partial table                                        */
  int32_t n_rows;              /* its number of rows (groups)                                                      */
  int32_t k_lo, k_hi;          /* in-box bins (signed)                                                             */
  int32_t s_lo, s_hi;          /* search span                                                                      */
  int32_t noise_l;             /* noise bins lie in [-noise_l  noise_l - 1]                                        */
  double scale;                /* 1 / (J N W2)                                                                     */
  double corr;                 /* median-to-mean correction, 1 / (1 - 1 / (9 J))^3                                 */
} sy11_psd_box;
int32_t sy11_iq_psd_group(void);                  /* G: frames per group, a constant of the build */
int sy11_iq_psd(int32_t n_fft, int32_t n_item, const sy11_psd_item* item_host, const sy11_psd_item* item, const float* window,
                const double* twiddle, double nw2, int64_t n_total, int64_t n0, int32_t n_in, const float* in, int64_t n_rows,
                float* partial, int64_t env_len, float* env, void* stream);
int sy11_psd_measure(int32_t n_fft, int32_t n_box, const sy11_psd_box* box_host, const sy11_psd_box* box, double frac_lo,
                     double frac_hi, int64_t n_rows, const float* partial, double* psd, double* out_f, int32_t* out_i,
                     void* stream);

/* ---- characterisation: symbol rate, carrier offset and kurtosis of every clip of an extraction (spec in DESIGN.md §4) ----
 * N = n_fft in {64 128 256 512 1024}, H = N / 2.  A clip is len complex64 samples at in[off]; its frame j is the clip's samples
 * [j H  j H + N), j = 0 .. J - 1, J = (len - N) / H + 1.  With x a sample, y_0 = |x|^2, y_1 = x^2, y_2 = x^4 (formed in float64) and
 *   Y_q,j[k] = sum_{i < N} window[i] y_q[j H + i] e^{-2 pi i k i / N}     k = 0 .. N - 1 (bin k >= N / 2 is the signed bin k - N)
 * Frames are grouped on their index in the clip, G = the value of sy11_iq_cyclo_group frames per group.
 *
 * Stage 1, sy11_iq_cyclo.  An item is the frames [j0  j0 + nf) of one clip, all of ONE group (1 <= nf <= G).  Per item
 *   partial[(row 3 + q) N + k] = f32(sum_j |Y_q,j[k]|^2)                    frames ascending, one after the other;  q = 0, 1, 2
 *   mom[row 4 + 0 .. 3]        = sum of Re x^2, Im x^2, |x|^2, |x|^4 over the clip's samples [j0 H  (j0 + nf) H), and with last = 1
 *                                over [j0 H  (j0 + nf - 1) H + N): the items of a clip count every sample of its frames once
 * computed in float64; a partial value is rounded once, to the f32 that is stored.  window, twiddle: the tables of sy11_iq_psd.  item: DEVICE
 * n_item items; item_host: a HOST copy, checked entry by entry before anything is launched: the clip lies inside in[0  n_in) and holds a
 * frame, the item's frames are frames of the clip and of one group, last = 1 exactly on the item that ends the clip, and every row of
 * partial[0  n_rows 3 N) / mom[0  n_rows 4) is written by one item of the call.  in: the packed complex64 clips (a clip may start
 * at an odd sample).  One fixed order for the FFT and for every sum: a value depends on (clip  frames) only.  No atomics.
 * Nothing is launched on an error.
 *
 * Stage 2, sy11_cyclo_peaks: one launch, one workgroup per (clip, q), float64 throughout, every product and sum rounded on its own.
 * With the rows row0 .. row0 + n_rows - 1 of partial (the clip's groups, ascending):
 *   P_q[k]  = (sum over the rows of partial[(row 3 + q) N + (k mod N)], ascending, one after the other) scale      -N/2 <= k < N/2
 *   search  = k_min <= k <= N/2 - 1 for q = 0 (the spectrum of a real sequence is symmetric; DC and the window's main lobe stay out),
 *             every k for q = 1, 2;   peak = the first maximum of P_q over it in ascending k;   median over it as in sy11_psd_measure
 * spectra: n_clip 3 N float64, spectra[(clip 3 + q) N + k + N/2] = P_q[k].  out: n_clip 22 float64 per clip: at 4 q: P_q[peak]  P_q[peak - 1]
 * P_q[peak + 1] (cyclic)  median;  12 .. 15: the clip's moments (Re m20  Im m20  m21  m42), its rows of mom added ascending;  16 + 2 q: peak,
 * 17 + 2 q: the size of the search set (integers, exact in float64).  row: DEVICE table, row_host: its HOST copy, checked before the
 * launch (rows inside partial, clip < n_clip and written once, 1 <= k_min <= N/2 - 1, scale positive and finite).  Entries of spectra
 * and out of clips that no row names are left alone.  Nothing is launched on an error.                                        */
typedef struct sy11_cyclo_item {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip, >= N                                                        */
  int32_t j0;                  /* first frame of the item (index in the clip)                                      */
  int32_t nf;                  /* number of frames, 1 .. G, all with the same j / G                                */
  int32_t row;                 /* row of the partial and moment tables the item writes                             */
  int32_t last;                /* 1: the item ends the clip and owns the last frame's second half; else 0          */
} sy11_cyclo_item;
typedef struct sy11_cyclo_row {
  int64_t row0;                /* first row of the clip in the partial table                                       */
  int32_t n_rows;              /* its number of rows (groups)                                                      */
  int32_t clip;                /* the row of spectra / out it writes                                               */
  int32_t k_min;               /* q = 0 searches [k_min  N/2 - 1]                                                  */
  int32_t reserved;            /* 0                                                                                */
  double scale;                /* 1 / (J N W2)                                                                     */
} sy11_cyclo_row;
int32_t sy11_iq_cyclo_group(void);                /* G: frames per group, a constant of the build */
int sy11_iq_cyclo(int32_t n_fft, int32_t n_item, const sy11_cyclo_item* item_host, const sy11_cyclo_item* item, const float* window,
                  const double* twiddle, int64_t n_in, const float* in, int64_t n_rows, float* partial, double* mom, void* stream);
int sy11_cyclo_peaks(int32_t n_fft, int32_t n_row, const sy11_cyclo_row* row_host, const sy11_cyclo_row* row, int64_t n_rows,
                     const float* partial, const double* mom, int32_t n_clip, double* spectra, double* out, void* stream);

/* ---- demodulation: the symbol stream and its error-vector magnitude of every clip of an extraction (spec in DESIGN.md §4) ----
 * Feed-forward, three launches over all clips; the two fits between them are the caller's (sy11/data/demodulate.py).  A phase is an
 * exact integer: sample n of a clip turns by (n W mod 2^64) 2^-64 cycles, whatever the tile it is computed in.
 *
 * Launch 1, sy11_iq_demod_filter.  An item is one tile of TILE = the value of sy11_iq_demod_tile usable samples [n0  n0 + cnt) of the
 * clip in[off  off + len): the usable span is [hw  len - hw), n0 - hw a multiple of TILE, cnt = TILE except on the clip's last tile.
 *   xr[n] = in[n] e^{-2 pi i (n wc mod 2^64) 2^-64}       y[n] = sum_{|k| <= hw} xr[n - k] taps[tap_off + hw + k]   (zeros outside the clip)
 * in float64 (the taps ascending in -k, fused multiply-adds) and rounded ONCE to the float32 written to y[off + n] for the item's usable samples, and for n < hw by the
 * item with first = 1, for n >= len - hw by the item with last = 1: the items of a clip write every y[n] of the clip once.  Per item
 *   rows[row 3 + 0 .. 2] = Re, Im of sum |y[n]|^2 e^{-2 pi i (n ws mod 2^64) 2^-64} and sum |y[n]|^2 over its usable samples
 * in float64 from the stored float32 y.  item: DEVICE table, item_host: its HOST copy, checked entry by entry before anything is launched:
 * the clip lies inside in[0  n_in), n_taps = 2 hw + 1 <= 513 taps lie inside taps[0  n_tap), the tile is a tile of the usable span,
 * first / last say what they must, and every row of rows[0  n_rows 3) is written by one item.  in, y: packed complex64 (a clip may
 * start at an odd sample).  One fixed order for every sum; no atomics.  Nothing is launched on an error.
 *
 * Launch 2, sy11_demod_symbols.  An item is 1 .. 256 consecutive symbols of one clip: symbol i sits at t0 + i step = (k + mu) 2^32
 * (Q32.32, mu cut to its top 24 bits) and is the 4-point cubic Lagrange interpolation of y[off + k - 1 .. k + 2] at mu, in float64 and rounded once, written
 * to sym[sym_off + i].  rows[row 3 + 0 .. 2] = Re, Im of sum s_i^order (negated at order 4) and sum |s_i|^2, float64 from the stored s.
 * Checked: 1 <= k <= len - 3 for every symbol, 2^32 <= step <= 2^40, the symbols inside sym[0  n_sym), order 2 or 4, one item per row.
 *
 * Launch 3, sy11_demod_decide.  An item is block b of the nb = ceil(n_sym / block) blocks of a clip's symbols sym[sym_off  sym_off + n_sym);
 * theta[row0 + q] is the carrier phase at the centre q block + (n_q - 1) / 2 of block q.  phi_i is theta interpolated linearly between the
 * centres and constant outside them, r_i = s_i e^{-i phi_i}, all in float64 and rounded once to float32 -> r[sym_off + i];
 * d[sym_off + i] = (Re r < 0) at order 2, 2 (Re r < 0) + (Im r < 0) at order 4;  rows[(row0 + b) 3 + 0 .. 2] = sum |r|^2, sum Re(r conj(p)),
 * n over the block, p the unit point that d names.  Checked: the symbols inside sym[0  n_sym), 8 <= block <= 256, nb and b as above, the
 * rows inside the tables, order 2 or 4, one item per row.                                                                       */
typedef struct sy11_demod_item {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip                                                              */
  int64_t n0;                  /* first usable sample of the tile (index in the clip)                              */
  int64_t tap_off;             /* first tap of the clip in the tap buffer                                          */
  uint64_t wc;                 /* carrier: cycles per sample 2^64, wrapping                                        */
  uint64_t ws;                 /* symbol rate: cycles per sample 2^64                                              */
  int32_t cnt;                 /* usable samples of the tile, 1 .. TILE                                            */
  int32_t hw;                  /* half width of the filter                                                         */
  int32_t n_taps;              /* 2 hw + 1                                                                         */
  int32_t row;                 /* row of the table the item writes                                                 */
  int32_t first;               /* 1: the clip's first tile, which also writes y[0  hw); else 0                     */
  int32_t last;                /* 1: the clip's last tile, which also writes y[len - hw  len); else 0              */
} sy11_demod_item;
typedef struct sy11_demod_block {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip                                                              */
  int64_t t0;                  /* position of the item's first symbol, Q32.32 samples from the clip's first        */
  int64_t step;                /* samples per symbol, Q32.32                                                       */
  int64_t sym_off;             /* the item's first symbol in the packed symbol buffer                              */
  int32_t n;                   /* symbols, 1 .. 256                                                                */
  int32_t order;               /* 2 or 4                                                                           */
  int32_t row;                 /* row of the table the item writes                                                 */
  int32_t reserved;            /* 0                                                                                */
} sy11_demod_block;
typedef struct sy11_demod_dec {
  int64_t sym_off;             /* the clip's first symbol in the packed symbol buffer                              */
  int64_t n_sym;               /* symbols of the clip                                                              */
  int64_t row0;                /* the clip's first row of theta and of the output table                            */
  int32_t nb;                  /* blocks of the clip                                                               */
  int32_t b;                   /* the item's block                                                                 */
  int32_t block;               /* symbols per block, 8 .. 256                                                      */
  int32_t order;               /* 2 or 4                                                                           */
} sy11_demod_dec;
int32_t sy11_iq_demod_tile(void);                 /* TILE: usable samples per item of launch 1, a constant of the build */
int sy11_iq_demod_filter(int32_t n_item, const sy11_demod_item* item_host, const sy11_demod_item* item, int64_t n_tap, const float* taps,
                         int64_t n_in, const float* in, float* y, int64_t n_rows, double* rows, void* stream);
int sy11_demod_symbols(int32_t n_item, const sy11_demod_block* item_host, const sy11_demod_block* item, int64_t n_in, const float* y,
                       int64_t n_sym, float* sym, int64_t n_rows, double* rows, void* stream);
int sy11_demod_decide(int32_t n_item, const sy11_demod_dec* item_host, const sy11_demod_dec* item, int64_t n_sym, const float* sym,
                      int64_t n_rows, const double* theta, float* r, uint8_t* d, double* rows, void* stream);

/* ---- frequency-keyed demodulation: 2-FSK / GFSK / GMSK clips of an extraction by their discriminator (spec in DESIGN.md §4) ----
 * Feed-forward, three launches over all clips; the two fits between them are the caller's (sy11/data/demodulate_fsk.py).  The result has the
 * shape of the demodulation's at order 2: real symbols around +-1, stored as complex64 with a zero imaginary part.
 *
 * Launch 1, sy11_iq_fsk_filter.  An item is one tile of TILE = the value of sy11_iq_demod_tile usable samples [n0  n0 + cnt) of the clip
 * in[off  off + len): the usable span is [hw + 1  len - hw), n0 - hw - 1 a multiple of TILE, cnt = TILE except on the clip's last tile.
 *   f[n] = arg(in[n] conj(in[n - 1]) e^{-2 pi i wc 2^-64}) / 2 pi  (cycles per sample, 1 <= n < len)     y[n] = sum_{|k| <= hw} f[n - k] taps[tap_off + hw + k]
 * in float64 (f once per sample, the taps ascending in -k, fused multiply-adds) and rounded ONCE to the float32 written to y[off + n] for the item's usable
 * samples; the item with first = 1 also writes the zeros of y[off  off + hw + 1), the item with last = 1 those of y[off + len - hw  off + len): the items of a clip
 * write every y[n] of the clip once.  Per item, with w[n] = e^{-2 pi i (n ws mod 2^64) 2^-64},
 *   rows[row 8 + 0 .. 7] = Re, Im of sum y^2 w;  Re, Im of sum y w;  Re, Im of sum w;  sum y;  sum y^2     over its usable samples
 * in float64 from the stored float32 y.  item: DEVICE table, item_host: its HOST copy, checked entry by entry before anything is launched:
 * the clip lies inside in[0  n_in), n_taps = 2 hw + 1 <= 513 taps lie inside taps[0  n_tap), the tile is a tile of the usable span,
 * first / last say what they must, and every row of rows[0  n_rows 8) is written by one item.  in: packed complex64 (a clip may start at an
 * odd sample), y: n_in float32, packed like in.  One fixed order for every sum; no atomics.  Nothing is launched on an error.
 *
 * Launch 2, sy11_fsk_symbols.  An item is 1 .. 256 consecutive symbols of one clip: symbol i sits at t0 + i step = (k + mu) 2^32
 * (Q32.32, mu cut to its top 24 bits) and is the 4-point cubic Lagrange interpolation of y[off + k - 1 .. k + 2] at mu, in float64 and rounded once, written
 * to sym[sym_off + i] (float32).  rows[row 4 + 0 .. 3] = the number of s_i >= m, their sum, the sum of the s_i < m, and sum s_i^2, float64 from the stored s.
 * Checked: 1 <= k <= len - 3 for every symbol, 2^32 <= step <= 2^40, the symbols inside sym[0  n_sym), m finite, one item per row.
 *
 * Launch 3, sy11_fsk_decide.  An item is 1 .. 256 consecutive symbols sym[sym_off  sym_off + n):  r_i = (s_i - f0) / dev in float64, rounded once to
 * float32 -> r[2 (sym_off + i)] with r[2 (sym_off + i) + 1] = 0;  d[sym_off + i] = (r_i < 0);  rows[row 3 + 0 .. 2] = sum r^2, sum |r|, n (the columns
 * of sy11_demod_decide at order 2).  Checked: the symbols inside sym[0  n_sym) (r: n_sym complex64, d: n_sym bytes), f0 finite, dev finite and > 0,
 * one item per row.                                                                                                              */
typedef struct sy11_fsk_item {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip                                                              */
  int64_t n0;                  /* first usable sample of the tile (index in the clip)                              */
  int64_t tap_off;             /* first tap of the clip in the tap buffer                                          */
  uint64_t wc;                 /* carrier: cycles per sample 2^64, wrapping                                        */
  uint64_t ws;                 /* symbol rate: cycles per sample 2^64                                              */
  int32_t cnt;                 /* usable samples of the tile, 1 .. TILE                                            */
  int32_t hw;                  /* half width of the filter                                                         */
  int32_t n_taps;              /* 2 hw + 1                                                                         */
  int32_t row;                 /* row of the table the item writes                                                 */
  int32_t first;               /* 1: the clip's first tile, which also zeroes y[0  hw + 1); else 0                 */
  int32_t last;                /* 1: the clip's last tile, which also zeroes y[len - hw  len); else 0              */
} sy11_fsk_item;
typedef struct sy11_fsk_block {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip                                                              */
  int64_t t0;                  /* position of the item's first symbol, Q32.32 samples from the clip's first        */
  int64_t step;                /* samples per symbol, Q32.32                                                       */
  int64_t sym_off;             /* the item's first symbol in the packed symbol buffer                              */
  double m;                    /* the clip's mean of y: the level that splits the two tones                        */
  int32_t n;                   /* symbols, 1 .. 256                                                                */
  int32_t row;                 /* row of the table the item writes                                                 */
} sy11_fsk_block;
typedef struct sy11_fsk_dec {
  int64_t sym_off;             /* the item's first symbol in the packed symbol buffer                              */
  double f0;                   /* the clip's level midpoint, cycles per sample                                     */
  double dev;                  /* the clip's deviation, cycles per sample, > 0                                     */
  int32_t n;                   /* symbols, 1 .. 256                                                                */
  int32_t row;                 /* row of the table the item writes                                                 */
} sy11_fsk_dec;
int sy11_iq_fsk_filter(int32_t n_item, const sy11_fsk_item* item_host, const sy11_fsk_item* item, int64_t n_tap, const float* taps,
                       int64_t n_in, const float* in, float* y, int64_t n_rows, double* rows, void* stream);
int sy11_fsk_symbols(int32_t n_item, const sy11_fsk_block* item_host, const sy11_fsk_block* item, int64_t n_in, const float* y,
                     int64_t n_sym, float* sym, int64_t n_rows, double* rows, void* stream);
int sy11_fsk_decide(int32_t n_item, const sy11_fsk_dec* item_host, const sy11_fsk_dec* item, int64_t n_sym, const float* sym, float* r,
                    uint8_t* d, int64_t n_rows, double* rows, void* stream);

/* ---- OFDM demodulation: cyclic-prefix OFDM clips of an extraction with fixed, uniformly spaced pilots (spec in DESIGN.md §4) ----
 * Feed-forward, three launches over all clips; the two fits between them are the caller's (sy11/data/demodulate_ofdm.py).  The result has the
 * shape of the demodulation's: the data carriers of every OFDM symbol, one after the other, as corrected symbols and decisions.  A clip has an
 * FFT size N = n_fft in {64, 128, 256, 512, 1024}, a prefix of G samples (1 <= G <= N / 2), a period S = N + G and Lp = (len - N) / S whole periods;
 * the clips of one call may differ in all of them.
 *
 * Launch 1, sy11_iq_ofdm_fold.  An item is a tile of 64 residues [r0  r0 + cnt_r) of the period (r0 a multiple of 64, cnt_r = min(64, S - r0)) and
 * a split of 16 periods [m0  m0 + cnt_m) of the clip (m0 a multiple of 16, cnt_m = 16 except on the clip's last split).  Per residue r, in float64,
 * the periods in ascending order (the products of two float32 values are exact):
 *   F = sum_m in[r + m S + N] conj(in[r + m S])     E = sum_m (|in[r + m S]|^2 + |in[r + m S + N]|^2) / 2     out[3 (out_off + r - r0) + 0 .. 2] = Re F, Im F, E
 * item: DEVICE table, item_host: its HOST copy, checked entry by entry before anything is launched: n_fft is in the set, the clip lies inside
 * in[0  n_in), the residues are a tile and the periods a split of the clip's, and every triple of out[0  3 n_out) is written by one item.
 * in: packed complex64 (a clip may start at an odd sample).  No atomics.  Nothing is launched on an error.
 *
 * Launch 2, sy11_ofdm_fft.  An item is 1 .. 1024 / N consecutive OFDM symbols of one clip; symbol f of the item transforms the N samples from
 * start + f S of the clip:  v[q] = in[n] e^{-2 pi i (n w mod 2^64) 2^-64} (n = start + f S + q, float64),  Y[k] = (sum_q v[q] e^{-2 pi i k q / N}) e^{+2 pi i k a / N}
 * (the advance turn is entry (k a) mod N of the twiddle table: exact).  The item's carriers are bin[bin_off  bin_off + n_used): signed k in
 * (-N / 2, N / 2), ascending; pil = 0 for a data carrier, +-(p + 1) for pilot p of n_pil with the value +-1.  Per symbol f and carrier j:
 *   yc[2 (yc_off + f n_used + j)] = f32(Y[k_j]) (rounded ONCE)     pil[2 (pil_off + f n_pil + p)] = +-Y[k_j] (float64)     pw[pow_off + f] = sum_j |Y[k_j]|^2 (float64)
 * twiddle: e^{-2 pi i m / 1024}, m < 512, as (Re, Im) float64 pairs, 16-byte aligned: the table of every N is a stride of it.  Checked: n_fft in the set,
 * S and a fit it, the symbols lie inside the clip and the clip inside in[0  n_in), the carriers are ascending and inside (-N / 2, N / 2) and name
 * every pilot once, and every entry of yc, pil and pw is written by one item.
 *
 * Launch 3, sy11_ofdm_decide.  An item is one OFDM symbol: its n_used carrier values yc[yc_off ..] and its n_data data carriers
 * car[car_off  car_off + n_data), each the index idx of its value among the used ones and its turn tau = (tr, ti).  In float64, rounded ONCE:
 *   r_j = f32((yc[yc_off + idx_j] rho) tau_j) -> r[2 (sym_off + j)]     d[sym_off + j] as sy11_demod_decide at the item's order     rows[row 3 + 0 .. 2] = sum |r|^2, sum Re(r conj(point(d))), n_data
 * Checked: the values inside yc[0  n_yc), the symbols inside r / d (n_sym entries) and written by one item, idx < n_used, rho and every tau finite,
 * order 2 or 4, one item per row.                                                                                                  */
typedef struct sy11_ofdm_fold_item {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip                                                              */
  int64_t out_off;             /* the triple of residue r0 in the item's partial row                               */
  int32_t n_fft;               /* N                                                                                */
  int32_t S;                   /* the period, N + G                                                                */
  int32_t r0;                  /* first residue of the tile, a multiple of 64                                      */
  int32_t cnt_r;               /* residues of the tile, min(64, S - r0)                                            */
  int32_t m0;                  /* first period of the split, a multiple of 16                                      */
  int32_t cnt_m;               /* periods of the split, 1 .. 16                                                    */
} sy11_ofdm_fold_item;
typedef struct sy11_ofdm_bin {
  int32_t k;                   /* signed carrier index, -N / 2 < k < N / 2                                         */
  int32_t pil;                 /* 0: a data carrier; +-(p + 1): pilot p with the value +-1                         */
} sy11_ofdm_bin;
typedef struct sy11_ofdm_fft_item {
  int64_t off;                 /* first sample of the clip in the packed buffer                                    */
  int64_t len;                 /* samples of the clip                                                              */
  int64_t start;               /* first sample of the item's first FFT window (index in the clip)                  */
  uint64_t w;                  /* carrier: cycles per sample 2^64, wrapping                                        */
  int64_t yc_off;              /* the item's first carrier value in yc (complex64 entries)                         */
  int64_t pil_off;             /* the item's first pilot value in pil (complex128 entries)                         */
  int64_t pow_off;             /* the item's first power row                                                       */
  int32_t n_fft;               /* N                                                                                */
  int32_t S;                   /* the period, N + G                                                                */
  int32_t a;                   /* the advance: samples the window starts inside the prefix, 0 .. G                 */
  int32_t nf;                  /* OFDM symbols of the item, 1 .. 1024 / N                                          */
  int32_t bin_off;             /* the clip's first carrier in the carrier table                                    */
  int32_t n_used;              /* its carriers, data and pilots, 1 .. N - 1                                        */
  int32_t n_pil;               /* its pilots, 1 .. n_used                                                          */
  int32_t reserved;
} sy11_ofdm_fft_item;
typedef struct sy11_ofdm_car {
  int32_t idx;                 /* the data carrier's place among the used carriers                                 */
  int32_t reserved;
  double tr;                   /* its turn tau, real part                                                          */
  double ti;                   /* and imaginary part                                                               */
} sy11_ofdm_car;
typedef struct sy11_ofdm_dec {
  int64_t yc_off;              /* the OFDM symbol's first carrier value in yc                                      */
  int64_t sym_off;             /* its first symbol in the packed symbol buffer                                     */
  double rho_r;                /* the symbol's correction rho, real part                                           */
  double rho_i;                /* and imaginary part                                                               */
  int32_t car_off;             /* the clip's first data carrier in the carrier table                               */
  int32_t n_data;              /* its data carriers, 1 .. n_used                                                   */
  int32_t n_used;              /* its used carriers, 1 .. 1023                                                     */
  int32_t order;               /* 2 or 4                                                                           */
  int32_t row;                 /* row of the table the item writes                                                 */
  int32_t reserved;
} sy11_ofdm_dec;
int sy11_iq_ofdm_fold(int32_t n_item, const sy11_ofdm_fold_item* item_host, const sy11_ofdm_fold_item* item, int64_t n_in, const float* in,
                      int64_t n_out, double* out, void* stream);
int sy11_ofdm_fft(int32_t n_item, const sy11_ofdm_fft_item* item_host, const sy11_ofdm_fft_item* item, int32_t n_bin, const sy11_ofdm_bin* bin_host,
                  const sy11_ofdm_bin* bin, const double* twiddle, int64_t n_in, const float* in, int64_t n_yc, float* yc, int64_t n_pil, double* pil,
                  int64_t n_pow, double* pw, void* stream);
int sy11_ofdm_decide(int32_t n_item, const sy11_ofdm_dec* item_host, const sy11_ofdm_dec* item, int32_t n_car, const sy11_ofdm_car* car_host,
                     const sy11_ofdm_car* car, int64_t n_yc, const float* yc, int64_t n_sym, float* r, uint8_t* d, int64_t n_rows, double* rows,
                     void* stream);

/* ---- frame search: where the sync words sit in the corrected symbols of every clip, and at which rotation (spec in DESIGN.md §4) ----
 * Three launches over all clips; between the second and the third the caller compacts the hits (sy11/data/frames.py).  sym: the packed
 * corrected symbols (complex64, what sy11_demod_decide wrote to r); words: packed DECISIONS of the words, one byte per symbol as d of
 * sy11_demod_decide holds them (bit 0 at order 2; 2 b0 + b1 at order 4; higher bits ignored).  A decision w names the un-normalised point
 * c = 1 - 2 w (order 2) or (1 - 2 (w >> 1)) + i (1 - 2 (w & 1)) (order 4), |c|^2 = order / 2.
 *
 * Launch 1, sy11_sync_correlate.  An item is one tile of TILE = the value of sy11_sync_tile positions [p0  p0 + cnt) of one pair (clip,
 * word): the clip is sym[sym_off  sym_off + n_sym), the word words[word_off  word_off + L), the pair has P = n_sym - L + 1 positions, p0 is a
 * multiple of TILE and cnt = TILE except on the pair's last tile.  For every position p, in float64 from the stored float32 symbols, k
 * ascending, every product and sum rounded on its own:
 *   Cr += re[p+k] Re c[k] + im[p+k] Im c[k]     Ci += im[p+k] Re c[k] - re[p+k] Im c[k]     E += re[p+k] re[p+k] + im[p+k] im[p+k]
 *   rho2[pos_off + p] = (Cr Cr + Ci Ci) / ((order / 2) L E), 0 where E == 0
 *   q[pos_off + p]    = Cr < 0 (order 2);  the index of the largest of (Cr, Ci, -Cr, -Ci), the lowest on a tie (order 4)
 * item: DEVICE table, item_host: its HOST copy, checked entry by entry before anything is launched: order 2 or 4, the clip inside
 * sym[0  n_sym), 8 <= L <= 256 and L <= n_sym, the word inside words[0  n_word), the tile a tile of [0  P), the pair's positions inside
 * [0  n_pos), and no position written by two items.  One fixed order for every sum; no atomics.  Nothing is launched on an error.
 *
 * Launch 2, sy11_sync_peaks.  The same item table, checked in the same way.  hit[pos_off + p] = 1 iff rho2[p] >= threshold2, no p' of
 * [p - L + 1  p) has rho2[p'] >= rho2[p] and no p' of (p  p + L - 1] has rho2[p'] > rho2[p] (windows clipped to [0  P)), else 0: of equal
 * peaks closer than L the earliest is the hit; a NaN is never one and never suppresses one.  0 < threshold2 <= 1.
 *
 * Launch 3, sy11_sync_frames.  A frame is a hit: position p of a pair, with the rotation q that launch 1 found.  v[k] = sym[sym_off + p + k]
 * turned back by q steps of 2 pi / order (negations and swaps: exact), decided as sy11_demod_decide decides, for k in [0  L + n_payload),
 * n_payload = min(payload, n_sym - p - L).  rows[row 3 + 0 .. 2] = the word symbols whose decision differs, the bits that differ,
 * n_payload.  bits[row stride  (row + 1) stride) = the payload's bits (1 per symbol at order 2; b0, b1 at order 4), MSB first, zeros after
 * them.  Checked: order 2 or 4, q < order, the clip and the word inside their buffers, 8 <= L <= 256, p + L <= n_sym, 0 <= payload < 2^20
 * and its ceil(payload log2(order) / 8) bytes inside a row of stride bytes, every row written by one frame.  bits may be null when stride
 * is 0.                                                                                                                          */
typedef struct sy11_sync_item {
  int64_t sym_off;             /* the clip's first symbol in the packed symbol buffer                              */
  int64_t n_sym;               /* symbols of the clip                                                              */
  int64_t word_off;            /* the word's first decision in the packed word buffer                              */
  int64_t pos_off;             /* the pair's first position in the packed position buffers                         */
  int64_t p0;                  /* first position of the tile (index in the pair)                                   */
  int32_t cnt;                 /* positions of the tile, 1 .. TILE                                                 */
  int32_t L;                   /* symbols of the word, 8 .. 256                                                    */
  int32_t order;               /* 2 or 4                                                                           */
  int32_t reserved;            /* 0                                                                                */
} sy11_sync_item;
typedef struct sy11_sync_frame {
  int64_t sym_off;             /* the clip's first symbol in the packed symbol buffer                              */
  int64_t n_sym;               /* symbols of the clip                                                              */
  int64_t word_off;            /* the word's first decision in the packed word buffer                              */
  int64_t p;                   /* position of the word's first symbol in the clip                                  */
  int32_t L;                   /* symbols of the word, 8 .. 256                                                    */
  int32_t order;               /* 2 or 4                                                                           */
  int32_t q;                   /* rotation: the symbols are turned back by q steps of 2 pi / order                 */
  int32_t payload;             /* payload symbols asked for after the word, 0 .. 2^20 - 1                          */
  int32_t row;                 /* row of the tables the frame writes                                               */
  int32_t reserved;            /* 0                                                                                */
} sy11_sync_frame;
int32_t sy11_sync_tile(void);                     /* TILE: positions per item of launches 1 and 2, a constant of the build */
int sy11_sync_correlate(int32_t n_item, const sy11_sync_item* item_host, const sy11_sync_item* item, int64_t n_word, const uint8_t* words,
                        int64_t n_sym, const float* sym, int64_t n_pos, double* rho2, uint8_t* q, void* stream);
int sy11_sync_peaks(int32_t n_item, const sy11_sync_item* item_host, const sy11_sync_item* item, int64_t n_word, int64_t n_sym, int64_t n_pos,
                    const double* rho2, double threshold2, uint8_t* hit, void* stream);
int sy11_sync_frames(int32_t n_frame, const sy11_sync_frame* frame_host, const sy11_sync_frame* frame, int64_t n_word, const uint8_t* words,
                     int64_t n_sym, const float* sym, int64_t n_rows, int32_t* rows, int64_t stride, uint8_t* bits, void* stream);

/* ---- equalisation: the sync-word least-squares equaliser of every found frame (spec in DESIGN.md §4) ----
 * Two launches (sy11/data/equalize.py), four when the taps are refined on the decisions of a first pass.  sym: the packed corrected symbols
 * (complex64, what sy11_demod_decide wrote to r), never written; words: packed decisions of the words as the frame search takes them.
 * taps = N, odd, 3 .. 15; D = (N - 1) / 2; a symbol outside its clip reads as 0.  A decision names a unit-modulus point: 1 - 2 d (order 2),
 * ((1 - 2 (d >> 1)) + i (1 - 2 (d & 1))) s with s = the float64 nearest 1 / sqrt(2) (order 4).
 *
 * Launch 1, sy11_eq_solve.  One wavefront per frame: the word words[word_off  word_off + L) at position p of the clip sym[sym_off  sym_off + n_sym),
 * found at rotation q, gain A.  Target t[k] = A point(word[k]) turned FORWARD by q steps of 2 pi / order (swaps and negations: exact) for k < L, and
 * A point(decisions[sym_off + p + k]) for L <= k < Lt (decisions: what launch 2 wrote in a first pass; may be null when Lt == L everywhere).  In
 * float64 from the stored float32 symbols, k ascending, with u_k[j] = r[p + k + D - j]:  R = sum_k conj(u_k) u_k^T,  z = sum_k conj(u_k) t[k];
 * R += reg (tr R / N) I;  R = G G^H (Cholesky);  w = R^-1 z by the two triangular solves.  w[row 30 + 2 j + 0 .. 1] = Re, Im of tap j, zeros from j = N
 * on.  rows[4 row + 0 .. 3] = mse_before = sum_(k<L) |r[p + k] - t[k]|^2 / (L A^2), mse_after = the same with w^T u_k for r[p + k], pivot_min = the
 * smallest G[a][a]^2 / (tr R / N) (tr R before reg is added), ok = 1.  A pivot that is not finite and positive, or a tap that is not finite: ok = 0,
 * w = the unit impulse at j = D, pivot_min = the failed pivot over tr R / N.  frame: DEVICE table, frame_host: its HOST copy, checked entry by entry
 * before anything is launched: order 2 or 4, q < order, the clip inside sym[0  n_sym), 1 <= L <= 256, L <= Lt <= 4096, the word inside
 * words[0  n_word), p >= 0 and p + Lt <= n_sym, the gain finite and positive, 0 <= reg <= 1, the row inside [0  n_rows) and written by one frame.
 * A sum depends neither on the launch's grouping nor on the frame's place in it; no atomics.  Nothing is launched and nothing written on an error.
 *
 * Launch 2, sy11_eq_apply.  A segment is the symbols [start  end) of a clip with one owner: row `frame` of w, or -1.  An item is tile `tile` of
 * TILE = the value of sy11_eq_tile symbols of segment `seg`.  With an owner  out[m] = f32(sum_j w[j] r[m + D - j]), in float64, j ascending,
 * re += (wr a) - (wi b), im += (wr b) + (wi a), every product and sum rounded on its own and the result rounded once to float32; without one
 * out[m] = sym[m] bit for bit.  decisions[m] = Re < 0 (order 2), 2 (Re < 0) + (Im < 0) (order 4) of out[m].  Checked: order 2 or 4, the clip inside
 * sym[0  n_sym), 0 <= start < end <= n_sym, the owner -1 or a row of w, no symbol inside two segments; every item a tile of a segment, none twice;
 * out is not sym.  No two items write the same symbol; no atomics.                                                                     */
typedef struct sy11_eq_frame {
  int64_t sym_off;             /* the clip's first symbol in the packed symbol buffer                              */
  int64_t n_sym;               /* symbols of the clip                                                              */
  int64_t word_off;            /* the word's first decision in the packed word buffer                              */
  int64_t p;                   /* position of the word's first symbol in the clip                                  */
  int32_t L;                   /* symbols of the word, 1 .. 256                                                    */
  int32_t Lt;                  /* training symbols, L .. 4096; those from L on are read from `decisions`           */
  int32_t order;               /* 2 or 4                                                                           */
  int32_t q;                   /* rotation: the word's points are turned forward by q steps of 2 pi / order        */
  int32_t row;                 /* row of w and rows the frame writes                                               */
  int32_t reserved;            /* 0                                                                                */
  double gain;                 /* A: the modulus of a clean symbol of the clip                                     */
} sy11_eq_frame;
typedef struct sy11_eq_segment {
  int64_t sym_off;             /* the clip's first symbol in the packed symbol buffer                              */
  int64_t n_sym;               /* symbols of the clip                                                              */
  int64_t start;               /* first symbol of the segment in the clip                                          */
  int64_t end;                 /* one past its last                                                                */
  int32_t frame;               /* the row of w that owns the segment, or -1: copied                                */
  int32_t order;               /* 2 or 4                                                                           */
} sy11_eq_segment;
typedef struct sy11_eq_item {
  int32_t seg;                 /* the segment                                                                      */
  int32_t tile;                /* symbols [start + tile TILE  min(start + (tile + 1) TILE, end)) of it              */
} sy11_eq_item;
int32_t sy11_eq_tile(void);                       /* TILE: symbols per item of launch 2, a constant of the build */
int sy11_eq_solve(int32_t n_frame, const sy11_eq_frame* frame_host, const sy11_eq_frame* frame, int32_t taps, double reg, int64_t n_word,
                  const uint8_t* words, int64_t n_sym, const float* sym, const uint8_t* decisions, int64_t n_rows, double* w, double* rows,
                  void* stream);
int sy11_eq_apply(int32_t n_item, const sy11_eq_item* item_host, const sy11_eq_item* item, int32_t n_seg, const sy11_eq_segment* seg_host,
                  const sy11_eq_segment* seg, int32_t taps, int64_t n_rows, const double* w, int64_t n_sym, const float* sym, float* out,
                  uint8_t* decisions, void* stream);

/* ---- frame decoding: soft bits, the Viterbi decoder of the rate 1/2, K = 7 code, de-whitening and CRC of every frame (spec in DESIGN.md §4) ----
 * Three launches over all frames (sy11/data/decode.py).  A frame's received stream starts at symbol sym_off of the packed corrected symbols
 * sym (complex64, what sy11_demod_decide wrote to r): the first symbol after its sync word.  w = log2(order) bits per symbol.  A frame has T
 * trellis steps, 1 <= T <= T_MAX = 8192, the value of sy11_fec_tmax, T >= 7 with a tail, and writes row `row` of every table of the call:
 * soft (n_rows, stride_soft) int8, bits (n_rows, stride_bits) uint8, out (n_rows, 2) int32, data (n_rows, stride_data) uint8, rows (n_rows, 5)
 * int32.  frame: DEVICE table, frame_host: its HOST copy, checked entry by entry before anything is launched: order 2 or 4, q < order, tail 0
 * or 1, T in range, the row inside the tables and written by one frame of the call, and what each launch adds below.  Nothing is launched on
 * an error.  Everything after the quantiser is integer arithmetic; no atomics; a frame's result does not depend on the other frames.
 *
 * The code: generators g0, g1, 7-bit integers with bits 6 and 0 set.  With input bit u_t and state s (6 bits, the newest input at bit 5):
 * R = (u_t << 6) | s, c[2t + j] = parity(R & g_j), next state R >> 1; the encoder starts in state 0.  With a tail the last 6 inputs are 0.
 *
 * Launch 1, sy11_fec_soft.  pattern: the puncture pattern over the mother stream c[0], c[1], ..., bit i of the word = position i, 1 = sent,
 * applied with the even period 2 .. 64 (nothing removed: period 2, pattern 3); at least one 1, none at or above `period`.  With `ones` the 1s of
 * a period, mother position j = full period + at holds received bit m = full ones + popcount(pattern & ((1 << at) - 1)) when bit `at` is set,
 * and an erasure otherwise.  Received bit m is component m % w (Re; Re then Im at order 4) of symbol m / w turned back by q steps of
 * 2 pi / order (negations and swaps: exact).  soft[row stride_soft + j] = clamp(rintf(x scale), -127, 127) for the float32 component x, ONE
 * float32 multiplication, 0 for a NaN product and for an erasure, j in [0  2T).  Positive means bit 0.  Checked too: the frame's
 * ceil(n_coded / w) symbols inside sym[0  n_sym), n_coded = the 1s of the pattern over [0  2T); 2T <= stride_soft (even); scale finite, > 0.
 *
 * Launch 2, sy11_fec_viterbi.  int32 path metrics, PM(0) = 0, PM(s != 0) = -2^30.  Step t, next state s', b in {0, 1}: R_b = (s' << 1) | b,
 * bm_b = sum_j (1 - 2 parity(R_b & g_j)) y[2t + j], m_b = PM(R_b & 63) + bm_b; d_t(s') = m_1 > m_0 (a tie keeps b = 0), PM'(s') = max(m_0, m_1).
 * No normalisation: |PM| <= 254 * 8192 + 2^30.  End state: 0 with a tail, else the state of the largest final metric, the lowest on a tie.
 * Traceback for t = T - 1 .. 0: u_t = s >> 5, s = ((s << 1) | d_t(s)) & 63.  bits[row stride_bits ...] = u_0 .. u_(T-1) packed MSB first,
 * zeros after them; out[2 row + 0 .. 1] = the end state's final metric, the end state.  One wavefront per frame, lane = state; 8 max(T) bytes
 * of dynamic LDS.  Checked too: the generators, 2T <= stride_soft (even, soft 2-byte aligned), ceil(T / 8) <= stride_bits.
 *
 * Launch 3, sy11_fec_check.  c^ = u_0 .. u_(T-1) encoded again from state 0.  n_channel = #{j : y[j] != 0}, channel_errors = #{j : y[j] != 0
 * and (y[j] < 0) != c^[j]}.  v_t = u_t ^ whiten[t], t < n_info (whiten: DEVICE, n_info bytes of 0 / 1, or null); data[row stride_data ...] = v
 * packed MSB first, zeros after them.  crc: HOST, the Rocksoft model; width 0 = none, else 8 .. 32 and n_info > width.  crc_recv = the last
 * `width` bits of v read MSB first; crc_calc runs over the n_info - width bits before them (with refin each group of 8 bits LSB first, and
 * the count a multiple of 8).  rows[5 row + 0 .. 4] = crc_calc, crc_recv (both uint32 bit patterns), crc_ok (1 / 0, -1 without a crc),
 * channel_errors, n_channel.  Checked too: T = n_info + 6 tail for every frame, the strides, the generators, the crc's fields.          */
typedef struct sy11_fec_frame {
  int64_t sym_off;             /* the frame's first payload symbol in the packed symbol buffer (launch 1 alone reads it) */
  int32_t T;                   /* trellis steps, 1 .. T_MAX (7 .. T_MAX with a tail)                                */
  int32_t order;               /* 2 or 4                                                                           */
  int32_t q;                   /* rotation: the symbols are turned back by q steps of 2 pi / order                 */
  int32_t tail;                /* 1: the last 6 inputs are 0 and the end state is 0; 0: the end state is free      */
  int32_t row;                 /* row of the tables the frame writes                                               */
  float scale;                 /* soft values per unit of a symbol's component (launch 1 alone reads it)           */
} sy11_fec_frame;
typedef struct sy11_fec_crc {
  int32_t width;               /* 0: no check; else 8 .. 32                                                        */
  uint32_t poly;               /* without the top bit                                                              */
  uint32_t init;
  uint32_t xorout;
  int32_t refin;               /* 0 or 1                                                                           */
  int32_t refout;              /* 0 or 1                                                                           */
} sy11_fec_crc;
int32_t sy11_fec_tmax(void);                      /* T_MAX: the trellis steps of a frame at the most, a constant of the build */
int sy11_fec_soft(int32_t n_frame, const sy11_fec_frame* frame_host, const sy11_fec_frame* frame, int32_t period, uint64_t pattern, int64_t n_sym,
                  const float* sym, int64_t n_rows, int64_t stride_soft, int8_t* soft, void* stream);
int sy11_fec_viterbi(int32_t n_frame, const sy11_fec_frame* frame_host, const sy11_fec_frame* frame, int32_t g0, int32_t g1, int64_t n_rows,
                     int64_t stride_soft, const int8_t* soft, int64_t stride_bits, uint8_t* bits, int32_t* out, void* stream);
int sy11_fec_check(int32_t n_frame, const sy11_fec_frame* frame_host, const sy11_fec_frame* frame, int32_t g0, int32_t g1, int32_t n_info,
                   const uint8_t* whiten, const sy11_fec_crc* crc, int64_t n_rows, int64_t stride_soft, const int8_t* soft, int64_t stride_bits,
                   const uint8_t* bits, int64_t stride_data, uint8_t* data, int32_t* rows, void* stream);

/* ---- frame correction: the Reed-Solomon outer code behind the frame decoder, with its byte interleaver (spec in DESIGN.md §4) ----
 * Two launches over all frames (sy11/data/correct.py).  Exact integer arithmetic; no atomics; a frame's result does not depend on the others.
 *
 * Field: GF(2^8) modulo `poly`, 9 bits with bit 8 set, primitive (x has order 255); alpha = 0x02.  Code: n bytes of which k carry information,
 * 1 <= k < n <= 255, nroots = n - k in [1, 64], t = nroots / 2 (rounded down), fcr in [0, 254], prim in [1, 254] with gcd(prim, 255) = 1.  A
 * codeword is the bytes c[0 .. n), c[0] the coefficient of x^(n-1); the first k are the information (systematic), the last nroots the parity.
 * c is a codeword iff S_j = sum_i c[i] alpha^(prim (fcr + j) (n - 1 - i)) = 0 for j in [0, nroots).  n < 255 is the shortened code: the missing
 * leading bytes are zero and not transmitted.  interleave = I in [1, 8] codewords lie byte by byte in a frame: byte offset + m of a frame's data
 * row, m in [0, I n), is byte m / I of codeword m % I (data as the frame decoder's launch 3 wrote it: the de-whitened bits packed MSB first).
 *
 * Both launches take the frames as a table of int32 rows: frame i reads row row[i] of data (n_rows, stride_data) uint8 and writes that row of
 * info (n_rows, stride_info) uint8, cw (n_rows, I, 2) int32 and rows (n_rows, 6) int32.  row: DEVICE, row_host: its HOST copy.  Checked before
 * anything is launched: the code's fields and the field polynomial as above, every row inside the tables and named once, offset >= 0,
 * offset + I n <= stride_data, I k <= stride_info, the alignment of the int32 tables.  Nothing is launched and nothing written on an error.
 *
 * Launch 1, sy11_rs_decode.  One work item per (frame, codeword w), received word r.  If a codeword c of the shortened code has Hamming
 * distance d(c, r) <= t it is unique and is the result: errors = d(c, r), bit_errors = popcount(c ^ r).  Otherwise errors = -1, bit_errors = 0
 * and the bytes pass through unchanged; so for a candidate of the full-length code that differs from r in an untransmitted byte, for a locator
 * polynomial whose degree is not its number of roots among the 255 positions, and for a degree above t.  nroots = 1 is t = 0: detection only.
 * info[row stride_info + w k + i] = c[i], i in [0, k): de-interleaved, codeword-major; the bytes of the row from I k on are not written.
 * cw[(row I + w) 2 + 0 .. 1] = errors, bit_errors.  One wavefront per codeword, whole frames per workgroup.
 *
 * Launch 2, sy11_rs_check.  One work item per frame.  rows[6 row + 0 .. 5] = n_failed (codewords with errors -1), the sum of errors and the sum
 * of bit_errors over the others, crc_calc, crc_recv (uint32 bit patterns), crc_ok (1 / 0, -1 without a crc).  crc: HOST, the Rocksoft model of
 * sy11_fec_crc; width 0 = none, else 8, 16, 24 or 32 and below the 8 I k information bits.  crc_recv = the last width / 8 bytes of info's I k,
 * MSB first; crc_calc runs over the bytes before them (with refin each byte LSB first).                                              */
typedef struct sy11_rs_code {
  int32_t n;                   /* bytes of a codeword, 2 .. 255                                                     */
  int32_t k;                   /* of which information, 1 .. n - 1, n - k <= 64                                     */
  int32_t fcr;                 /* the first of the consecutive roots, 0 .. 254                                      */
  int32_t prim;                /* the roots are powers of alpha^prim, 1 .. 254, coprime to 255                      */
  int32_t interleave;          /* codewords of a frame, 1 .. 8                                                      */
  int32_t poly;                /* the field polynomial with its bit 8, primitive                                    */
} sy11_rs_code;
int sy11_rs_decode(int32_t n_frame, const int32_t* row_host, const int32_t* row, const sy11_rs_code* code, int32_t offset, int64_t n_rows,
                   int64_t stride_data, const uint8_t* data, int64_t stride_info, uint8_t* info, int32_t* cw, void* stream);
int sy11_rs_check(int32_t n_frame, const int32_t* row_host, const int32_t* row, const sy11_rs_code* code, const sy11_fec_crc* crc, int64_t n_rows,
                  int64_t stride_info, const uint8_t* info, const int32_t* cw, int32_t* rows, void* stream);

/* ---- LDPC frame decoding: the layered normalised min-sum decoder of a quasi-cyclic LDPC code, de-whitening and CRC (spec in DESIGN.md §4) ----
 * Three launches over all frames (sy11/data/ldpc.py).  Launch 1 is sy11_fec_soft, unchanged, with T = N / 2, tail 0, period 2, pattern 3: it
 * writes the N int8 soft bits y of a frame, y > 0 = bit 0, 0 = an erasure.  Launches 2 and 3 take the frames as a table of int32 rows, as the
 * Reed-Solomon launches do: frame i reads row row[i] of soft (n_rows, stride_soft) int8 and writes that row of bits (n_rows, stride_bits) uint8,
 * out (n_rows, 2) int32, post (n_rows, stride_post) int16, data (n_rows, stride_data) uint8 and rows (n_rows, 5) int32.  row: DEVICE, row_host:
 * its HOST copy; every row inside the tables and named once.  Exact integer arithmetic; no atomics; a frame's result does not depend on the
 * others.  Nothing is launched and nothing written on an error.
 *
 * The code: an mb x nb base matrix over Z x Z circulants, 1 <= mb <= 64, mb < nb <= 128, 1 <= Z <= 512, N = nb Z even and at most N_MAX = 16384
 * (what launch 1 can write; the value of sy11_ldpc_nmax), M = mb Z, K = N - M; systematic: the first K bits of a codeword are the information.
 * Layer i holds the entries layer[i] .. layer[i + 1] of the entry table, 2 .. 32 of them, each a (column, shift) with column in [0, nb), no column
 * twice in a layer, and shift in [0, Z); layer[0] = 0, layer[mb] = n_entry; every column has an entry.  Entry j of layer i joins check
 * c = i Z + r to variable n_j = column Z + (r + shift) mod Z, r in [0, Z).  layer, entry: DEVICE; layer_host, entry_host: their HOST copies,
 * checked entry by entry before the launch.  sy11_ldpc_lds_bytes: the dynamic LDS the code takes, 2 N + 8 M + 4 n_entry + 4 (mb + 1) + 16 with
 * each part rounded up to 16 (-1 for a Z, mb, nb or n_entry outside the limits); a code that takes more than 160 KiB is refused.
 *
 * Launch 2, sy11_ldpc_decode.  Q[n] = y[n], R[c, j] = 0.  Iteration it = 1 .. iterations (1 .. 100), layer i = 0 .. mb - 1 in order, every check
 * c of the layer: T_j = Q[n_j] - R[c, j], s_j = T_j < 0, a_j = |T_j|; m1 = min_j a_j at j1 (any j attaining it), m2 = min over j != j1, S = XOR_j
 * s_j; R[c, j] = (S ^ s_j ? -1 : +1) min((scale (j == j1 ? m2 : m1)) >> 4, 127), Q[n_j] = T_j + R[c, j]; scale in [1, 16], sixteenths.  After the
 * mb layers x[n] = Q[n] < 0, unsat = #{c : XOR_j x[n_j] = 1}; the frame stops at unsat = 0.  |Q| <= 127 * 65: int16 holds it unclamped.
 * bits[row stride_bits ...] = x packed MSB first, zeros after the N bits to the end of the row; out[2 row + 0 .. 1] = iterations run, unsat;
 * post[row stride_post + n] = Q[n], n in [0, N) (post may be null; stride_post counts int16; what follows the N values is not written).  One
 * workgroup per frame, 64 threads per started 64 checks of a layer, 256 at the most.
 *
 * Launch 3, sy11_ldpc_check.  n_channel = #{n : y[n] != 0}, channel_errors = #{n : y[n] != 0 and (y[n] < 0) != x[n]}.  v_t = x_t ^ whiten[t],
 * t < K (whiten: DEVICE, K bytes of 0 / 1, or null); data[row stride_data ...] = v packed MSB first, zeros after them.  crc: HOST, the Rocksoft
 * model of sy11_fec_crc with the semantics of sy11_fec_check: width 0 = none, else 8 .. 32 and K > width; crc_recv = the last `width` bits of v,
 * crc_calc over the K - width bits before them.  rows[5 row + 0 .. 4] = crc_calc, crc_recv, crc_ok (1 / 0, -1 without a crc), channel_errors,
 * n_channel.  Checked too: N even in [2, N_MAX], 1 <= K < N, the strides.                                                              */
typedef struct sy11_ldpc_code {
  int32_t Z;                   /* the circulants' size, 1 .. 512                                                    */
  int32_t mb;                  /* block rows (layers), 1 .. 64                                                      */
  int32_t nb;                  /* block columns, mb + 1 .. 128, nb Z even and at most N_MAX                         */
  int32_t n_entry;             /* entries of the base matrix that are not -1                                        */
} sy11_ldpc_code;
typedef struct sy11_ldpc_entry {
  int32_t column;              /* block column, 0 .. nb - 1                                                         */
  int32_t shift;               /* row r of the block has its one in column (r + shift) mod Z, 0 .. Z - 1            */
} sy11_ldpc_entry;
int32_t sy11_ldpc_nmax(void);                     /* N_MAX: the bits of a codeword at the most, a constant of the build */
int64_t sy11_ldpc_lds_bytes(int32_t Z, int32_t mb, int32_t nb, int32_t n_entry);
int sy11_ldpc_decode(int32_t n_frame, const int32_t* row_host, const int32_t* row, const sy11_ldpc_code* code, const int32_t* layer_host,
                     const int32_t* layer, const sy11_ldpc_entry* entry_host, const sy11_ldpc_entry* entry, int32_t iterations, int32_t scale,
                     int64_t n_rows, int64_t stride_soft, const int8_t* soft, int64_t stride_bits, uint8_t* bits, int32_t* out,
                     int64_t stride_post, int16_t* post, void* stream);
int sy11_ldpc_check(int32_t n_frame, const int32_t* row_host, const int32_t* row, int32_t N, int32_t K, const uint8_t* whiten,
                    const sy11_fec_crc* crc, int64_t n_rows, int64_t stride_soft, const int8_t* soft, int64_t stride_bits, const uint8_t* bits,
                    int64_t stride_data, uint8_t* data, int32_t* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SY11_H */
