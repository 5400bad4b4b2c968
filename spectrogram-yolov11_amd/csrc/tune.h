// tune.h — first-call tile-shape selection for the GEMM-shaped kernels (igemm fwd/dgrad, wgrad).
//
// The best block tile depends on the layer (pixels vs channels vs reduction length vs how many workgroups the grid
// gets on 256 CUs) in ways the static heuristics only approximate (r01 sweeps: +-30 % per layer).  The first EAGER call
// of a given problem times every legal candidate on the caller's stream (2 launches each, HIP events) and caches the
// winner for the process; calls made while the stream is being captured into a hipGraph never measure — they use the
// cached pick or fall back to the heuristic, so graph capture stays legal.  SY11_TUNE=0 disables measuring,
// SY11_TUNE_LOG=1 prints every decision.
#pragma once
// sizes of the two tile-configuration tables (igemm.hip / wgrad.hip own the meaning of an index; core.hip validates imported picks
// against these — ONE definition, so that adding a configuration cannot leave the importer behind)
constexpr int SY11_IGEMM_NCFG = 26;
constexpr int SY11_WGRAD_NCFG = 20;

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <unordered_map>

// process-wide options (core.hip): defaults come from the environment (SY11_TUNE, SY11_TUNE_LOG, SY11_IGEMM_CFG,
// SY11_WGRAD_CFG, SY11_IGEMM_KORDER, SY11_IGEMM_DEEP, SY11_IGEMM_BPOL, SY11_MAXPOOL_SEP), sy11_set_option() changes them at run time
enum Sy11Opt { OPT_TUNE = 0, OPT_TUNE_LOG, OPT_IGEMM_CFG, OPT_WGRAD_CFG, OPT_IGEMM_KORDER, OPT_IGEMM_DEEP, OPT_IGEMM_BPOL, OPT_DGRAD_S2_HALO, OPT_ROW_MAP, OPT_DETERMINISTIC, OPT_MAXPOOL_SEP, OPT_DWGRAD_WG, OPT_DWGRAD_FUSED, OPT_COUNT };
int sy11_opt(int which);
// the configuration of the most recent launch of each table (core.hip), read-only through sy11_get_option as "igemm_last_cfg" /
// "wgrad_last_cfg"; -1 before the first launch.  One host-side int store per launch: tests read back which kernel they checked.
// The fused-parity stride-2 input gradient (conv3x3.hip halo_dgrad_s2_kernel) is no entry of the igemm table: it records this value.
constexpr int SY11_CFG_HALO_DGRAD_S2 = 100;
// The grouped filter-gradient launch (wgrad.hip wgrad16g_kernel, sy11_conv2d_wgrad_group) is no entry of the wgrad table either (it
// cannot be forced or imported): "wgrad_last_cfg" reads this value after it.
constexpr int SY11_CFG_WGRAD_GROUP = 100;
// The fused input + filter gradient of a 1x1 layer (dwgrad1x1.hip, sy11_conv2d_dgrad_wgrad_1x1) records this value as "wgrad_last_cfg".
// "dwgrad_wg" (SY11_DWGRAD_WG): workgroups per column block of that launch, 0 = one resident round (occupancy API).
// "dwgrad_fused" (SY11_DWGRAD_FUSED, default 1): the engine's switch — 0 keeps every layer on the pair; the entry point itself ignores it.
constexpr int SY11_CFG_DWGRAD_1X1 = 101;
void sy11_note_cfg(int kind, int cfg);     // kind 0 = igemm (fwd / dgrad), 1 = wgrad, 2 = stem forward, 3 = stem filter gradient,
                                            // 4 = 5x5 pool forward, 5 = 5x5 pool backward, 6 = channel-vector width of a data-movement launch
constexpr int SY11_NOTE_KINDS = 7;
// which of the first layer's kernels (direct.hip) the last sy11_stem_conv_fwd[_bn] / sy11_stem_conv_wgrad launched, read-only as
// "stem_fwd_last" / "stem_wgrad_last" (kinds 2 / 3 of sy11_note_cfg); -1 before the first launch
constexpr int SY11_STEM_GATHER = 1;         // stem_fwd_kernel / stem_wgrad_kernel: any dtype, N, leading dimension, geometry
constexpr int SY11_STEM_MMA = 2;            // stem_fwd_mma / stem_wgrad_mma: MFMA, operands gathered from the image
constexpr int SY11_STEM_TILE_VEC = 3;       // stem_fwd_tile / stem_wgrad_tile, image rows by 16-byte loads
constexpr int SY11_STEM_TILE_SCALAR = 4;    // stem_fwd_tile / stem_wgrad_tile, image rows element by element
// which 5x5 max-pool kernel (elementwise.hip) the last sy11_maxpool5_fwd / sy11_maxpool5_bwd launched, read-only as "pool_fwd_last" /
// "pool_bwd_last" (kinds 4 / 5); "maxpool_sep" 0 (SY11_MAXPOOL_SEP) keeps the 16-bit vector case on the 25-way kernels
constexpr int SY11_POOL_SCALAR = 1;         // maxpool5_fwd_kernel / maxpool5_bwd_kernel<T, 1>: 25-way, one element per thread
constexpr int SY11_POOL_VEC = 2;            // maxpool5_fwd_kernel / maxpool5_bwd_kernel<T, 16 / sizeof(T)>: 25-way, 16-byte channel vectors
constexpr int SY11_POOL_WALK = 3;           // maxpool5_fwd_sep_kernel / maxpool5_bwd_walk_kernel: 16-bit, five rows of one column per thread
// "ew_vec_last" (kind 6): the channel-vector width (1, 4 or 8 elements) of the last sy11_copy2d / sy11_upsample2x_fwd / sy11_upsample2x_bwd
constexpr int SY11_NOTE_POOL_FWD = 4, SY11_NOTE_POOL_BWD = 5, SY11_NOTE_EW_VEC = 6;

namespace sy11tune {

inline bool enabled() { return sy11_opt(OPT_TUNE) == 1; }
inline bool logging() { return sy11_opt(OPT_TUNE_LOG) == 1; }
inline bool capturing(hipStream_t st) {
  hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &s) != hipSuccess) { (void)hipGetLastError(); return true; }   // unknown -> do not measure
  return s != hipStreamCaptureStatusNone;
}
inline uint64_t hash(const int* v, int n) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < n; ++i) { h ^= (uint32_t)v[i]; h *= 1099511628211ull; }
  return h;
}

struct Cache {
  std::unordered_map<uint64_t, int> map;
  std::mutex mu;
  bool get(uint64_t k, int* out) {
    std::lock_guard<std::mutex> g(mu);
    auto it = map.find(k);
    if (it == map.end()) return false;
    *out = it->second;
    return true;
  }
  void put(uint64_t k, int v) {
    std::lock_guard<std::mutex> g(mu);
    map[k] = v;
  }
};
// the process's pick tables (core.hip): kind 0 = igemm (fwd / dgrad), 1 = wgrad.  One table per kind so that the picks
// can be exported / imported as a whole (sy11_tune_export / sy11_tune_import: every rank of a data-parallel job runs the
// kernels rank 0 measured).
Cache& cache(int kind);

// run(cand) launches candidate `cand` on `st` and returns 0 on success.  Returns the fastest candidate, or -1 if
// nothing could be measured.
template <class F>
int pick(const int* cands, int ncand, F&& run, hipStream_t st, const char* what, const int* key, int nkey) {
  // one measurement at a time per process: the event pair is shared, and two threads timing candidates concurrently would also
  // time each other's kernels (the library's only other process-wide state is the option table and the pick tables, core.hip)
  static std::mutex mu;
  std::lock_guard<std::mutex> guard(mu);
  static hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!e0 && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) { (void)hipGetLastError(); return -1; }
  // candidates are timed with the rest of the GPU idle: the caller may be one of several streams (the engine launches filter
  // gradients on a second one), and kernels still draining elsewhere would be timed along with the first candidates.  Never
  // reached while `st` is being captured (the callers check), and measuring is a first-call event per problem key.
  (void)hipDeviceSynchronize();
  int best = -1;
  float best_ms = 0.f;
  for (int i = 0; i < ncand; ++i) {
    if (run(cands[i]) != 0) continue;                                   // warm-up (code object load, caches)
    if (hipEventRecord(e0, st) != hipSuccess) return -1;
    if (run(cands[i]) != 0 || run(cands[i]) != 0) continue;
    if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) { (void)hipGetLastError(); return -1; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); continue; }
    if (logging()) fprintf(stderr, "[sy11 tune] %s cand %d: %.1f us\n", what, cands[i], ms * 500.f);
    if (best < 0 || ms < best_ms) { best = cands[i]; best_ms = ms; }
  }
  if (logging() && best >= 0) {
    fprintf(stderr, "[sy11 tune] %s key", what);
    for (int i = 0; i < nkey; ++i) fprintf(stderr, " %d", key[i]);
    fprintf(stderr, " -> %d (%.1f us)\n", best, best_ms * 500.f);
  }
  return best;
}

}  // namespace sy11tune
