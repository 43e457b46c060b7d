// common.h — internal definitions shared by the libmxlo.so translation units.
// gfx950 (MI355X, CDNA4) only: wave = 64 lanes, 256 CUs in 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mxlo.h"

#define MXLO_API extern "C" __attribute__((visibility("default")))

namespace mxlo {

constexpr int kBlock = 256;          // 4 waves of 64 lanes: one wave per SIMD of a CU
constexpr int kWave = 64;
constexpr int kMaxRedCols = 128;     // columns a single reduction call may produce
constexpr int kQnfMaxCols = 40, kQnfMaxGrid = 256;   // single-launch quasi-Newton apply: panel columns x workgroups of its exchange
constexpr int kQnfSlots = kQnfMaxCols * kQnfMaxGrid;
constexpr int kFusedSlots = 512;     // workgroups of a single-launch (grid-exchange) kernel: all co-resident (round 6: up to two per CU)
constexpr int kMaxRedBlocks = 4096;  // partial slots per column in the workspace
constexpr int kScalarSlots = 8192;   // doubles in the device scalar buffer

void set_error(const char *fmt, ...);

// ---- runtime-call accounting (the f2 contract: a warmed mul!/diag!/solve allocates nothing, copies nothing, never
// synchronises) -----------------------------------------------------------------------------------------------
// Every HIP runtime entry point the library uses that allocates, copies or blocks goes through these macros (a
// function-like macro is not re-expanded inside its own replacement, so the inner name is the real HIP function);
// kernel launches are counted in MXLO_LAUNCH_CHECK. mxlo_debug_counters() exports the totals for the contract test.
struct ApiCounters {
  std::atomic<int64_t> n_malloc{0}, n_free{0}, n_h2d{0}, n_d2h{0}, n_d2d{0}, n_d2h_bytes{0}, n_stream_sync{0},
      n_device_sync{0}, n_event_sync{0}, n_memset_async{0}, n_launch{0}, n_blocking_copy{0};
};
inline ApiCounters &api_counters() {   // one instance per linked image (the library's is what mxlo_debug_counters reports)
  static ApiCounters c;
  return c;
}
inline void count_copy(size_t bytes, hipMemcpyKind kind, bool blocking) {
  ApiCounters &c = api_counters();
  if (kind == hipMemcpyDeviceToHost) { ++c.n_d2h; c.n_d2h_bytes += (int64_t)bytes; }
  else if (kind == hipMemcpyHostToDevice) ++c.n_h2d;
  else ++c.n_d2d;
  if (blocking) ++c.n_blocking_copy;
}
inline hipError_t counted_memcpy(void *d, const void *s, size_t b, hipMemcpyKind k) {
  count_copy(b, k, true);
  return hipMemcpy(d, s, b, k);
}
inline hipError_t counted_memcpy_async(void *d, const void *s, size_t b, hipMemcpyKind k, hipStream_t st) {
  count_copy(b, k, false);
  return hipMemcpyAsync(d, s, b, k, st);
}
#define hipMalloc(...) (++mxlo::api_counters().n_malloc, hipMalloc(__VA_ARGS__))
#define hipFree(...) (++mxlo::api_counters().n_free, hipFree(__VA_ARGS__))
#define hipHostMalloc(...) (++mxlo::api_counters().n_malloc, hipHostMalloc(__VA_ARGS__))
#define hipHostFree(...) (++mxlo::api_counters().n_free, hipHostFree(__VA_ARGS__))
#define hipMemcpy(...) mxlo::counted_memcpy(__VA_ARGS__)
#define hipMemcpyAsync(...) mxlo::counted_memcpy_async(__VA_ARGS__)
#define hipStreamSynchronize(...) (++mxlo::api_counters().n_stream_sync, hipStreamSynchronize(__VA_ARGS__))
#define hipDeviceSynchronize(...) (++mxlo::api_counters().n_device_sync, hipDeviceSynchronize(__VA_ARGS__))
#define hipEventSynchronize(...) (++mxlo::api_counters().n_event_sync, hipEventSynchronize(__VA_ARGS__))
#define hipMemsetAsync(...) (++mxlo::api_counters().n_memset_async, hipMemsetAsync(__VA_ARGS__))

#define MXLO_HIP(call)                                                                           \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      mxlo::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      return MXLO_EHIP;                                                                          \
    }                                                                                            \
  } while (0)

#define MXLO_REQUIRE(cond, code, ...)                                                            \
  do {                                                                                           \
    if (!(cond)) {                                                                               \
      mxlo::set_error(__VA_ARGS__);                                                              \
      return (code);                                                                             \
    }                                                                                            \
  } while (0)

#define MXLO_TRY(expr)                                                                           \
  do {                                                                                           \
    int32_t s__ = (expr);                                                                        \
    if (s__ != MXLO_OK) return s__;                                                              \
  } while (0)

// MXLO_TRACE=1 in the environment: synchronise after every launch and log its source line (a GPU memory fault
// aborts the process without an error code; the last line logged is the launch that faulted).
inline bool mxlo_trace_on() {
  static const bool on = getenv("MXLO_TRACE") != nullptr;
  return on;
}
#define MXLO_LAUNCH_CHECK()                                                                      \
  do {                                                                                           \
    ++mxlo::api_counters().n_launch;                                                             \
    if (mxlo_trace_on()) {                                                                       \
      fprintf(stderr, "[mxlo] launched %s:%d ... ", __FILE__, __LINE__);                         \
      fflush(stderr);                                                                            \
      (void)hipDeviceSynchronize();                                                              \
      fprintf(stderr, "done\n");                                                                 \
    }                                                                                            \
    hipError_t e__ = hipGetLastError();                                                          \
    if (e__ != hipSuccess) {                                                                     \
      mxlo::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__,      \
                      __LINE__);                                                                 \
      return MXLO_EHIP;                                                                          \
    }                                                                                            \
  } while (0)

struct Tune {   // the members, their defaults and why the defaults are what they are: tune_keys.def
#define MXLO_TUNE_KEY(type, name, def, lo, hi, rule, doc) type name = def;
#include "tune_keys.def"
};

}  // namespace mxlo

struct mxlo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cu = 256;
  double *partials = nullptr;  // [kMaxRedCols][kMaxRedBlocks] per-block partial sums
  double *scalars = nullptr;   // finalized reduction results / device-resident coefficients
  bool lds_attr_set = false;   // dynamic-LDS limits of the shifted-solve kernels raised on THIS device
  bool inv_lds_attr_set = false;   // ... and inv_coef_kernel at na = 64
  unsigned *ticket = nullptr;  // arrival counter of the fused (last-workgroup) finalize; zero between launches
  unsigned long long *xslots = nullptr;  // [2][kFusedSlots] partial-exchange slots + epoch word of the single-launch Householder
  unsigned long long *qslots = nullptr;  // [2][40 x 64] exchange slots + epoch word of the single-launch quasi-Newton apply (qn.hip)
  unsigned *fault_host = nullptr;        // pinned, device-mapped word: a single-launch kernel that timed out on its exchange
  unsigned *fault_dev = nullptr;         // stores its code here (system scope); the host reads it without synchronising
  int wall_clock_khz = 100000;           // rate of wall_clock64() on this device (hipDeviceAttributeWallClockRate)
  mxlo_allreduce_fn allreduce = nullptr;
  void *allreduce_user = nullptr;
  double *herm_slots = nullptr;   // self-validating partial slots of the single-launch opHermitian (all empty between applies)
  size_t herm_slots_bytes = 0;
  int64_t herm_slots_layout = 0;  // (n, strip shape) the slots were last used with
  bool herm_slots_dirty = false;  // a timed-out apply left slots filled: re-arm before the next use
  unsigned *kron_cnt = nullptr;   // counters of the XCD-local kron fusion (gemm_glds.h: kron_fused_kernel), zero between applies
  int kron_cnt_n = 0;
  int xcd_map = 0;                // 0: not probed; 1: workgroup id % 8 == XCC_ID on this device (probed once); -1: it is not
  void *scratch = nullptr;     // grow-on-demand workspace (opHermitian tile partials); owned by the ctx
  size_t scratch_bytes = 0;
  hipStream_t own_stream = nullptr;  // created by mxlo_ctx_create_stream, destroyed with the ctx
  hipEvent_t switch_event = nullptr; // orders the ctx workspaces across mxlo_ctx_set_stream
  bool capturing = false;      // between mxlo_graph_begin and mxlo_graph_end
  std::vector<std::pair<mxlo_qn *, int64_t>> captured_qn;   // quasi-Newton handles (and their generation) applied inside the open capture
  int64_t scratch_generation = 0;   // bumped whenever `scratch` is reallocated (captured opHermitian applies go stale)
  bool scratch_used_in_capture = false;
  void *stage = nullptr;       // copy of a v that overlaps res (stage_alias); grow-on-demand, owned by the ctx
  size_t stage_bytes = 0;
  mxlo::Tune tune;
};

#include "grid_exchange.h"   // (behind the counting macros above: its host call is a counted hipMemcpy)

namespace mxlo {

// Every entry point that allocates or launches runs on the device its ctx was created for, whatever the calling
// thread's current device is (one process driving several GPUs), and leaves the caller's current device untouched.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define MXLO_DEVICE_GUARD(ctxexpr) mxlo::DeviceGuard dev_guard__((ctxexpr)->device)

// ---- res aliasing v: mul!(x, op, x), or two overlapping windows of one buffer -------------------------------------------
// The reference defines these calls for the operators whose closures read (or copy) all of v before they write res.
// Our kernels take both pointers __restrict__, so the entry points decide: `same_ok` entry points (every element of res
// written by the lane that read the same element of v, after it read it) accept res == v as it is; any other overlap is
// STAGED — v is copied into the ctx's staging buffer with one D2D copy on the ctx stream (a memcpy node inside a graph
// capture) and the kernels read the copy, placed at v's own address modulo 256 so every alignment-dependent path (and
// its bits) is the one the unstaged call takes. A staging buffer that would have to grow inside a capture is MXLO_ESTATE,
// before anything is enqueued. Calls whose operands do not overlap pay one comparison.
inline bool bytes_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return na > 0 && nb > 0 && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}
int32_t stage_alias(mxlo_ctx *ctx, const void *res, int64_t res_bytes, const void **v, int64_t v_bytes, bool same_ok,
                    const char *what);   // api_ctx.hip

// ---- ctx->scratch: the grow-on-demand workspace of the dense leaves (tile / chunk partials) --------------------------------
// At least `need` bytes behind ctx->scratch; `what` names the user in the out-of-memory message ("<what> scratch: ...").
inline int32_t ensure_scratch(mxlo_ctx *ctx, size_t need, const char *what) {
  if (ctx->scratch_bytes < need) {            // stream-ordered users only: drain before the buffer is replaced
    if (ctx->scratch) {
      MXLO_HIP(hipStreamSynchronize(ctx->stream));
      MXLO_HIP(hipFree(ctx->scratch));
    }
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    hipError_t e = hipMalloc(&ctx->scratch, need);
    MXLO_REQUIRE(e == hipSuccess, MXLO_ENOMEM, "%s scratch: %s", what, hipGetErrorString(e));
    ctx->scratch_bytes = need;
    ++ctx->scratch_generation;     // graphs that recorded the old workspace pointer are stale now
  }
  if (ctx->capturing) ctx->scratch_used_in_capture = true;
  return MXLO_OK;
}

// ---- single-launch (grid-exchange) kernels: the exchange, its bounded wait and the fault codes are grid_exchange.h ------
int32_t fused_fault_check(mxlo_ctx *ctx);           // api_ctx.hip
inline unsigned long long fused_timeout_ticks(const mxlo_ctx *ctx) {   // wall_clock64() ticks: the device's constant-rate clock
  return (unsigned long long)ctx->tune.fused_timeout_ms * (unsigned long long)ctx->wall_clock_khz;
}
// true when `grid` workgroups of `kernel` (BLOCK threads, `lds_worst` bytes of dynamic LDS) fit on the device at once.
// Evaluated once per kernel instantiation and device (the occupancy query costs microseconds) — so `lds_worst` must be
// the LARGEST dynamic LDS size the kernel is ever launched with, not the size of the launch at hand: the cached answer
// then holds for every launch (a smaller request can only fit better).
template <auto Kernel, int BLOCK = kBlock>
inline bool coresident(mxlo_ctx *ctx, int64_t grid, size_t lds_worst = 0) {
  static std::atomic<int> cache[64];                // per kernel: blocks per CU + 1 by device ordinal, 0 = unknown
  const int d = ctx->device & 63;
  int per = cache[d].load(std::memory_order_relaxed);
  if (per == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, BLOCK, lds_worst) != hipSuccess) {
      (void)hipGetLastError();
      nb = 0;
    }
    per = nb + 1;
    cache[d].store(per, std::memory_order_relaxed);
  }
  return (int64_t)(per - 1) * ctx->num_cu >= grid;
}

// ---- 16-byte vector types --------------------------------------------------
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Complex element, laid out as Julia's Complex{R} / C's R _Complex: (re, im) adjacent.
template <typename R>
struct alignas(2 * sizeof(R)) cx {
  R re, im;
  __host__ __device__ constexpr cx(R r = R(0), R i = R(0)) : re(r), im(i) {}
};
template <typename T>
struct is_cx : std::false_type {};
template <typename R>
struct is_cx<cx<R>> : std::true_type {};
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <typename T>
struct Vec16;
template <>
struct Vec16<cx<double>> {   // one ComplexF64 per 16-byte access
  using type = f64x2;
  static constexpr int N = 1;
};
template <>
struct Vec16<cx<float>> {    // two ComplexF32
  using type = f32x4;
  static constexpr int N = 2;
};
template <>
struct Vec16<double> {
  using type = f64x2;
  static constexpr int N = 2;
};
template <>
struct Vec16<float> {
  using type = f32x4;
  static constexpr int N = 4;
};

// ---- wave-wide sum of a double, result in EVERY lane --------------------------------------------------------------
// The coefficient recurrences of the quasi-Newton operators (one wave, O(m) .. O(m^2) dependent reductions) spent their
// time in xor-shuffle trees: a 64-bit __shfl_xor is two ds_bpermute_b32 (~100+ cycles of latency each), six dependent
// levels per sum. DPP moves run on the VALU at register speed: quad_perm x2, row_shr:4, row_shr:8, then row_bcast:15 /
// row_bcast:31 (GFX9-family wave64 modes) leave the total in lane 63, which v_readlane broadcasts. Deterministic (one
// fixed tree), ~20x shorter than the shuffle tree. Masked-off / out-of-row sources read 0 (bound_ctrl).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_shift_or_zero(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, true);
  return __hiloint2double(hi, lo);
#else
  return v;   // host pass of the single-source compile: never executed
#endif
}
__device__ __forceinline__ double wave_allsum(double v) {
  v += dpp_shift_or_zero<0xb1, 0xf>(v);    // quad_perm [1,0,3,2]
  v += dpp_shift_or_zero<0x4e, 0xf>(v);    // quad_perm [2,3,0,1]: every lane holds its quad's sum
  v += dpp_shift_or_zero<0x114, 0xf>(v);   // row_shr:4
  v += dpp_shift_or_zero<0x118, 0xf>(v);   // row_shr:8: lanes 12..15 of a row hold the row's sum
  v += dpp_shift_or_zero<0x142, 0xa>(v);   // row_bcast:15 into rows 1, 3
  v += dpp_shift_or_zero<0x143, 0xc>(v);   // row_bcast:31 into rows 2, 3: lane 63 holds the wave's sum
#if defined(__HIP_DEVICE_COMPILE__)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63), hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
#else
  return v;
#endif
}

// Sum over the wave in LANE 0 (other lanes: unspecified), on the tree of the shuffle-down loop this replaces —
//   v[l] += v[l + 32]; v[l] += v[l + 16]; ... ; v[l] += v[l + 1]
// — so every reduction of the library keeps its bits. A 64-bit __shfl_down is two ds_bpermute_b32 with an LDS round trip
// each and six dependent levels per sum: the 2 NC + 4 sums at the end of a push pass cost 1.8 us (5 columns) to 5.5 us (20)
// at launch-bound sizes. Here the upper half arrives with v_permlane32_swap, the odd rows with v_permlane16_swap (gfx950),
// the rest with DPP row shifts: register-speed VALU work that independent sums overlap freely.
__device__ __forceinline__ double wave_sum(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto slo = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);   // [1]: lanes 0..31 hold lanes 32..63
    const auto shi = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    v += __hiloint2double((int)shi[1], (int)slo[1]);
  }
  {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto slo = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);   // [1]: rows 0, 2 hold rows 1, 3
    const auto shi = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v += __hiloint2double((int)shi[1], (int)slo[1]);
  }
  v += dpp_shift_or_zero<0x108, 0xf>(v);   // row_shl:8: lane l reads lane l + 8 of its row
  v += dpp_shift_or_zero<0x104, 0xf>(v);   // row_shl:4
  v += dpp_shift_or_zero<0x102, 0xf>(v);   // row_shl:2
  v += dpp_shift_or_zero<0x101, 0xf>(v);   // row_shl:1
#endif
  return v;
}
// Sum over a workgroup of kBlock lanes, in EVERY lane: wave_sum, then the four wave sums as (l0 + l1) + (l2 + l3)
// through `lds`. Two uses of one `lds` need a barrier between them.
__device__ __forceinline__ double block_sum4(double v, double (&lds)[kBlock / kWave]) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// ---- halving butterfly steps without LDS ---------------------------------------------------------------------------
// One step of a halving reduction over the lanes: every lane holds TWO partial sums x, y; lanes whose bit B is clear keep
// x and hand y to lane l ^ B, the others keep y and hand x over — afterwards each lane holds ONE sum over twice the lanes:
//   bit clear: x[l] + x[l ^ B]          bit set: y[l] + y[l ^ B]
// i.e. exactly  (bit ? y : x) + __shfl_xor(bit ? x : y, B)  (the adds are the same two operands: same bits), but a 64-bit
// __shfl_xor is two ds_bpermute_b32 round trips through LDS. B = 32 / 16 are ONE v_permlane32_swap / v_permlane16_swap per
// register half (gfx950: the swap IS the exchange — no select at all), B = 8 / 4 DPP row moves under bank masks.
__device__ __forceinline__ double halve_step32(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto l = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(y), false, false);
  const auto h = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(y), false, false);
  // [0]: lanes 0..31 x[l], lanes 32..63 y[l - 32];  [1]: lanes 0..31 x[l + 32], lanes 32..63 y[l]
  return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
#else
  return x + y;
#endif
}
__device__ __forceinline__ double halve_step16(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto l = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(y), false, false);
  const auto h = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(y), false, false);
  // [0]: even rows x[l], odd rows y[l - 16];  [1]: even rows x[l + 16], odd rows y[l]
  return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
#else
  return x + y;
#endif
}
// CTRL_UP: lane l reads lane l + B of its row (row_shl:B), CTRL_DN: lane l - B (row_shr:B); BANKS_CLR = the banks
// (4-lane groups of a row) whose lanes have bit B clear.
template <int CTRL_UP, int CTRL_DN, int BANKS_CLR>
__device__ __forceinline__ double halve_step_dpp(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BANKS_SET = 0xf & ~BANKS_CLR;
  int kl = __double2loint(x), kh = __double2hiint(x);       // keep: x where the bit is clear, y where it is set
  kl = __builtin_amdgcn_update_dpp(kl, __double2loint(y), 0xe4, 0xf, BANKS_SET, false);   // quad_perm [0,1,2,3]
  kh = __builtin_amdgcn_update_dpp(kh, __double2hiint(y), 0xe4, 0xf, BANKS_SET, false);
  int rl = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL_UP, 0xf, BANKS_CLR, false);   // x[l + B] into the clear lanes
  int rh = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL_UP, 0xf, BANKS_CLR, false);
  rl = __builtin_amdgcn_update_dpp(rl, __double2loint(y), CTRL_DN, 0xf, BANKS_SET, false);      // y[l - B] into the set lanes
  rh = __builtin_amdgcn_update_dpp(rh, __double2hiint(y), CTRL_DN, 0xf, BANKS_SET, false);
  return __hiloint2double(kh, kl) + __hiloint2double(rh, rl);
#else
  return x + y;
#endif
}
__device__ __forceinline__ double halve_step8(double x, double y) { return halve_step_dpp<0x108, 0x118, 0x3>(x, y); }
__device__ __forceinline__ double halve_step4(double x, double y) { return halve_step_dpp<0x104, 0x114, 0x5>(x, y); }
// v[l] + v[l ^ 2], v[l] + v[l ^ 1] in every lane (quad permutes)
__device__ __forceinline__ double pair_step2(double v) { return v + dpp_shift_or_zero<0x4e, 0xf>(v); }
__device__ __forceinline__ double pair_step1(double v) { return v + dpp_shift_or_zero<0xb1, 0xf>(v); }

// ---- alignment analysis for the vector path ---------------------------------
// All operands of an elementwise kernel can use 16-byte accesses iff they share
// the same address modulo 16; then `head` leading elements are peeled so the
// body starts 16-byte aligned. Returns -1 when the operands disagree.
template <typename T>
inline int64_t common_head(std::initializer_list<const void *> ptrs) {
  int64_t mis = -1;
  for (const void *p : ptrs) {
    if (!p) continue;
    int64_t m = (int64_t)((uintptr_t)p & 15u);
    if (m % (int64_t)sizeof(T)) return -1;
    if (mis < 0) mis = m;
    else if (mis != m) return -1;
  }
  if (mis <= 0) return 0;
  return (16 - mis) / (int64_t)sizeof(T);
}

inline int grid_for(const mxlo_ctx *ctx, int64_t work_items, int64_t items_per_block, int per_cu) {
  int64_t need = (work_items + items_per_block - 1) / items_per_block;
  int64_t g = need;
  if (per_cu > 0) {  // per_cu == 0: one work chunk per workgroup (no persistent loop)
    const int64_t cap = (int64_t)ctx->num_cu * per_cu;
    if (g > cap) g = cap;
  }
  if (g > 0x7fffffffLL) g = 0x7fffffffLL;
  return (int)(g < 1 ? 1 : g);
}

// qn.hip: current generation of a live quasi-Newton handle (false: the handle was destroyed)
bool qn_generation(const mxlo_qn *h, int64_t *gen);

// reductions.hip
int32_t finalize_and_reduce(mxlo_ctx *ctx, int ncols, int nblocks, double *out_dev);
// ... also posting the results (and extra_n earlier doubles) to mapped pinned host memory, reductions.hip
int32_t finalize_and_post(mxlo_ctx *ctx, int ncols, int nblocks, double *out_dev, double *post_dev, unsigned long long seq,
                          const double *extra_src, int extra_n);
int32_t allreduce_hook(mxlo_ctx *ctx, double *dev, int64_t count);
template <typename T>
int32_t panel_dots(mxlo_ctx *ctx, const T *const *cols_host, int ncols, const T *x, int64_t n,
                   double *out_dev);
// the dots pass alone: per-workgroup partials left in ctx->partials, *nblocks per column (<= 4 columns, n >= 1)
template <typename T>
int32_t panel_dots_partials(mxlo_ctx *ctx, const T *const *cols_host, int ncols, const T *x, int64_t n, int *nblocks);
// out1[c] = dot(cols[c], x1), out2[c] = dot(cols[c], x2) in one pass; all operands are aligned, padded panel columns
template <typename T>
int32_t panel_dots2(mxlo_ctx *ctx, const T *const *cols, int ncols, const T *x1, const T *x2, int64_t n_padded,
                    double *out1, double *out2);
// push! pass (reductions.hip): dual-x dots over <= 10 panel columns with the new pair in registers, optional in-pass
// stores into the slot being replaced; LOCAL sums (the caller runs the all-reduce hook)
// Extra jobs the pass's finalize launch can carry, so that a launch-bound push! needs no separate launches for them:
//   cp_*: cp_dst[i] = cp_src[i], i < cp_n (doubles; cp_src was written by an EARLIER kernel) — the inverse push!'s
//         S'y_new -> SY column copy;
//   post: x1·x2 and x2·x2 also go to mapped pinned host memory as (value, sequence number) pairs post[0..1], post[2..3]
//         — the decision scalars of an L-BFGS push!, which the host polls for (qn.hip: await_posted_pairs).
struct PushExtras {
  const double *cp_src = nullptr;
  double *cp_dst = nullptr;
  int cp_n = 0;
  double *post = nullptr;
  unsigned long long post_seq = 0;
};
template <typename T>
int32_t panel_push_pass(mxlo_ctx *ctx, const T *const *cols, int ncols, int slot, int slot_src, const T *x1,
                        const T *x2, int64_t n, int64_t n_padded, T *st1, T *st2, T *stb, double sq, double *out1,
                        double *out2, double *out_x1x2, double *out_x2x2, double *out_bb, double *out_x1x1 = nullptr,
                        const PushExtras *extras = nullptr);

}  // namespace mxlo
