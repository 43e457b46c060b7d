// grid_exchange.h — the partial-sum exchange of the single-launch kernels, once.
//
// householder_fused_kernel, householder_dots_keep_kernel, qn_apply_fused_kernel and qn_apply_persist_kernel make their
// workgroups wait for each other inside one launch: every workgroup publishes partial sums, waits for those of all its
// peers and adds them up in a fixed order, so each one obtains the bit-identical totals. Included by common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

namespace mxlo {

constexpr unsigned long long kSlotEmpty = 0x7FF8DEADBEEF0001ull;   // a NaN payload no arithmetic produces (partials are canonicalised)

// ---- single-launch (grid-exchange) kernels: bounded wait + fault flag -----------------------------------------------
// The workgroups of householder_fused_kernel / qn_apply_fused_kernel wait for each other's partials, so the whole grid
// must be resident at once. The launch sites check that against the occupancy of the kernel (coresident()); what no
// host-side check can see — other processes occupying the CUs, CU masking, a launch killed half-way that left the
// slots inconsistent — is caught by the wait itself: a lane that has polled one slot for longer than
// `fused_timeout_ms` raises the ctx fault word (pinned host memory, system-scope store) and continues with a NaN, so
// the kernel ENDS with NaN results instead of hanging the GPU. The host looks at the word (a plain read of pinned
// memory, no synchronisation) before every single-launch apply and inside mxlo_ctx_sync: fused_fault_check() then
// re-arms the slots, switches the single-launch forms of the ctx off and returns MXLO_EHIP naming what happened.
constexpr unsigned kFaultHouseholder = 1u, kFaultQn = 2u, kFaultHermitian = 4u, kFaultKron = 8u;
constexpr unsigned long long kCanonicalNaN = 0x7FF8000000000000ull;

// Both slot sets empty, the eight epoch words behind them zero: `ptr` holds 2 * nslots + 8 words.
inline hipError_t exchange_slots_init(unsigned long long *ptr, size_t nslots) {
  std::vector<unsigned long long> init(2 * nslots + 8, kSlotEmpty);
  for (int i = 0; i < 8; ++i) init[2 * nslots + i] = 0;
  return hipMemcpy(ptr, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
}

#if defined(__HIPCC__)
__device__ __forceinline__ unsigned long long poll_slot(const unsigned long long *slot, unsigned long long ticks,
                                                        unsigned *fault, unsigned code) {
  unsigned long long bits, t0 = 0;
  unsigned it = 0;
  while ((bits = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kSlotEmpty) {
    __builtin_amdgcn_s_sleep(1);
    if ((++it & 255u) == 0) {                       // the clock is read once per 256 polls (each poll is a memory round trip)
      const unsigned long long now = (unsigned long long)wall_clock64();
      if (t0 == 0) t0 = now;
      else if (now - t0 > ticks) {
        __hip_atomic_store(fault, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return kCanonicalNaN;
      }
    }
  }
  return bits;
}

// The bits of a partial as a slot holds them: any NaN becomes the canonical one, never the empty marker.
__device__ __forceinline__ unsigned long long slot_bits(double v) {
  return v != v ? kCanonicalNaN : (unsigned long long)__double_as_longlong(v);
}

// The exchange. `slots` is [2][nslots] words and the epoch word behind them (exchange_slots_init).
//  - No fence. A partial is ONE self-contained 64-bit agent-scope store and readers poll with agent-scope loads: the
//    value is its own "ready" flag, so nothing has to be ordered against it (an agent-scope release fence would write
//    back the whole L2 of every XCD: profiles/r01_sweep_fuse.txt).
//  - An empty slot is kSlotEmpty, a NaN payload. Arithmetic produces NaNs of other payloads at most, and publish()
//    stores slot_bits(): every NaN partial is the canonical NaN. A reader can never take a partial for "empty".
//  - Two slot sets alternate by the epoch word, which lives in device memory and not in a kernel argument, so a captured
//    graph replays correctly: a launch uses set e and re-arms set 1 - e, the one its successor will use. It never
//    re-arms its own set, which its slower workgroups are still reading.
//  - One launch per ctx and slot set is in flight at a time: all work of a ctx is stream-ordered (mxlo_ctx_set_stream),
//    and kernels that share a slot set share its epoch word. Two launches overlapping on one set would read each
//    other's partials.
//  - finish() may flip the epoch as soon as workgroup 0 has seen every partial: a workgroup publishes after begin(), so
//    by then every workgroup has read e. The re-armed set is complete by the end of the launch, before the successor starts.
//  - Every wait is bounded (poll_slot above).
struct GridExchange {
  unsigned long long *mine, *epoch;
  unsigned e;
  // BLOCK: threads per workgroup. Every thread of the grid calls it.
  template <int BLOCK>
  __device__ __forceinline__ void begin(unsigned long long *slots, int nslots) {
    epoch = slots + 2 * nslots;
    e = (unsigned)__hip_atomic_load(epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u;
    e = __builtin_amdgcn_readfirstlane(e);   // one value per grid: it lives in a scalar register to the end of the kernel
    mine = slots + e * nslots;
    unsigned long long *other = slots + (1u - e) * nslots;
    for (int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x; i < nslots; i += (int)gridDim.x * BLOCK)
      __hip_atomic_store(other + i, kSlotEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // `dropped`: the test hook fused_debug_drop — this workgroup's partial never arrives
  __device__ __forceinline__ void publish(int index, double value, bool dropped) const {
    if (!dropped) __hip_atomic_store(mine + index, slot_bits(value), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // one look at a slot without waiting: kSlotEmpty, or the partial's bits
  __device__ __forceinline__ unsigned long long peek(int index) const {
    return __hip_atomic_load(mine + index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ double wait(int index, unsigned long long ticks, unsigned *fault, unsigned code) const {
    return __longlong_as_double((long long)poll_slot(mine + index, ticks, fault, code));
  }
  // only after this workgroup has seen every partial
  __device__ __forceinline__ void finish() const {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      __hip_atomic_store(epoch, (unsigned long long)(1u - e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
#endif

}  // namespace mxlo
