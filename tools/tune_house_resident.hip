// Would the HEADLINE (opHouseholder mul!, n = 1e8 fp64: a dot launch + an update launch, every stream nontemporal) gain from
// keeping a fixed SLICE of h — the operator's own vector, the same bytes in every apply, read twice per apply — in the 256 MiB
// Infinity Cache from one apply to the next? The slice is loaded with the default policy, everything else stays nontemporal.
//   hipcc -O3 --offload-arch=gfx950 tools/tune_house_resident.hip -o tools/tune_house_resident && tools/tune_house_resident
//   (tools/tune_house_resident pmc: part 1a only, every step launched once, for a counters-only rocprofv3 --pmc run)
// 1a survival: a contiguous slice of S MiB is loaded with the default policy, then nothing / 1.6 GB of nontemporal loads /
//    0.8 GB of nontemporal stores / both run, then the slice is read again and that read is timed (cold: after 1.6 GB of
//    default-policy loads).
// 1b the dot launch's shape (num_cu workgroups x 256 lanes, 4 vectors per stream and round, nontemporal) with q of every 16
//    chunks of h on the default policy, chosen diagonally in (round, workgroup) as csrc/house_keep_plan.h does; warm (the
//    apply loop) and cold (slice evicted before).
// 1c the update launch's shape (one 1024-vector chunk per workgroup, back to front, 2 reads + 1 nontemporal write), same rule,
//    measured directly behind 1b in a loop of applies.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef double f64x2 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
constexpr int B = 256, U = 4;
constexpr int64_t CHUNK = (int64_t)B * U;

__device__ __forceinline__ bool resident(int t, int q) { return (t * q) % 16 >= 16 - q; }   // = house_resident_diag
// The nontemporal hint is metadata: the compiler merges the otherwise identical loads of the two sides of a policy choice
// and drops it (the first version of this harness measured default-policy h loads at EVERY q). A differing side-effecting
// marker in front of and behind the loads keeps the sides apart; it emits no instruction.
#define SIDE(tag) asm volatile("; h loads: " tag ::: "memory")

// persistent read of vectors [0, nvec): POLICY 0 default, 1 nontemporal; the sum goes to sink[workgroup]
template <int POLICY>
__global__ void __launch_bounds__(B) read_kernel(const f64x2 *__restrict__ p, int64_t nvec, double *__restrict__ sink) {
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x; base < nvec; base += (int64_t)gridDim.x * CHUNK) {
    f64x2 a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * B;
      a[u] = i < nvec ? (POLICY ? __builtin_nontemporal_load(p + i) : p[i]) : f64x2{0, 0};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc += a[u][0] + a[u][1];
  }
  if (acc == 12345.678) sink[blockIdx.x] = acc;   // never true for the zero-filled buffers; keeps the loads
}
__global__ void __launch_bounds__(B) nt_store_kernel(f64x2 *__restrict__ p, int64_t nvec) {
  for (int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x; base < nvec; base += (int64_t)gridDim.x * CHUNK)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * B;
      if (i < nvec) __builtin_nontemporal_store(f64x2{0, 0}, p + i);
    }
}

// 1b: whole rounds of G chunks, then at most one (possibly partial) chunk per workgroup
__global__ void __launch_bounds__(B) dots_kernel(const f64x2 *__restrict__ h, const f64x2 *__restrict__ v, int64_t nvec, int q,
                                                 double *__restrict__ part) {
  const int tid = threadIdx.x, G = gridDim.x, b = blockIdx.x;
  const int64_t rounds = nvec / CHUNK / G;
  double acc = 0.0;
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t base = (r * G + b) * CHUNK + tid;
    f64x2 a[U], x[U];
    if (resident((int)((r + b) & 15), q)) {
      SIDE("resident");
#pragma unroll
      for (int u = 0; u < U; ++u) { x[u] = __builtin_nontemporal_load(v + base + u * B); a[u] = h[base + u * B]; }
      SIDE("resident, issued");
    } else {
      SIDE("streamed");
#pragma unroll
      for (int u = 0; u < U; ++u) { x[u] = __builtin_nontemporal_load(v + base + u * B); a[u] = __builtin_nontemporal_load(h + base + u * B); }
      SIDE("streamed, issued");
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = fma(a[u][0], x[u][0], fma(a[u][1], x[u][1], acc));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = (rounds * G + b) * CHUNK + tid + (int64_t)u * B;
    if (i < nvec) {
      const f64x2 x = __builtin_nontemporal_load(v + i), a = __builtin_nontemporal_load(h + i);
      acc = fma(a[0], x[0], fma(a[1], x[1], acc));
    }
  }
  __shared__ double red[B / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) part[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// 1c: grid = number of chunks, back to front; G = the dot launch's grid (the rule's rounds and workgroups)
__global__ void __launch_bounds__(B) update_kernel(f64x2 *__restrict__ r, const f64x2 *__restrict__ h, const f64x2 *__restrict__ v, int64_t nvec,
                                                   int G, int q, const double *__restrict__ part) {
  const double c = 2.0 * part[0];
  const int64_t nch = (nvec + CHUNK - 1) / CHUNK, ch = nch - 1 - blockIdx.x, base = ch * CHUNK + threadIdx.x;
  f64x2 a[U], x[U];
  if (base + (int64_t)(U - 1) * B < nvec) {
    if (resident((int)((ch / G + ch % G) & 15), q)) {
      SIDE("resident");
#pragma unroll
      for (int u = 0; u < U; ++u) { a[u] = h[base + u * B]; x[u] = __builtin_nontemporal_load(v + base + u * B); }
      SIDE("resident, issued");
    } else {
      SIDE("streamed");
#pragma unroll
      for (int u = 0; u < U; ++u) { a[u] = __builtin_nontemporal_load(h + base + u * B); x[u] = __builtin_nontemporal_load(v + base + u * B); }
      SIDE("streamed, issued");
    }
#pragma unroll
    for (int u = 0; u < U; ++u) __builtin_nontemporal_store(f64x2{x[u][0] - c * a[u][0], x[u][1] - c * a[u][1]}, r + base + u * B);
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * B;
      if (i < nvec) {
        const f64x2 aa = __builtin_nontemporal_load(h + i), xx = __builtin_nontemporal_load(v + i);
        __builtin_nontemporal_store(f64x2{xx[0] - c * aa[0], xx[1] - c * aa[1]}, r + i);
      }
    }
  }
}

static double median(std::vector<double> t) {
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

int main(int argc, char **argv) {
  const bool pmc = argc > 1 && !strcmp(argv[1], "pmc");
  hipDeviceProp_t pr;
  CK(hipGetDeviceProperties(&pr, 0));
  const int cus = pr.multiProcessorCount;
  const int64_t ne = 100000000, nv = ne / 2;
  double *h, *v, *r, *part;
  CK(hipMalloc(&h, 8 * ne)); CK(hipMalloc(&v, 8 * ne)); CK(hipMalloc(&r, 8 * ne)); CK(hipMalloc(&part, 8 * 4096));
  CK(hipMemset(h, 0, 8 * ne)); CK(hipMemset(v, 0, 8 * ne)); CK(hipMemset(r, 0, 8 * ne)); CK(hipMemset(part, 0, 8 * 4096));
  hipEvent_t e0, e1, e2;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); CK(hipEventCreate(&e2));
  auto us_between = [&](hipEvent_t a, hipEvent_t b) { float ms; CK(hipEventElapsedTime(&ms, a, b)); return (double)ms * 1e3; };
  const f64x2 *H = (const f64x2 *)h, *V = (const f64x2 *)v;
  f64x2 *R = (f64x2 *)r;
  const int rg = cus * 4;   // persistent read / store grid
  printf("device %s, %d CUs, n = %lld f64 per buffer\n", pr.gcnArchName, cus, (long long)ne);

  // ---- 1a
  const char *between_name[5] = {"nothing", "1.6 GB nontemporal loads", "0.8 GB nontemporal stores", "both", "1.6 GB default loads (cold)"};
  printf("1a: re-read of a default-policy slice of h after ... (us, TB/s of the slice; median of %d)\n", pmc ? 1 : 7);
  for (int S : {64, 128, 192, 224}) {
    const int64_t sv = (int64_t)S * (1 << 20) / 16;
    for (int bt = 0; bt < 5; ++bt) {
      std::vector<double> t;
      for (int rep = 0; rep < (pmc ? 1 : 7); ++rep) {
        hipLaunchKernelGGL(read_kernel<0>, dim3(rg), dim3(B), 0, 0, H, sv, part);
        if (bt == 1 || bt == 3) {
          hipLaunchKernelGGL(read_kernel<1>, dim3(rg), dim3(B), 0, 0, V, nv, part);
          hipLaunchKernelGGL(read_kernel<1>, dim3(rg), dim3(B), 0, 0, (const f64x2 *)R, nv, part);
        }
        if (bt == 2 || bt == 3) hipLaunchKernelGGL(nt_store_kernel, dim3(rg), dim3(B), 0, 0, R, nv);
        if (bt == 4) {
          hipLaunchKernelGGL(read_kernel<0>, dim3(rg), dim3(B), 0, 0, V, nv, part);
          hipLaunchKernelGGL(read_kernel<0>, dim3(rg), dim3(B), 0, 0, (const f64x2 *)R, nv, part);
        }
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(read_kernel<0>, dim3(rg), dim3(B), 0, 0, H, sv, part);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        t.push_back(us_between(e0, e1));
      }
      const double m = median(t);
      printf("  S = %3d MiB  between: %-28s %8.1f us  %5.2f TB/s\n", S, between_name[bt], m, (double)sv * 16 / m / 1e6);
    }
  }
  if (pmc) return 0;

  // ---- 1b + 1c: a loop of applies (dot launch, update launch); cold: the slice evicted before the dot launch
  const int gu = (int)((nv + CHUNK - 1) / CHUNK);
  printf("1b / 1c: dot launch (%d workgroups) and update launch (%d workgroups) of one apply; median of 15 applies, us\n", cus, gu);
  printf("   q  slice MB |  warm: dots  update    sum | cold: dots  update    sum\n");
  for (int round = 0; round < 2; ++round)
    for (int q : {0, 1, 2, 3, 4, 5, 8, 16}) {
      double res[2][3];
      for (int cold = 0; cold < 2; ++cold) {
        std::vector<double> td, tu;
        for (int rep = 0; rep < 18; ++rep) {
          if (cold) hipLaunchKernelGGL(read_kernel<0>, dim3(rg), dim3(B), 0, 0, (const f64x2 *)R, nv, part);   // 0.8 GB default loads
          CK(hipEventRecord(e0));
          hipLaunchKernelGGL(dots_kernel, dim3(cus), dim3(B), 0, 0, H, V, nv, q, part);
          CK(hipEventRecord(e1));
          hipLaunchKernelGGL(update_kernel, dim3(gu), dim3(B), 0, 0, R, H, V, nv, cus, q, (const double *)part);
          CK(hipEventRecord(e2));
          CK(hipEventSynchronize(e2));
          CK(hipGetLastError());
          if (rep >= 3) { td.push_back(us_between(e0, e1)); tu.push_back(us_between(e1, e2)); }
        }
        res[cold][0] = median(td); res[cold][1] = median(tu); res[cold][2] = res[cold][0] + res[cold][1];
      }
      printf("  %2d  %7.0f  |      %7.1f %7.1f %7.1f |     %7.1f %7.1f %7.1f\n", q, q / 16.0 * 8e-6 * ne, res[0][0], res[0][1], res[0][2],
             res[1][0], res[1][1], res[1][2]);
    }
  CK(hipDeviceSynchronize());
  return 0;
}
