// Issue-rate and semantics probe for the packed 16-bit min/max pairs (not
// part of the library): can the median's selection network run on
// v_pk_min_f16 / v_pk_max_f16 over raw bf16 words instead of v_pk_min_u16 /
// v_pk_max_u16 over transformed keys?
//   1. register-only loops, u16 pair against f16 pair:
//      dep  : one chain, every op reads the previous op's result;
//      ce16 : compare-exchanges over 16 registers (the network's pattern:
//             min and max of the same two registers, 8 independent sites
//             per layer);
//   2. what the f16 pair returns for +0 / -0 in either order and for
//      f16-subnormal patterns (the kernel descriptor keeps f16 denormals).
// Build: hipcc --offload-arch=gfx950 -O3 pkminprobe.hip -o pkminprobe
#include <hip/hip_runtime.h>
#include <cstdio>

#define CK(x) do { auto e = (x); if (e) { printf("ERR %d @%d\n", e, __LINE__); return 1; } } while (0)

typedef unsigned int u32;

struct U16 {
  static __device__ __forceinline__ u32 mn(u32 a, u32 b) {
    u32 r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
  static __device__ __forceinline__ u32 mx(u32 a, u32 b) {
    u32 r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
};
struct F16 {
  static __device__ __forceinline__ u32 mn(u32 a, u32 b) {
    u32 r;
    asm("v_pk_min_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
  static __device__ __forceinline__ u32 mx(u32 a, u32 b) {
    u32 r;
    asm("v_pk_max_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
};

constexpr int ITERS = 4096;

// 64 dependent ops per iteration
template <typename OP>
__global__ void __launch_bounds__(256) dep_kernel(const u32* in, u32* out) {
  u32 x = in[threadIdx.x];
  const u32 c0 = in[256 + threadIdx.x], c1 = in[512 + threadIdx.x];
  for (int it = 0; it < ITERS; ++it) {
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      x = OP::mn(x, c0);
      x = OP::mx(x, c1);
    }
  }
  out[blockIdx.x * 256 + threadIdx.x] = x;
}

// 4 layers of 8 compare-exchanges over 16 registers per iteration: 64 ops
template <typename OP>
__global__ void __launch_bounds__(256) ce16_kernel(const u32* in, u32* out) {
  u32 v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = in[(i * 256 + threadIdx.x) & 1023];
  for (int it = 0; it < ITERS; ++it) {
#pragma unroll
    for (int j = 8; j >= 1; j >>= 1)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((i ^ j) > i) {
          const u32 a = v[i], b = v[i ^ j];
          // alternate the direction so that the data never settle
          v[i] = (j & 5) ? OP::mn(a, b) : OP::mx(a, b);
          v[i ^ j] = (j & 5) ? OP::mx(a, b) : OP::mn(a, b);
        }
  }
  u32 acc = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc ^= v[i];
  out[blockIdx.x * 256 + threadIdx.x] = acc;
}

template <typename OP>
__global__ void sem_kernel(const u32* a, const u32* b, u32* mn, u32* mx, int n) {
  const int i = threadIdx.x;
  if (i < n) {
    mn[i] = OP::mn(a[i], b[i]);
    mx[i] = OP::mx(a[i], b[i]);
  }
}

int main() {
  const int blocks = 256 * 8;  // 8 blocks of 4 waves per CU: 8 waves per SIMD
  u32 *in, *out;
  CK(hipMalloc(&in, 1024 * 4));
  CK(hipMalloc(&out, (size_t)blocks * 256 * 4));
  u32 h[1024];
  // legal f16-finite patterns, both signs, so that both pairs see the same
  // kind of data
  for (int i = 0; i < 1024; ++i) {
    const u32 lo = (u32)(i * 2654435761u >> 17) % 0x7C00u;
    const u32 hi = (u32)(i * 40503u + 77u) % 0x7C00u;
    h[i] = (lo | ((i & 1) << 15)) | ((hi | ((i & 2) << 14)) << 16);
  }
  CK(hipMemcpy(in, h, sizeof(h), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  float res[4] = {0, 0, 0, 0};
  int slot = 0;
  auto bench = [&](const char* name, auto kern) {
    float best = 1e30f;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, in, out);
    CK(hipDeviceSynchronize());
    for (int r = 0; r < 5; ++r) {
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, in, out);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (ms < best) best = ms;
    }
    // wave-ops issued: blocks * 4 waves * ITERS * 64
    const double wops = (double)blocks * 4 * ITERS * 64;
    printf("%-28s %8.3f ms  %7.2f G wave-ops/s\n", name, best,
           wops / best / 1e6);
    res[slot++] = best;
    return 0;
  };
  if (bench("dep  v_pk_min/max_u16", dep_kernel<U16>)) return 1;
  if (bench("dep  v_pk_min/max_f16", dep_kernel<F16>)) return 1;
  if (bench("ce16 v_pk_min/max_u16", ce16_kernel<U16>)) return 1;
  if (bench("ce16 v_pk_min/max_f16", ce16_kernel<F16>)) return 1;
  printf("f16 / u16 time: dep %.3f  ce16 %.3f\n", res[1] / res[0],
         res[3] / res[2]);

  // semantics: {a, b} per 16-bit half
  const u32 pa[] = {0x00008000u, 0x80000000u, 0x00010002u, 0x80018001u,
                    0x03FF0400u, 0x83FF8400u, 0x7BFFFBFFu, 0x00018000u,
                    0x3F80BF80u, 0x03FF83FFu};
  const u32 pb[] = {0x80000000u, 0x00008000u, 0x00020001u, 0x00010001u,
                    0x040003FFu, 0x840083FFu, 0xFBFF7BFFu, 0x80000001u,
                    0xBF803F80u, 0x83FF03FFu};
  const int np = sizeof(pa) / sizeof(pa[0]);
  u32 *da, *db, *dmn, *dmx;
  CK(hipMalloc(&da, sizeof(pa)));
  CK(hipMalloc(&db, sizeof(pa)));
  CK(hipMalloc(&dmn, sizeof(pa)));
  CK(hipMalloc(&dmx, sizeof(pa)));
  CK(hipMemcpy(da, pa, sizeof(pa), hipMemcpyHostToDevice));
  CK(hipMemcpy(db, pb, sizeof(pa), hipMemcpyHostToDevice));
  u32 hmn[np], hmx[np];
  hipLaunchKernelGGL(sem_kernel<F16>, dim3(1), dim3(64), 0, 0, da, db, dmn, dmx,
                     np);
  CK(hipMemcpy(hmn, dmn, sizeof(pa), hipMemcpyDeviceToHost));
  CK(hipMemcpy(hmx, dmx, sizeof(pa), hipMemcpyDeviceToHost));
  bool multiset = true;
  for (int i = 0; i < np; ++i) {
    printf("f16 a=%08x b=%08x  min=%08x max=%08x\n", pa[i], pb[i], hmn[i],
           hmx[i]);
    for (int sh = 0; sh < 32; sh += 16) {
      const u32 a = (pa[i] >> sh) & 0xFFFFu, b = (pb[i] >> sh) & 0xFFFFu;
      const u32 lo = (hmn[i] >> sh) & 0xFFFFu, hi = (hmx[i] >> sh) & 0xFFFFu;
      if (!((lo == a && hi == b) || (lo == b && hi == a))) multiset = false;
    }
  }
  const bool zeros = hmn[0] == 0x80008000u && hmx[0] == 0x00000000u &&
                     hmn[1] == 0x80008000u && hmx[1] == 0x00000000u;
  printf("f16 pair returns {-0, +0} for (+0, -0) in either order: %s\n",
         zeros ? "yes" : "NO");
  printf("f16 pair returns its two inputs, bit for bit, every time: %s\n",
         multiset ? "yes" : "NO");
  return 0;
}
