// Attack-math kernels for gfx950.
//
// little_fused: the Little attack's mu + z * sigma per coordinate in ONE
// streaming pass (per-column sum / sum-of-squares, the reference's
// chunked Sigma-x / Sigma-x^2 decomposition little.py:219-224 fused into
// one kernel). Column-per-thread, adjacent lanes on adjacent columns.
//
// attack_stats: everything the Min-Max / Min-Sum attacks need from X —
// column mean, perturbation direction and 2n + 1 row statistics — in one
// pass of the same shape, the column held in registers (n <= 64).
//
// gaussian_fill: counter-based Philox4x32-10 + Box-Muller normal fill —
// the Gaussian attack stops consuming torch RNG on the hot path. The
// stream is deterministic per (seed, index) and independent of grid
// shape; it is a DIFFERENT sequence than torch's CPU generator (the
// seeded-CPU contract stays available through the functional path).
#include "common.h"
#include "launchers.h"
#include <type_traits>

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

// -- Little -----------------------------------------------------------------

template <typename T>
__global__ void little_kernel(const T* __restrict__ X, T* __restrict__ out,
                              int n, long d, float z) {
  const long col0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long col = col0; col < d; col += stride) {
    const T* xc = X + col;
    float s = 0.0f, s2 = 0.0f;
    int row = 0;
    for (; row + 3 < n; row += 4) {
      // 4 loads in flight per step
      const float v0 = to_f<T>(xc[(long)(row + 0) * d]);
      const float v1 = to_f<T>(xc[(long)(row + 1) * d]);
      const float v2 = to_f<T>(xc[(long)(row + 2) * d]);
      const float v3 = to_f<T>(xc[(long)(row + 3) * d]);
      s += v0 + v1 + v2 + v3;
      s2 += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
    }
    for (; row < n; ++row) {
      const float v = to_f<T>(xc[(long)row * d]);
      s += v;
      s2 += v * v;
    }
    const float mu = s / n;
    const float var = fmaxf(s2 / n - mu * mu, 0.0f);  // population variance
    out[col] = from_f<T>(mu + z * sqrtf(var));
  }
}

// -- Min-Max / Min-Sum statistics -------------------------------------------
//
// Both attacks send m = mu + gamma * p with the largest gamma that keeps m
// inside the honest cloud; since ||m - x_i||^2 = a_i + 2 gamma b_i +
// gamma^2 c, everything gamma needs from the (n, d) matrix is
//   mu_c, p_c          the column mean and the perturbation direction
//   a_i = ||mu - x_i||^2,  b_i = p . (mu - x_i),  c = ||p||^2
// attack_stats_reg_kernel produces all of it in one pass over X.

enum Perturb { PERT_UNIT = 0, PERT_STD = 1, PERT_SIGN = 2 };

// p_c from the column's mean and population variance. PERT_UNIT is -mu, not
// -mu / ||mu||: m does not change when p is rescaled, and the column-local
// form needs no global norm before the pass.
template <int PERT>
DEV float perturbation(float mu, float var) {
  if (PERT == PERT_UNIT) return -mu;
  if (PERT == PERT_STD) return -sqrtf(var);
  return mu > 0.0f ? -1.0f : (mu < 0.0f ? 1.0f : 0.0f);
}

constexpr int STATS_BLOCK = 256;
constexpr int STATS_WAVES = STATS_BLOCK / WAVE;

// n <= P, P in {8, 16, 32, 64}: the column stays in a register array, so mu
// and the deviations come from the same loaded values (variance as the mean
// squared deviation, no sum-of-squares cancellation), and the 2P row
// accumulators stay in registers across the grid-stride loop. Every index is
// compile-time (runtime-indexed register arrays spill). One LDS reduction
// and 2n + 1 atomic adds per block into the caller-zeroed
// stats = [a_0..a_{n-1}, b_0..b_{n-1}, c].
// At P = 64 the three 64-float arrays alone are 192 VGPRs: those
// instantiations ask for 2 waves/SIMD so the allocator may use 256 instead
// of spilling at 128 (it ends at 256; figures in
// benchmarks/RESULTS_MI355X_minmax.md).
template <int P, int PERT, typename T>
__global__ void __launch_bounds__(STATS_BLOCK, P >= 64 ? 2 : 4)
attack_stats_reg_kernel(const T* __restrict__ X, float* __restrict__ mu_out,
                        float* __restrict__ p_out, float* __restrict__ stats,
                        int n, long d) {
  __shared__ float red[STATS_WAVES][2 * P + 1];
  const long col0 = (long)blockIdx.x * STATS_BLOCK + threadIdx.x;
  const long stride = (long)gridDim.x * STATS_BLOCK;
  const float inv_n = 1.0f / (float)n;
  float a[P], b[P];
#pragma unroll
  for (int i = 0; i < P; ++i) a[i] = b[i] = 0.0f;
  float c = 0.0f;
  for (long col = col0; col < d; col += stride) {
    // raw loads with a pinned load/advance alternation, converted after:
    // see the load phase of colsel_reg_kernel. Slots past n repeat the last
    // row and are zeroed below. Both n and the row stride are made opaque
    // once per column (volatile asm: the compiler may neither hoist nor
    // merge them): left loop-invariant, the P pad masks and the P row
    // bases are hoisted into SGPR pairs, far more than there are, and come
    // back through v_writelane/readlane. n goes to a VGPR so the masks are
    // v_cmp/v_cndmask pairs (the vecify idiom of colsel.hip).
    int nv;
    asm volatile("v_mov_b32_e32 %0, %1" : "=v"(nv) : "s"(n));
    long step = d;
    asm volatile("" : "+s"(step));
    T raw[P];
    const T* q = X + col;
    if (n == P) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        raw[i] = *q;
        if (i + 1 < P) q += step;
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        raw[i] = *q;
        q += (i + 1 < nv) ? step : 0;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    float x[P];
#pragma unroll
    for (int i = 0; i < P; ++i) x[i] = to_f<T>(raw[i]);
    if (n < P) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i >= nv) x[i] = 0.0f;
    }
    // four partial sums: a single chain of P dependent adds would stall the
    // two waves per SIMD this kernel runs at
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < P; ++i) s[i & 3] += x[i];
    const float mu = ((s[0] + s[1]) + (s[2] + s[3])) * inv_n;
#pragma unroll
    for (int i = 0; i < P; ++i) x[i] = mu - x[i];  // x now holds mu - x_i
    if (n < P) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (i >= nv) x[i] = 0.0f;
    }
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < P; ++i) v[i & 3] = fmaf(x[i], x[i], v[i & 3]);
    const float var = ((v[0] + v[1]) + (v[2] + v[3])) * inv_n;
    const float p = perturbation<PERT>(mu, var);
    mu_out[col] = mu;
    p_out[col] = p;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      a[i] = fmaf(x[i], x[i], a[i]);
      b[i] = fmaf(p, x[i], b[i]);
    }
    c = fmaf(p, p, c);
  }
  // every thread gets here (threads past d with zero accumulators), so the
  // shuffles below see whole waves
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const float ra = wave_reduce_sum(a[i]);
    const float rb = wave_reduce_sum(b[i]);
    if (lane == 0) {
      red[wid][i] = ra;
      red[wid][P + i] = rb;
    }
  }
  const float rc = wave_reduce_sum(c);
  if (lane == 0) red[wid][2 * P] = rc;
  __syncthreads();
  const int t = threadIdx.x;
  if (t <= 2 * P) {
    float r = 0.0f;
#pragma unroll
    for (int w = 0; w < STATS_WAVES; ++w) r += red[w][t];
    // slot t of [a(P) | b(P) | c] -> slot of [a(n) | b(n) | c]
    const int row = t < P ? t : t - P;
    if (t == 2 * P)
      atomicAdd(&stats[2 * n], r);
    else if (row < n)
      atomicAdd(&stats[(t < P ? 0 : n) + row], r);
  }
}

// Any n: mu, p and c only, from per-column sum / sum of squares as in
// little_kernel. The rows' a and b then come from the rowops kernels (see
// launch_attack_stats).
template <int PERT, typename T>
__global__ void __launch_bounds__(STATS_BLOCK)
attack_moments_kernel(const T* __restrict__ X, float* __restrict__ mu_out,
                      float* __restrict__ p_out, float* __restrict__ c_out,
                      int n, long d) {
  __shared__ float red[STATS_WAVES];
  const long col0 = (long)blockIdx.x * STATS_BLOCK + threadIdx.x;
  const long stride = (long)gridDim.x * STATS_BLOCK;
  float c = 0.0f;
  for (long col = col0; col < d; col += stride) {
    const T* xc = X + col;
    float s = 0.0f, s2 = 0.0f;
    int row = 0;
    for (; row + 3 < n; row += 4) {
      const float v0 = to_f<T>(xc[(long)(row + 0) * d]);
      const float v1 = to_f<T>(xc[(long)(row + 1) * d]);
      const float v2 = to_f<T>(xc[(long)(row + 2) * d]);
      const float v3 = to_f<T>(xc[(long)(row + 3) * d]);
      s += v0 + v1 + v2 + v3;
      s2 += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
    }
    for (; row < n; ++row) {
      const float v = to_f<T>(xc[(long)row * d]);
      s += v;
      s2 += v * v;
    }
    const float mu = s / n;
    const float var = fmaxf(s2 / n - mu * mu, 0.0f);
    const float p = perturbation<PERT>(mu, var);
    mu_out[col] = mu;
    p_out[col] = p;
    c = fmaf(p, p, c);
  }
  c = block_reduce_sum(c, red, STATS_WAVES);
  if (threadIdx.x == 0) atomicAdd(c_out, c);
}

__global__ void negate_kernel(float* __restrict__ v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = -v[i];
}

// fn receives std::integral_constant<int, PERT>
template <typename F>
inline void by_perturb(int perturb, F&& fn) {
  if (perturb == PERT_UNIT) fn(std::integral_constant<int, PERT_UNIT>{});
  else if (perturb == PERT_STD) fn(std::integral_constant<int, PERT_STD>{});
  else fn(std::integral_constant<int, PERT_SIGN>{});
}

// -- Philox4x32-10 Gaussian fill --------------------------------------------

DEV u32 mulhi32(u32 a, u32 b) { return (u32)(((u64)a * b) >> 32); }

DEV void philox_round(u32& c0, u32& c1, u32& c2, u32& c3, u32 k0, u32 k1) {
  const u32 lo0 = 0xD2511F53u * c0;
  const u32 hi0 = mulhi32(0xD2511F53u, c0);
  const u32 lo1 = 0xCD9E8D57u * c2;
  const u32 hi1 = mulhi32(0xCD9E8D57u, c2);
  const u32 n0 = hi1 ^ c1 ^ k0;
  const u32 n1 = lo1;
  const u32 n2 = hi0 ^ c3 ^ k1;
  const u32 n3 = lo0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

DEV void philox10(u32 ctr_lo, u32 ctr_hi, u32 key_lo, u32 key_hi, u32& r0,
                  u32& r1, u32& r2, u32& r3) {
  u32 c0 = ctr_lo, c1 = ctr_hi, c2 = 0x2E7366CFu, c3 = 0x69C4C6E5u;
  u32 k0 = key_lo, k1 = key_hi;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r0 = c0; r1 = c1; r2 = c2; r3 = c3;
}

// two Box-Muller normals from two u32s
DEV void box_muller(u32 a, u32 b, float& n0, float& n1) {
  // (a + 1) in (0, 2^32]: avoids log(0)
  const float u1 = ((float)a + 1.0f) * 2.3283064e-10f;
  const float u2 = (float)b * 2.3283064e-10f;
  const float r = sqrtf(-2.0f * __logf(u1));
  const float th = 6.2831853f * u2;
  n0 = r * __cosf(th);
  n1 = r * __sinf(th);
}

template <typename T>
__global__ void gaussian_fill_kernel(T* __restrict__ out, long d, u32 seed_lo,
                                     u32 seed_hi, float mu, float sigma) {
  const long q0 = (long)blockIdx.x * blockDim.x + threadIdx.x;  // quad index
  const long nquads = (d + 3) >> 2;
  const long qstride = (long)gridDim.x * blockDim.x;
  for (long q = q0; q < nquads; q += qstride) {
    u32 r0, r1, r2, r3;
    philox10((u32)q, (u32)(q >> 32) ^ seed_hi, seed_lo, seed_hi, r0, r1, r2,
             r3);
    float n0, n1, n2, n3;
    box_muller(r0, r1, n0, n1);
    box_muller(r2, r3, n2, n3);
    const float v[4] = {n0, n1, n2, n3};
    const long base = q << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (base + j < d) out[base + j] = from_f<T>(mu + sigma * v[j]);
  }
}

}  // namespace

template <typename T>
void launch_little(const T* X, T* out, int n, long d, float z,
                   hipStream_t stream) {
  const int block = 256;
  const long want = (d + block - 1) / block;
  const int grid = (int)(want < 8192 ? (want > 0 ? want : 1) : 8192);
  hipLaunchKernelGGL(little_kernel<T>, dim3(grid), dim3(block), 0, stream, X,
                     out, n, d, z);
}

template <typename T>
void launch_gaussian_fill(T* out, long d, unsigned long long seed, float mu,
                          float sigma, hipStream_t stream) {
  const int block = 256;
  const long nquads = (d + 3) >> 2;
  const long want = (nquads + block - 1) / block;
  const int grid = (int)(want < 8192 ? (want > 0 ? want : 1) : 8192);
  hipLaunchKernelGGL(gaussian_fill_kernel<T>, dim3(grid), dim3(block), 0,
                     stream, out, d, (u32)seed, (u32)(seed >> 32), mu, sigma);
}

// CUs of the MI355X: the register kernel's grid is sized to be resident at
// once, because every block ends in 2n + 1 atomic adds on the same words
constexpr int STATS_CUS = 256;

template <typename T>
void launch_attack_stats(const T* X, float* mu, float* p, float* stats, int n,
                         long d, int perturb, hipStream_t stream) {
  const long want = (d + STATS_BLOCK - 1) / STATS_BLOCK;
  const bool fused = n <= 64;
  by_perturb(perturb, [&](auto pt) {
    constexpr int PERT = decltype(pt)::value;
    if (fused) {
      // one block is one wave per SIMD: blocks per CU = waves per SIMD
      const long cap = STATS_CUS * (n > 32 ? 2 : 4);
      const int grid = (int)(want < cap ? (want > 0 ? want : 1) : cap);
      auto launch = [&](auto w) {
        hipLaunchKernelGGL(
            (attack_stats_reg_kernel<decltype(w)::value, PERT, T>), dim3(grid),
            dim3(STATS_BLOCK), 0, stream, X, mu, p, stats, n, d);
      };
      if (n <= 8) launch(std::integral_constant<int, 8>{});
      else if (n <= 16) launch(std::integral_constant<int, 16>{});
      else if (n <= 32) launch(std::integral_constant<int, 32>{});
      else launch(std::integral_constant<int, 64>{});
      return;
    }
    const int grid = (int)(want < 2048 ? (want > 0 ? want : 1) : 2048);
    hipLaunchKernelGGL((attack_moments_kernel<PERT, T>), dim3(grid),
                       dim3(STATS_BLOCK), 0, stream, X, mu, p, stats + 2 * n, n,
                       d);
  });
  if (fused) return;
  // a_i = ||x_i - mu||^2; caf_matvec gives sum_j (x_ij - mu_j) p_j = -b_i
  launch_row_center_sqdists<T>(X, mu, stats, n, d, stream);
  launch_caf_matvec<T>(X, mu, p, stats + n, n, d, stream);
  hipLaunchKernelGGL(negate_kernel, dim3((n + 255) / 256), dim3(256), 0, stream,
                     stats + n, n);
}

INSTANTIATE_LAUNCHER(launch_little)
INSTANTIATE_LAUNCHER(launch_attack_stats)
INSTANTIATE_LAUNCHER(launch_gaussian_fill)
