// Row/column primitives, by binding and kernel:
//   row_sqnorms        (n,d) -> (n,)        per-row ||x||^2   row_red_kernel
//   row_center_sqdists (n,d),(d,) -> (n,)   per-row ||x - z||^2
//                                           center_sqdists_group_kernel
//   row_scale          (n,d),(n,) -> (n,d)  row scaling (clip apply)
//                                           row_scale_kernel
//   mean_rows          gather-mean of selected rows -> (d,)
//   group_mean_rows    per-group gather-mean -> (g,d)   (NNM mixing)
//                                           gather_mean_kernel (both)
//   mean_rows(count=)  the same over idx[:count], count read on the device
//                                           gather_mean_counted_kernel
//   mean_rows(count=, weights=)  the weighted mean over idx[:count]
//                                           gather_wmean_counted_kernel
//   bucket_mean        permuted segmented mean -> (nb,d) (Bucketing)
//                                           bucket_mean_kernel
//   weiszfeld_iter/_apply  w=1/max(dist,eps); z' = sum(w x)/sum(w); ||dz||^2
//                                           weiszfeld_update_kernel
//   weiszfeld_iter_grouped the same for G independent (m,d) problems
//       center_sqdists_grouped_kernel + weiszfeld_update_grouped_kernel
//   cc_iter/_apply     alpha=min(1,c/dist); v' = v + sum(alpha (x-v))/n
//                                           cc_update_kernel
//   caf_matvec         s_i = sum_j (x_ij - mu_j) v_j
//                                           caf_matvec_group_kernel
//   caf_colsum         t_j = scale * sum_i a_i (x_ij - mu_j)
//                                           caf_colsum_kernel
//
// All kernels are HBM-bound; loads are vectorized to 16 B/lane (f32x4 /
// bf16x8 — guide G13: hipcc does not auto-vectorize bf16) with a scalar
// fallback when d is not a multiple of the vector width. Row reductions:
// 2D grid (k-slab, row) + block reduce + one f32 atomic per block (G12).
// Column kernels: V consecutive coordinates per thread, row loop inside;
// per-row weights (1/dist etc.) are staged once in LDS per block.
//
// Two loop nests carry nine of the eleven kernels and are written once:
// col_wsum (weighted column sum) and row_group_reduce (per-row reduction of
// a group of rows against shared f32 operands). Two paths stay outside on
// purpose, each with its reason next to it: cc_update's scalar path (another
// expression) and caf_colsum's vector path (bit-equality). Whatever depends
// on the launch geometry (start, stride, block size, wave count) is computed
// in the kernel body and passed in: hipcc folds blockDim.x to the plain block
// size only there, and reads it again per use inside a device function.
#include "common.h"
#include "launchers.h"
#include <type_traits>

namespace {

// MAX_N_LDS (launchers.h): per-row weight stage, 4 KB

// -- vector load/store ------------------------------------------------------

template <typename T>
struct VecTraits;

template <>
struct VecTraits<float> {
  static constexpr int V = 4;
  static DEV void load(const float* p, float (&o)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  static DEV void store(float* p, const float (&o)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  }
};

template <>
struct VecTraits<__hip_bfloat16> {
  static constexpr int V = 8;
  static DEV float unpack(unsigned u) {
    union { unsigned short s; __hip_bfloat16 h; } c;
    c.s = (unsigned short)u;
    return __bfloat162float(c.h);
  }
  static DEV unsigned short pack(float x) {
    union { unsigned short s; __hip_bfloat16 h; } c;
    c.h = __float2bfloat16(x);
    return c.s;
  }
  static DEV void load(const __hip_bfloat16* p, float (&o)[8]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    o[0] = unpack(v.x); o[1] = unpack(v.x >> 16);
    o[2] = unpack(v.y); o[3] = unpack(v.y >> 16);
    o[4] = unpack(v.z); o[5] = unpack(v.z >> 16);
    o[6] = unpack(v.w); o[7] = unpack(v.w >> 16);
  }
  static DEV void store(__hip_bfloat16* p, const float (&o)[8]) {
    uint4 v;
    v.x = pack(o[0]) | ((unsigned)pack(o[1]) << 16);
    v.y = pack(o[2]) | ((unsigned)pack(o[3]) << 16);
    v.z = pack(o[4]) | ((unsigned)pack(o[5]) << 16);
    v.w = pack(o[6]) | ((unsigned)pack(o[7]) << 16);
    *reinterpret_cast<uint4*>(p) = v;
  }
};

// -- weighted column sum -----------------------------------------------------
// out[j] = fin(j, sum_{i in [lo, hi)} wt(i) * X[row(i), j]) for the columns
// of this thread: V consecutive coordinates per grid-stride step when VEC,
// else one. row(i) maps the loop index to a row of X, wt(i) is its f32
// weight (a constant 1.0f folds away), fin(j, acc) finishes coordinate j.
// Association is fixed: (w0 x0 + w1 x1) + (w2 x2 + w3 x3) per 4 rows, then
// a one-row tail.

template <typename T, bool VEC, typename O, typename Row, typename Wt,
          typename Fin>
DEV void col_wsum(const T* __restrict__ X, O* __restrict__ out, long d,
                  long start, long stride, int lo, int hi, Row row, Wt wt,
                  Fin fin) {
  if constexpr (VEC) {
    constexpr int V = VecTraits<T>::V;
    const long dv = d / V;
    for (long jv = start; jv < dv; jv += stride) {
      float acc[V] = {0};
      // 4 independent row loads in flight per step (a single runtime-n
      // loop leaves one load outstanding and goes latency-bound)
      int i = lo;
      for (; i + 4 <= hi; i += 4) {
        float x0[V], x1[V], x2[V], x3[V];
        VecTraits<T>::load(X + (long)row(i + 0) * d + jv * V, x0);
        VecTraits<T>::load(X + (long)row(i + 1) * d + jv * V, x1);
        VecTraits<T>::load(X + (long)row(i + 2) * d + jv * V, x2);
        VecTraits<T>::load(X + (long)row(i + 3) * d + jv * V, x3);
        const float w0 = wt(i), w1 = wt(i + 1), w2 = wt(i + 2), w3 = wt(i + 3);
#pragma unroll
        for (int c = 0; c < V; ++c)
          acc[c] += (w0 * x0[c] + w1 * x1[c]) + (w2 * x2[c] + w3 * x3[c]);
      }
      for (; i < hi; ++i) {
        const float w = wt(i);
        float x[V];
        VecTraits<T>::load(X + (long)row(i) * d + jv * V, x);
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] += w * x[c];
      }
      if constexpr (std::is_same<O, float>::value) {
#pragma unroll
        for (int c = 0; c < V; ++c) out[jv * V + c] = fin(jv * V + c, acc[c]);
      } else {  // bf16 results: one packed 16 B store
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] = fin(jv * V + c, acc[c]);
        VecTraits<O>::store(out + jv * V, acc);
      }
    }
  } else {
    for (long j = start; j < d; j += stride) {
      float acc = 0.0f;
      for (int i = lo; i < hi; ++i)
        acc += wt(i) * to_f<T>(X[(long)row(i) * d + j]);
      out[j] = from_f<O>(fin(j, acc));
    }
  }
}

// Stages w(i), i < n, in w_lds once per block of nthreads threads; returns
// sum_i w(i) in every thread (summed in row order).
template <typename W>
DEV float stage_weights(float* w_lds, int n, unsigned nthreads, W w) {
  for (int i = threadIdx.x; i < n; i += nthreads) w_lds[i] = w(i);
  __syncthreads();
  float sum = 0.0f;
  for (int i = 0; i < n; ++i) sum += w_lds[i];
  return sum;
}

// -- row-group reduction -----------------------------------------------------
// out[i] += sum_j term(Xg[i, j], f_0[j], .., f_{K-1}[j]) for the `rows` <=
// DIST_GROUP rows of one block. The K f32 operand vectors (a center z; or
// mu and v) are read once per column step and shared by the whole group
// instead of once per row — at small n the f32 center dominates traffic
// (n=8 bf16: z re-reads were 2/3 of all bytes). One block reduction and one
// atomic per row; nw is the kernel's block_waves().

constexpr int DIST_GROUP = 32;  // rows per block (blockIdx.y = group of 32)

template <typename T, bool VEC, int K, typename Term>
DEV void row_group_reduce(const T* __restrict__ Xg,
                          const float* const (&ops)[K],
                          float* __restrict__ out, int rows, long d,
                          long start, long stride, int nw, Term term) {
  __shared__ float lds[DIST_GROUP][16];
  float acc[DIST_GROUP] = {0};
  if constexpr (VEC) {
    constexpr int V = VecTraits<T>::V;
    const long dv = d / V;
    for (long jv = start; jv < dv; jv += stride) {
      float f[V][K];
      {
        // operands are f32; load V floats as V/4 float4s
        float tmp[4];
#pragma unroll
        for (int q4 = 0; q4 < V / 4; ++q4) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            VecTraits<float>::load(ops[k] + jv * V + q4 * 4, tmp);
#pragma unroll
            for (int c = 0; c < 4; ++c) f[q4 * 4 + c][k] = tmp[c];
          }
        }
      }
      // full groups of 4 rows keep 4 loads in flight
      int i = 0;
      for (; i + 4 <= rows; i += 4) {
        float x0[V], x1[V], x2[V], x3[V];
        VecTraits<T>::load(Xg + (long)(i + 0) * d + jv * V, x0);
        VecTraits<T>::load(Xg + (long)(i + 1) * d + jv * V, x1);
        VecTraits<T>::load(Xg + (long)(i + 2) * d + jv * V, x2);
        VecTraits<T>::load(Xg + (long)(i + 3) * d + jv * V, x3);
#pragma unroll
        for (int c = 0; c < V; ++c) {
          acc[i + 0] += term(x0[c], f[c]);
          acc[i + 1] += term(x1[c], f[c]);
          acc[i + 2] += term(x2[c], f[c]);
          acc[i + 3] += term(x3[c], f[c]);
        }
      }
      for (; i < rows; ++i) {
        float x[V];
        VecTraits<T>::load(Xg + (long)i * d + jv * V, x);
#pragma unroll
        for (int c = 0; c < V; ++c) acc[i] += term(x[c], f[c]);
      }
    }
  } else {
    for (long j = start; j < d; j += stride) {
      float f[K];
#pragma unroll
      for (int k = 0; k < K; ++k) f[k] = ops[k][j];
      for (int i = 0; i < rows; ++i)
        acc[i] += term(to_f<T>(Xg[(long)i * d + j]), f);
    }
  }
#pragma unroll
  for (int i = 0; i < DIST_GROUP; ++i) {
    if (i < rows) {
      const float s = block_reduce_sum(acc[i], lds[i], nw);
      if (threadIdx.x == 0) atomicAdd(&out[i], s);
    }
    __syncthreads();
  }
}

// (x - z)^2, the term of both center-distance kernels
struct SqDistTerm {
  DEV float operator()(float x, const float (&f)[1]) const {
    const float dd = x - f[0];
    return dd * dd;
  }
};

// -- row reductions ---------------------------------------------------------

template <typename T, bool CENTER, bool VEC>
__global__ void row_red_kernel(const T* __restrict__ X,
                               const float* __restrict__ z,
                               float* __restrict__ out, long d) {
  __shared__ float lds[16];
  constexpr int V = VecTraits<T>::V;
  const int row = blockIdx.y;
  const T* xr = X + (long)row * d;
  float acc = 0.0f;
  if (VEC) {
    const long dv = d / V;
    const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    long jv = start;
    // 4 grid-stride positions per step: 4 loads in flight
    for (; jv + 3 * stride < dv; jv += 4 * stride) {
      float x0[V], x1[V], x2[V], x3[V];
      VecTraits<T>::load(xr + jv * V, x0);
      VecTraits<T>::load(xr + (jv + stride) * V, x1);
      VecTraits<T>::load(xr + (jv + 2 * stride) * V, x2);
      VecTraits<T>::load(xr + (jv + 3 * stride) * V, x3);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        float v0 = x0[c], v1 = x1[c], v2 = x2[c], v3 = x3[c];
        if (CENTER) {
          v0 -= z[jv * V + c];
          v1 -= z[(jv + stride) * V + c];
          v2 -= z[(jv + 2 * stride) * V + c];
          v3 -= z[(jv + 3 * stride) * V + c];
        }
        acc += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
      }
    }
    for (; jv < dv; jv += stride) {
      float x[V];
      VecTraits<T>::load(xr + jv * V, x);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        float v = x[c];
        if (CENTER) v -= z[jv * V + c];
        acc += v * v;
      }
    }
  } else {
    const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long j = start; j < d; j += stride) {
      float v = to_f<T>(xr[j]);
      if (CENTER) v -= z[j];
      acc += v * v;
    }
  }
  acc = block_reduce_sum(acc, lds);
  if (threadIdx.x == 0) atomicAdd(&out[row], acc);
}

// -- center distances ---------------------------------------------------------
// ||x_i - z||^2 for the rows [g0, g0 + DIST_GROUP) of one (n, d) matrix.

template <typename T, bool VEC>
__global__ void center_sqdists_group_kernel(const T* __restrict__ X,
                                            const float* __restrict__ z,
                                            float* __restrict__ out, int n,
                                            long d) {
  const int g0 = blockIdx.y * DIST_GROUP;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const float* const ops[1] = {z};
  row_group_reduce<T, VEC>(X + (long)g0 * d, ops, out + g0,
                           min(DIST_GROUP, n - g0), d, start, stride,
                           block_waves(), SqDistTerm{});
}

// -- grouped center distances + Weiszfeld update ---------------------------
// G independent small aggregation problems per launch (gossip: every
// node's geomed iteration in ONE kernel pair instead of 2G launches on
// G streams). blockIdx.y = group; each group has its own center and its
// m <= DIST_GROUP rows.

template <typename T, bool VEC>
__global__ void center_sqdists_grouped_kernel(const T* __restrict__ X,
                                              const float* __restrict__ Z,
                                              float* __restrict__ out, int m,
                                              long d) {
  const int g = blockIdx.y;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const float* const ops[1] = {Z + (long)g * d};
  row_group_reduce<T, VEC>(X + (long)g * m * d, ops, out + (long)g * m, m, d,
                           start, stride, block_waves(), SqDistTerm{});
}

template <typename T, bool VEC>
__global__ void weiszfeld_update_grouped_kernel(
    const T* __restrict__ X, const float* __restrict__ Z,
    const float* __restrict__ dist2, float* __restrict__ Z_new, int m, long d,
    float eps) {
  __shared__ float w_lds[DIST_GROUP];
  const int g = blockIdx.y;
  const float* d2 = dist2 + (long)g * m;
  const float den = stage_weights(w_lds, m, blockDim.x, [&](int i) {
    return 1.0f / fmaxf(sqrtf(d2[i]), eps);
  });
  const float inv_den = 1.0f / den;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  col_wsum<T, VEC>(
      X + (long)g * m * d, Z_new + (long)g * d, d, start, stride, 0, m,
      [](int i) { return i; }, [&](int i) { return w_lds[i]; },
      [&](long, float num) { return num * inv_den; });
}

// -- row scaling ------------------------------------------------------------

template <typename T, bool VEC>
__global__ void row_scale_kernel(const T* __restrict__ X,
                                 const float* __restrict__ s,
                                 T* __restrict__ out, long d) {
  constexpr int V = VecTraits<T>::V;
  const int row = blockIdx.y;
  const float sc = s[row];
  const T* xr = X + (long)row * d;
  T* yr = out + (long)row * d;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  if (VEC) {
    const long dv = d / V;
    for (long jv = start; jv < dv; jv += stride) {
      float x[V];
      VecTraits<T>::load(xr + jv * V, x);
#pragma unroll
      for (int c = 0; c < V; ++c) x[c] *= sc;
      VecTraits<T>::store(yr + jv * V, x);
    }
  } else {
    for (long j = start; j < d; j += stride)
      yr[j] = from_f<T>(to_f<T>(xr[j]) * sc);
  }
}

// -- gather means -----------------------------------------------------------
// GROUPED=false: idx is (k,) and blockIdx.y==0 -> out (d,).
// GROUPED=true:  idx is (g,k) rows per group g=blockIdx.y -> out (g,d).

template <typename T, bool VEC, bool GROUPED>
__global__ void gather_mean_kernel(const T* __restrict__ X,
                                   const int* __restrict__ idx, int k,
                                   T* __restrict__ out, long d) {
  const int g = GROUPED ? blockIdx.y : 0;
  const int* gi = idx + (long)g * k;
  const float inv = 1.0f / (float)k;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  col_wsum<T, VEC>(
      X, out + (long)g * d, d, start, stride, 0, k,
      [&](int i) { return gi[i]; }, [](int) { return 1.0f; },
      [&](long, float acc) { return acc * inv; });
}

// Counted variant (DnC): the row count is an int on the device, read here,
// so a selection whose size is only known on the device needs no host sync.
// A kernel of its own, not a flag on gather_mean_kernel: the un-counted
// instantiations (mean_rows is in the flagship's timed region) keep their
// arguments and instruction stream. Same col_wsum association over
// idx[0 .. count), so the result is bitwise that of mean_rows on idx[:count];
// count 0 writes zeros.
template <typename T, bool VEC>
__global__ void gather_mean_counted_kernel(const T* __restrict__ X,
                                           const int* __restrict__ idx, int k,
                                           const int* __restrict__ count,
                                           T* __restrict__ out, long d) {
  const int cnt = min(max(*count, 0), k);
  const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.0f;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  col_wsum<T, VEC>(
      X, out, d, start, stride, 0, cnt, [&](int i) { return idx[i]; },
      [](int) { return 1.0f; }, [&](long, float acc) { return acc * inv; });
}

// Weighted counted variant (AFA): sum_i w[idx[i]] x[idx[i]] / sum_i w[idx[i]]
// over i < count. Again a kernel of its own, so that the counted kernel
// above keeps its instruction stream too. The cnt <= MAX_N_LDS weights are
// staged once per block; a weight sum that is not positive reads no row and
// writes zeros, like count 0.
template <typename T, bool VEC>
__global__ void gather_wmean_counted_kernel(const T* __restrict__ X,
                                            const int* __restrict__ idx, int k,
                                            const int* __restrict__ count,
                                            const float* __restrict__ w,
                                            int n_src, T* __restrict__ out,
                                            long d) {
  __shared__ float w_lds[MAX_N_LDS];
  int cnt = min(max(*count, 0), min(k, MAX_N_LDS));
  // idx comes from device memory: clamped to the n_src rows of X and w
  const auto src = [&](int i) { return min(max(idx[i], 0), n_src - 1); };
  const float den =
      stage_weights(w_lds, cnt, blockDim.x, [&](int i) { return w[src(i)]; });
  const bool ok = den > 0.0f && den < INFINITY;
  if (!ok) cnt = 0;
  const float inv = ok ? 1.0f / den : 0.0f;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  col_wsum<T, VEC>(
      X, out, d, start, stride, 0, cnt, src, [&](int i) { return w_lds[i]; },
      [&](long, float acc) { return acc * inv; });
}

template <typename T, bool VEC>
__global__ void bucket_mean_kernel(const T* __restrict__ X,
                                   const int* __restrict__ perm, int n,
                                   int bucket, T* __restrict__ out, long d) {
  const int b = blockIdx.y;
  const int lo = b * bucket;
  const int hi = min(n, lo + bucket);
  const float inv = 1.0f / (float)(hi - lo);
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  col_wsum<T, VEC>(
      X, out + (long)b * d, d, start, stride, lo, hi,
      [&](int i) { return perm[i]; }, [](int) { return 1.0f; },
      [&](long, float acc) { return acc * inv; });
}

// -- fused fixed-point iterations ------------------------------------------
// Per-row weights are a function of the global distances only; stage them
// in LDS once per block instead of recomputing per column.

template <typename T, bool VEC>
__global__ void weiszfeld_update_kernel(const T* __restrict__ X,
                                        const float* __restrict__ z,
                                        const float* __restrict__ dist2,
                                        float* __restrict__ z_new,
                                        float* __restrict__ shift2, int n,
                                        long d, float eps) {
  __shared__ float w_lds[MAX_N_LDS];
  __shared__ float red[16];
  const float den = stage_weights(w_lds, n, blockDim.x, [&](int i) {
    return 1.0f / fmaxf(sqrtf(dist2[i]), eps);
  });
  const float inv_den = 1.0f / den;
  float local_shift = 0.0f;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  col_wsum<T, VEC>(
      X, z_new, d, start, stride, 0, n, [](int i) { return i; },
      [&](int i) { return w_lds[i]; },
      [&](long j, float num) {
        const float zi = num * inv_den;
        const float dz = zi - z[j];
        local_shift += dz * dz;
        return zi;
      });
  const float s = block_reduce_sum(local_shift, red);
  if (threadIdx.x == 0) atomicAdd(shift2, s);
}

template <typename T, bool VEC>
__global__ void cc_update_kernel(const T* __restrict__ X,
                                 const float* __restrict__ v,
                                 const float* __restrict__ dist2,
                                 float* __restrict__ v_new, int n, long d,
                                 float c_tau, float eps) {
  __shared__ float a_lds[MAX_N_LDS];
  const float alpha_sum = stage_weights(a_lds, n, blockDim.x, [&](int i) {
    return fminf(1.0f, c_tau / fmaxf(sqrtf(dist2[i]), eps));
  });
  const float inv_n = 1.0f / (float)n;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    // sum(alpha (x - v)) = sum(alpha x) - alpha_sum v: v leaves the row loop
    col_wsum<T, true>(
        X, v_new, d, start, stride, 0, n, [](int i) { return i; },
        [&](int i) { return a_lds[i]; },
        [&](long j, float acc) {
          const float vj = v[j];
          return vj + (acc - alpha_sum * vj) * inv_n;
        });
  } else {
    // the scalar path subtracts v per row: another expression, another
    // rounding, kept as it is
    for (long j = start; j < d; j += stride) {
      const float vj = v[j];
      float acc = 0.0f;
      for (int i = 0; i < n; ++i)
        acc += a_lds[i] * (to_f<T>(X[(long)i * d + j]) - vj);
      v_new[j] = vj + acc * inv_n;
    }
  }
}

// -- CAF fused power-iteration pair (reference caf.py:133-184)
// s_i = sum_j (X_ij - mu_j) v_j            (caf_matvec_group_kernel)
// t_j = (*scale) * sum_i a_i (X_ij - mu_j) (caf_colsum_kernel)
// Neither materializes diffs = X - mu (32 GB f32 at 64 x 125M) and both
// replace rocblas gemvt, which runs at ~260 GB/s on this skinny shape.

template <typename T, bool VEC>
__global__ void caf_matvec_group_kernel(const T* __restrict__ X,
                                        const float* __restrict__ mu,
                                        const float* __restrict__ v,
                                        float* __restrict__ out, int n,
                                        long d) {
  const int g0 = blockIdx.y * DIST_GROUP;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const float* const ops[2] = {mu, v};
  row_group_reduce<T, VEC>(
      X + (long)g0 * d, ops, out + g0, min(DIST_GROUP, n - g0), d, start,
      stride, block_waves(),
      [](float x, const float (&f)[2]) { return (x - f[0]) * f[1]; });
}

// sum_i a_i X_ij - mu_j * sum_i a_i, scaled: the mu subtraction factors out
// of the row loop, so the inner walk is a plain weighted column sum.
// mu may be null (plain weighted sum: computes the weighted mean when
// a = w and *scale = 1/sum(w)); scale may be null (1.0).
template <typename T, bool VEC>
__global__ void caf_colsum_kernel(const T* __restrict__ X,
                                  const float* __restrict__ a,
                                  const float* __restrict__ mu,
                                  const float* __restrict__ scale,
                                  float* __restrict__ out, int n, long d) {
  __shared__ float a_lds[MAX_N_LDS];
  const float a_sum =
      stage_weights(a_lds, n, blockDim.x, [&](int i) { return a[i]; });
  const float sc = scale ? *scale : 1.0f;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    // Not through col_wsum: with the nullable mu, hipcc fuses a_sum * m into
    // the subtraction for only some of the V coordinates, and which ones
    // changes with the shape of the surrounding code; through the skeleton
    // the low bits of t_j moved. This copy stays until a change that may
    // move them.
    constexpr int V = VecTraits<T>::V;
    const long dv = d / V;
    for (long jv = start; jv < dv; jv += stride) {
      float acc[V] = {0};
      int i = 0;
      for (; i + 4 <= n; i += 4) {
        float x0[V], x1[V], x2[V], x3[V];
        VecTraits<T>::load(X + (long)(i + 0) * d + jv * V, x0);
        VecTraits<T>::load(X + (long)(i + 1) * d + jv * V, x1);
        VecTraits<T>::load(X + (long)(i + 2) * d + jv * V, x2);
        VecTraits<T>::load(X + (long)(i + 3) * d + jv * V, x3);
        const float a0 = a_lds[i], a1 = a_lds[i + 1], a2 = a_lds[i + 2],
                    a3 = a_lds[i + 3];
#pragma unroll
        for (int c = 0; c < V; ++c)
          acc[c] += (a0 * x0[c] + a1 * x1[c]) + (a2 * x2[c] + a3 * x3[c]);
      }
      for (; i < n; ++i) {
        const float ai = a_lds[i];
        float x[V];
        VecTraits<T>::load(X + (long)i * d + jv * V, x);
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] += ai * x[c];
      }
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float m = mu ? mu[jv * V + c] : 0.0f;
        out[jv * V + c] = (acc[c] - a_sum * m) * sc;
      }
    }
  } else {
    col_wsum<T, false>(
        X, out, d, start, stride, 0, n, [](int i) { return i; },
        [&](int i) { return a_lds[i]; },
        [&](long j, float acc) {
          const float m = mu ? mu[j] : 0.0f;
          return (acc - a_sum * m) * sc;
        });
  }
}

inline int col_grid(long work, int block) {
  const long want = (work + block - 1) / block;
  return (int)(want < 4096 ? (want > 0 ? want : 1) : 4096);
}

inline int slab_grid(long d, int n, int block) {
  // target ~2048 blocks total across the (slab, row) grid
  long per_row = (d + (long)block * 8 - 1) / ((long)block * 8);
  long cap = 2048 / (n > 0 ? n : 1);
  if (cap < 1) cap = 1;
  return (int)(per_row < cap ? (per_row > 0 ? per_row : 1) : cap);
}

// Picks the VEC instantiation: calls fn(true_type) when d is a multiple of
// the 16 B/lane vector width (VEC kernels), else fn(false_type) (scalar).
template <typename T, typename F>
inline void by_vec(long d, F&& fn) {
  if ((d % VecTraits<T>::V) == 0)
    fn(std::true_type{});
  else
    fn(std::false_type{});
}

// work items of a column kernel: V coordinates per thread when VEC
template <typename T, bool VEC>
inline long col_work(long d) {
  return VEC ? d / VecTraits<T>::V : d;
}

constexpr int BLOCK = 256;  // threads per block, every launcher below

}  // namespace

// ---------------------------------------------------------------------------
// host-side launchers (declared in launchers.h)
// ---------------------------------------------------------------------------

#define VEC_OF(v) decltype(v)::value

template <typename T>
void launch_row_sqnorms(const T* X, float* out, int n, long d,
                        hipStream_t stream) {
  dim3 grid(slab_grid(d, n, BLOCK), n);
  by_vec<T>(d, [&](auto v) {
    hipLaunchKernelGGL((row_red_kernel<T, false, VEC_OF(v)>), grid,
                       dim3(BLOCK), 0, stream, X, nullptr, out, d);
  });
}

template <typename T>
void launch_row_center_sqdists(const T* X, const float* z, float* out, int n,
                               long d, hipStream_t stream) {
  const int groups = (n + DIST_GROUP - 1) / DIST_GROUP;
  dim3 grid(slab_grid(d, groups, BLOCK), groups);
  by_vec<T>(d, [&](auto v) {
    hipLaunchKernelGGL((center_sqdists_group_kernel<T, VEC_OF(v)>), grid,
                       dim3(BLOCK), 0, stream, X, z, out, n, d);
  });
}

template <typename T>
void launch_grouped_weiszfeld(const T* X, const float* Z, float* dist2,
                              float* Z_new, int G, int m, long d, float eps,
                              hipStream_t stream) {
  dim3 grid(slab_grid(d, G, BLOCK), G);
  by_vec<T>(d, [&](auto v) {
    hipLaunchKernelGGL((center_sqdists_grouped_kernel<T, VEC_OF(v)>), grid,
                       dim3(BLOCK), 0, stream, X, Z, dist2, m, d);
    hipLaunchKernelGGL((weiszfeld_update_grouped_kernel<T, VEC_OF(v)>), grid,
                       dim3(BLOCK), 0, stream, X, Z, dist2, Z_new, m, d, eps);
  });
}

template <typename T>
void launch_row_scale(const T* X, const float* s, T* out, int n, long d,
                      hipStream_t stream) {
  dim3 grid(slab_grid(d, n, BLOCK), n);
  by_vec<T>(d, [&](auto v) {
    hipLaunchKernelGGL((row_scale_kernel<T, VEC_OF(v)>), grid, dim3(BLOCK), 0,
                       stream, X, s, out, d);
  });
}

template <typename T>
void launch_mean_rows(const T* X, const int* idx, int k, T* out, long d,
                      hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d);
    hipLaunchKernelGGL((gather_mean_kernel<T, VEC_OF(v), false>),
                       dim3(col_grid(work, BLOCK)), dim3(BLOCK), 0, stream, X,
                       idx, k, out, d);
  });
}

template <typename T>
void launch_mean_rows_counted(const T* X, const int* idx, int k,
                              const int* count, T* out, long d,
                              hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d);
    hipLaunchKernelGGL((gather_mean_counted_kernel<T, VEC_OF(v)>),
                       dim3(col_grid(work, BLOCK)), dim3(BLOCK), 0, stream, X,
                       idx, k, count, out, d);
  });
}

template <typename T>
void launch_mean_rows_counted_weighted(const T* X, const int* idx, int k,
                                       const int* count, const float* w,
                                       int n_src, T* out, long d,
                                       hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d);
    hipLaunchKernelGGL((gather_wmean_counted_kernel<T, VEC_OF(v)>),
                       dim3(col_grid(work, BLOCK)), dim3(BLOCK), 0, stream, X,
                       idx, k, count, w, n_src, out, d);
  });
}

template <typename T>
void launch_group_mean_rows(const T* X, const int* idx, int g, int k, T* out,
                            long d, hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d) / (g > 4 ? 4 : 1) + 1;
    hipLaunchKernelGGL((gather_mean_kernel<T, VEC_OF(v), true>),
                       dim3(col_grid(work, BLOCK), g), dim3(BLOCK), 0, stream,
                       X, idx, k, out, d);
  });
}

template <typename T>
void launch_bucket_mean(const T* X, const int* perm, int n, int bucket, int nb,
                        T* out, long d, hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d) / (nb > 4 ? 4 : 1) + 1;
    hipLaunchKernelGGL((bucket_mean_kernel<T, VEC_OF(v)>),
                       dim3(col_grid(work, BLOCK), nb), dim3(BLOCK), 0, stream,
                       X, perm, n, bucket, out, d);
  });
}

template <typename T>
void launch_weiszfeld_update(const T* X, const float* z, const float* dist2,
                             float* z_new, float* shift2, int n, long d,
                             float eps, hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d);
    hipLaunchKernelGGL((weiszfeld_update_kernel<T, VEC_OF(v)>),
                       dim3(col_grid(work, BLOCK)), dim3(BLOCK), 0, stream, X,
                       z, dist2, z_new, shift2, n, d, eps);
  });
}

template <typename T>
void launch_cc_update(const T* X, const float* v, const float* dist2,
                      float* v_new, int n, long d, float c_tau, float eps,
                      hipStream_t stream) {
  by_vec<T>(d, [&](auto vec) {
    const long work = col_work<T, VEC_OF(vec)>(d);
    hipLaunchKernelGGL((cc_update_kernel<T, VEC_OF(vec)>),
                       dim3(col_grid(work, BLOCK)), dim3(BLOCK), 0, stream, X,
                       v, dist2, v_new, n, d, c_tau, eps);
  });
}

template <typename T>
void launch_caf_matvec(const T* X, const float* mu, const float* v, float* out,
                       int n, long d, hipStream_t stream) {
  const int groups = (n + DIST_GROUP - 1) / DIST_GROUP;
  dim3 grid(slab_grid(d, groups, BLOCK), groups);
  by_vec<T>(d, [&](auto vec) {
    hipLaunchKernelGGL((caf_matvec_group_kernel<T, VEC_OF(vec)>), grid,
                       dim3(BLOCK), 0, stream, X, mu, v, out, n, d);
  });
}

template <typename T>
void launch_caf_colsum(const T* X, const float* a, const float* mu,
                       const float* scale, float* out, int n, long d,
                       hipStream_t stream) {
  by_vec<T>(d, [&](auto v) {
    const long work = col_work<T, VEC_OF(v)>(d);
    hipLaunchKernelGGL((caf_colsum_kernel<T, VEC_OF(v)>),
                       dim3(col_grid(work, BLOCK)), dim3(BLOCK), 0, stream, X,
                       a, mu, scale, out, n, d);
  });
}
#undef VEC_OF

INSTANTIATE_LAUNCHER(launch_row_sqnorms)
INSTANTIATE_LAUNCHER(launch_row_center_sqdists)
INSTANTIATE_LAUNCHER(launch_grouped_weiszfeld)
INSTANTIATE_LAUNCHER(launch_row_scale)
INSTANTIATE_LAUNCHER(launch_mean_rows)
INSTANTIATE_LAUNCHER(launch_mean_rows_counted)
INSTANTIATE_LAUNCHER(launch_mean_rows_counted_weighted)
INSTANTIATE_LAUNCHER(launch_group_mean_rows)
INSTANTIATE_LAUNCHER(launch_bucket_mean)
INSTANTIATE_LAUNCHER(launch_weiszfeld_update)
INSTANTIATE_LAUNCHER(launch_cc_update)
INSTANTIATE_LAUNCHER(launch_caf_matvec)
INSTANTIATE_LAUNCHER(launch_caf_colsum)
