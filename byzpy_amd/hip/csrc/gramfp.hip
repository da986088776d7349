// Fixed-point aggregators solved on the Gram (K20) for gfx950.
//
// A Weiszfeld update is a convex combination of the rows whatever the current
// centre is, and a centered-clipping update keeps v in the row span when v
// starts there. So the iterate is z = sum_i a_i x_i for n numbers a, and with
// G = X X^T, u = G a, q = a^T u
//   ||x_i - z||^2 = G_ii - 2 u_i + q,
//   ||z' - z||^2  = (a' - a)^T G (a' - a).
// The whole data-dependent loop therefore runs on the (n, n) Gram in ONE
// block and one launch: no pass over X per step and no host poll. The loop
// ends on a block-wide vote (every thread holds the same shift^2).
//
// Thread (r, i) keeps G[i][16 r .. 16 r + 15] in registers for every step
// (the layout of afa_select_kernel in subsets.hip). Thread i < n also owns
// row i's scalars a_i, u_i, G_ii in registers. A step is ONE matvec
// t = G (a' - a): 16 f64 FMAs per thread against a' - a in LDS, then one
// thread per row adds its <= 8 segment partials in segment order. From t:
// shift^2 = (a' - a)^T t, u += t, q = a'^T u. Sums over the rows go in two
// levels, both in index order: thread s < segs adds the 16 terms of segment
// s, then every thread adds the <= 8 segment sums. Everything past the f32
// Gram entries is f64 and there are no atomics: the same G bits give the same
// output bits, and the result differs from an f64 evaluation of the same
// loop by reordering of order 1e-16 only.
//
// Dead rows (G_ii not finite: the row holds inf, NaN or overflows the f32
// Gram) have coefficient 0 from start to end, enter no sum, and their Gram
// entries are read as 0, so no 0 * inf is ever formed: the limit of the
// iterative rule, whose weight for such a row is 1 / inf.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int GFP_THREADS = 1024;
constexpr int GFP_SEG = 16;  // Gram entries of one row per thread
constexpr int GFP_MAX_SEGS = GRAMFP_MAX_N / GFP_SEG;
static_assert(GFP_MAX_SEGS * GRAMFP_MAX_N <= GFP_THREADS, "one thread per (segment, row)");

struct GfpShared {
  double part[GFP_MAX_SEGS][GRAMFP_MAX_N];  // segment partials of the matvec
  double x[GRAMFP_MAX_N];                   // the matvec's operand, 0 past n
  double v[2][GRAMFP_MAX_N];                // two vectors to be summed, 0 past n
  double seg[2][GFP_MAX_SEGS];              // their segment sums
};

// Which part of the block a thread is: (r, i) of the matvec, a row owner
// (tid < n), an owner of one slot of the LDS vectors (tid < GRAMFP_MAX_N).
struct GfpThread {
  int tid, i, r, segs;
  bool active, row, slot;
};

// y_tid = sum_k G[tid][k] x[k], valid in the row threads. s.x must have been
// written by the slot threads; the leading barrier publishes it.
DEV double gfp_matvec(GfpShared& s, const GfpThread& t,
                      const float (&g)[GFP_SEG]) {
  __syncthreads();
  if (t.active) {
    double p = 0.0;
#pragma unroll
    for (int m = 0; m < GFP_SEG; ++m)
      p = fma((double)g[m], s.x[t.r * GFP_SEG + m], p);
    s.part[t.r][t.i] = p;
  }
  __syncthreads();
  double y = 0.0;
  if (t.row)
    for (int k = 0; k < t.segs; ++k) y += s.part[k][t.tid];
  return y;
}

// s0 = sum s.v[0], s1 = sum s.v[1], the same in every thread. s.v must have
// been written by the slot threads; the leading barrier publishes it.
DEV void gfp_sum2(GfpShared& s, const GfpThread& t, double& s0, double& s1) {
  __syncthreads();
  if (t.tid < t.segs) {
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int k = 0; k < GFP_SEG; ++k) {
      t0 += s.v[0][t.tid * GFP_SEG + k];
      t1 += s.v[1][t.tid * GFP_SEG + k];
    }
    s.seg[0][t.tid] = t0;
    s.seg[1][t.tid] = t1;
  }
  __syncthreads();
  s0 = 0.0;
  s1 = 0.0;
  for (int k = 0; k < t.segs; ++k) {
    s0 += s.seg[0][k];
    s1 += s.seg[1][k];
  }
}

template <bool CC>
__global__ void __launch_bounds__(GFP_THREADS)
gram_fixed_point_kernel(const float* __restrict__ G,
                        const float* __restrict__ a0, int n, double eps,
                        double tol2, double c_tau, int iters,
                        float* __restrict__ a_out, int* __restrict__ steps_out,
                        float* __restrict__ shift2_out) {
  __shared__ GfpShared s;
  GfpThread t;
  t.tid = threadIdx.x;
  t.segs = (n + GFP_SEG - 1) / GFP_SEG;
  t.i = t.tid % n;
  t.r = t.tid / n;
  t.active = t.r < t.segs;
  t.row = t.tid < n;
  t.slot = t.tid < GRAMFP_MAX_N;

  float g[GFP_SEG];
#pragma unroll
  for (int m = 0; m < GFP_SEG; ++m) {
    const int k = t.r * GFP_SEG + m;
    float x = (t.active && k < n) ? G[(long)t.i * n + k] : 0.0f;
    if (!(fabsf(x) < INFINITY)) x = 0.0f;
    g[m] = x;
  }
  // row scalars; all 0 in the threads that own no live row
  double gii = 0.0, a = 0.0;
  bool live = false;
  if (t.row) {
    const float gf = G[(long)t.tid * n + t.tid];
    live = fabsf(gf) < INFINITY;
    if (live) {
      gii = (double)gf;
      a = (double)a0[t.tid];
    }
  }

  if (t.slot) s.x[t.tid] = a;
  double u = gfp_matvec(s, t, g);
  if (t.slot) {
    s.v[0][t.tid] = a * u;
    s.v[1][t.tid] = 0.0;
  }
  double q, shift2;
  gfp_sum2(s, t, q, shift2);

  int steps = 0;
  for (int it = 0; it < iters; ++it) {
    const double dist = fmax(sqrt(fmax(gii - 2.0 * u + q, 0.0)), eps);
    double c = 0.0;  // Weiszfeld weight or clipping factor of a live row
    if (live) c = CC ? fmin(1.0, c_tau / dist) : 1.0 / dist;
    if (t.slot) {
      s.v[0][t.tid] = c;
      s.v[1][t.tid] = 0.0;
    }
    double sc, unused;
    gfp_sum2(s, t, sc, unused);
    double an;
    if (CC)
      an = (1.0 - sc / (double)n) * a + c / (double)n;
    else
      an = sc > 0.0 ? c / sc : 0.0;
    const double da = an - a;
    if (t.slot) s.x[t.tid] = da;
    const double tv = gfp_matvec(s, t, g);
    u += tv;
    a = an;
    if (t.slot) {
      s.v[0][t.tid] = da * tv;
      s.v[1][t.tid] = a * u;
    }
    gfp_sum2(s, t, shift2, q);
    ++steps;
    // every thread holds the same shift2: the vote is unanimous
    if (!CC && tol2 > 0.0 && shift2 <= tol2) break;
  }

  if (t.row) a_out[t.tid] = (float)a;
  if (t.tid == 0) {
    *steps_out = steps;
    *shift2_out = (float)shift2;
  }
}

}  // namespace

void launch_gram_fixed_point(const float* G, const float* a0, int n, int rule,
                             double eps, double tol2, double c_tau, int iters,
                             float* a, int* steps, float* shift2,
                             hipStream_t stream) {
  // one thread per (segment, row) in whole waves, and at least the
  // GRAMFP_MAX_N threads that own the LDS vectors' slots
  const int segs = (n + GFP_SEG - 1) / GFP_SEG;
  int threads = ((segs * n + 63) / 64) * 64;
  if (threads < GRAMFP_MAX_N) threads = GRAMFP_MAX_N;
  if (rule == GRAMFP_CC)
    hipLaunchKernelGGL(gram_fixed_point_kernel<true>, dim3(1), dim3(threads), 0,
                       stream, G, a0, n, eps, tol2, c_tau, iters, a, steps,
                       shift2);
  else
    hipLaunchKernelGGL(gram_fixed_point_kernel<false>, dim3(1), dim3(threads),
                       0, stream, G, a0, n, eps, tol2, c_tau, iters, a, steps,
                       shift2);
}
