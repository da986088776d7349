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
constexpr int GFP_MAX_SUMS = 4;  // vectors one two-level sum reduces at once

struct GfpShared {
  double part[GFP_MAX_SEGS][GRAMFP_MAX_N];  // segment partials of the matvec
  double x[GRAMFP_MAX_N];                   // the matvec's operand, 0 past n
  double v[GFP_MAX_SUMS][GRAMFP_MAX_N];     // vectors to be summed, 0 past n
  double seg[GFP_MAX_SUMS][GFP_MAX_SEGS];   // their segment sums
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

// out[j] = sum s.v[j] for j < K, the same in every thread; with MAXLAST the
// last one is the maximum of s.v[K - 1] instead (values >= 0). s.v must have
// been written by the slot threads; the leading barrier publishes it.
template <int K, bool MAXLAST = false>
DEV void gfp_sum(GfpShared& s, const GfpThread& t, double (&out)[K]) {
  static_assert(K <= GFP_MAX_SUMS, "one LDS vector per sum");
  __syncthreads();
  if (t.tid < t.segs) {
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < GFP_SEG; ++k) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double x = s.v[j][t.tid * GFP_SEG + k];
        acc[j] = (MAXLAST && j == K - 1) ? fmax(acc[j], x) : acc[j] + x;
      }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) s.seg[j][t.tid] = acc[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double r = 0.0;
    for (int k = 0; k < t.segs; ++k) {
      const double x = s.seg[j][k];
      r = (MAXLAST && j == K - 1) ? fmax(r, x) : r + x;
    }
    out[j] = r;
  }
}

DEV void gfp_sum2(GfpShared& s, const GfpThread& t, double& s0, double& s1) {
  double r[2];
  gfp_sum<2>(s, t, r);
  s0 = r[0];
  s1 = r[1];
}

// Which part of the block this thread is, for n rows.
DEV GfpThread gfp_thread(int n) {
  GfpThread t;
  t.tid = threadIdx.x;
  t.segs = (n + GFP_SEG - 1) / GFP_SEG;
  t.i = t.tid % n;
  t.r = t.tid / n;
  t.active = t.r < t.segs;
  t.row = t.tid < n;
  t.slot = t.tid < GRAMFP_MAX_N;
  return t;
}

// Thread (r, i)'s 16 Gram entries; entries that are not finite are read as 0.
DEV void gfp_load(const float* __restrict__ G, int n, const GfpThread& t,
                  float (&g)[GFP_SEG]) {
#pragma unroll
  for (int m = 0; m < GFP_SEG; ++m) {
    const int k = t.r * GFP_SEG + m;
    float x = (t.active && k < n) ? G[(long)t.i * n + k] : 0.0f;
    if (!(fabsf(x) < INFINITY)) x = 0.0f;
    g[m] = x;
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
  const GfpThread t = gfp_thread(n);
  float g[GFP_SEG];
  gfp_load(G, n, t, g);
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

// -- CAF on the Gram (K21) ----------------------------------------------------
//
// The covariance-bound filter never leaves the span of the centred rows. With
// weights w, p = w / sum w, mu = X^T p, y_i = x_i - mu and a direction
// v = Y^T b, the weighted covariance acts on the n coefficients as
//   C b = H G H^T b,  H = I - 1 p^T:
//   bt = b - p sum(b),  u = G bt,  (C b)_i = u_i - p.u,  p.u = (G p).bt.
// s = C b are the projections Y v, a power step is b' = p o s with
// ||Y^T b'||^2 = b'^T C b', and the downweighting, the stop test and the
// best-lambda tracking need s, w and lambda only. So the whole filter, all
// its rounds, is this one block on the register-resident Gram.
//
// What a round costs is block-wide barriers, 2 per matvec and 2 per two-level
// sum, so the loop is laid out to need few of them:
//  - G p is one matvec per round. With it, p.u = (G p).b - ((G p).p) sum(b):
//    the centring scalar sum(b) and (G p).b ride in ONE sum, taken BEFORE the
//    matvec, and the centring itself is folded into the operand bt.
//  - A power step is one matvec and one sum. The sum that follows the matvec
//    returns the quadratic form b'^T C b', and already sum(b'') and
//    (G p).b'' of the next step's b'' = p o s' (scaled by 1 / lambda
//    afterwards, C being linear), and max |s'| for the downweighting. The
//    C b' that gives lambda is, over lambda, the next step's s: no matvec is
//    spent on projections.
//  Barriers: 4 per power step; per round 2 (G p) + 2 (seed sums) + 2 (C seed)
//  + 2 (its norm) + 4 * steps + 2 (sum w_next) = 10 + 4 * steps, 22 at the
//  default 3 steps. There are at most n rounds.
// The loop ends on a block-wide vote: every thread holds the same wsum and
// sum(w_next). The next round's wsum IS this round's sum(w_next).
//
// Everything past the f32 Gram entries is f64, every sum runs in index order
// and there are no atomics: the same bits in give the same bits out. Every
// quadratic form is clamped at 0 before its square root (an f32-rounded Gram
// is not exactly PSD). Dead rows (G_ii not finite) have w = 0 from the start,
// seed entry 0, projection 0, and enter no sum and no maximum.
//
// Measured on MI355X (benchmarks/RESULTS_MI355X_caf_gram.md): a round takes
// about 10 us at n = 64 and 16 us at n = 128. A typical launch (2 rounds) is
// 0.02 to 0.04 ms, 6 % of one pass over a 64 x 16M bf16 matrix (0.37 ms). The
// worst case, all n rounds, is 0.63 ms at n = 64 and 2.03 ms at n = 128: MORE
// than one pass over X, five of them at n = 128.
__global__ void __launch_bounds__(GFP_THREADS)
caf_gram_kernel(const float* __restrict__ G, const float* __restrict__ seeds,
                int n, int f, int steps, float* __restrict__ a_out,
                float* __restrict__ lam_out, int* __restrict__ rounds_out) {
  __shared__ GfpShared s;
  const GfpThread t = gfp_thread(n);
  float g[GFP_SEG];
  gfp_load(G, n, t, g);
  const bool live = t.row && fabsf(G[(long)t.tid * n + t.tid]) < INFINITY;

  double w = live ? 1.0 : 0.0;
  double r1[1], r3[3], r4[4];
  if (t.slot) s.v[0][t.tid] = w;
  gfp_sum<1>(s, t, r1);
  double wsum = r1[0];  // the number of live rows
  const double target = (double)(n - 2 * f);
  double best = wsum > 0.0 ? w / wsum : 0.0;
  double best_lambda = INFINITY;
  int rounds = 0;

  // wsum > 0 at the top of every round: a round whose sum(w_next) is 0 stops
  for (int r = 0; r < n && wsum > 0.0; ++r) {
    const double p = w / wsum;
    if (t.slot) s.x[t.tid] = p;
    const double gp = gfp_matvec(s, t, g);  // 0 in dead rows: p is 0 there
    const double b = live ? (double)seeds[(long)r * n + t.tid] : 0.0;
    if (t.slot) {
      s.v[0][t.tid] = b;
      s.v[1][t.tid] = gp * b;
      s.v[2][t.tid] = gp * p;
    }
    gfp_sum<3>(s, t, r3);
    const double gpp = r3[2];
    // sc = s / nrm is C of the unit-length seed direction
    if (t.slot) s.x[t.tid] = b - p * r3[0];
    double sc = gfp_matvec(s, t, g);
    sc = live ? sc - (r3[1] - gpp * r3[0]) : 0.0;
    if (t.slot) {
      s.v[0][t.tid] = b * sc;
      s.v[1][t.tid] = p * sc;
      s.v[2][t.tid] = gp * p * sc;
    }
    gfp_sum<3>(s, t, r3);
    double scale = fmax(sqrt(fmax(r3[0], 0.0)), 1e-20);
    sc /= scale;
    double sb = r3[1] / scale;  // sum(b') and (G p).b' of b' = p o sc
    double gb = r3[2] / scale;
    double lambda = 0.0, smax = 0.0;
    for (int k = 0; k < steps; ++k) {
      const double bp = p * sc;
      if (t.slot) s.x[t.tid] = bp - p * sb;
      double sn = gfp_matvec(s, t, g);
      sn = live ? sn - (gb - gpp * sb) : 0.0;
      if (t.slot) {
        s.v[0][t.tid] = bp * sn;
        s.v[1][t.tid] = p * sn;
        s.v[2][t.tid] = gp * p * sn;
        s.v[3][t.tid] = fabs(sn);
      }
      gfp_sum<4, true>(s, t, r4);
      lambda = sqrt(fmax(r4[0], 0.0));
      scale = fmax(lambda, 1e-20);
      sc = sn / scale;
      sb = r4[1] / scale;
      gb = r4[2] / scale;
      smax = r4[3] / scale;
    }
    if (lambda < best_lambda) {  // strict: the first minimum wins
      best_lambda = lambda;
      best = p;
    }
    // max_i (sc_i^2) == (max_i |sc_i|)^2 bit for bit: rounding is monotone
    const double pmax = fmax(smax * smax, 1e-20);
    const double wn = fmax(w * (1.0 - sc * sc / pmax), 0.0);
    if (t.slot) s.v[0][t.tid] = wn;
    gfp_sum<1>(s, t, r1);
    ++rounds;
    // every thread holds the same wsum and r1[0]: the vote is unanimous
    if (wsum <= target || r1[0] <= 0.0) break;
    w = wn;
    wsum = r1[0];
  }

  if (t.row) a_out[t.tid] = (float)best;
  if (t.tid == 0) {
    *lam_out = (float)best_lambda;
    *rounds_out = rounds;
  }
}

// -- a whole gossip round on one shared Gram (K23) ----------------------------
//
// All node states are rows of one matrix, so its Gram G holds every node's
// neighbourhood sub-Gram G[S, S]. One WAVE solves one node, four nodes to a
// workgroup: a neighbourhood has m <= 32 rows, so lane r owns row r, a node
// never leaves its wave, and the loop has no block barrier at all (the K20
// kernel above pays four a step because it serves n = 128).
//  - gather: lane r reads row r of the sub-Gram straight into 32 f64
//    registers (the entries are f32: widening is exact). A padded slot (-1)
//    is dead, and so is a slot whose G_ii is not finite; entries of dead
//    pairs and entries that are not finite read as 0.
//  - NNM (nnm_f >= 0): lane r ranks D_rs = G_rr + G_ss - 2 G_rs over the live
//    s and keeps the k = max(live - f, 1) nearest, itself included, the lower
//    slot on a tie: a 32-bit mask per row. G_Y = W G W^T in two halves:
//    lane r sums its row over each mask j (T = G W^T, to the wave's LDS
//    tile), lane i sums the rows of T in its own mask; both in slot order,
//    then one scale by 1 / k^2. A dead row mixes nothing and stays dead.
//  - loop: K20's, with lane i holding row i of G_Y. The matvec reads the
//    operand lane by lane (32 fma in slot order), the sums are a 6-level
//    xor butterfly whose partners add the same two numbers, so every lane
//    holds the same bits and the wave stops as one.
//  - pull back c = W^T a, scatter through a wave-private LDS row so that
//    row i of A is written once, zeros included.
// f64 throughout, no atomics: the same G bits give the same A bits.
constexpr int GSP_WAVES = 4;
constexpr int GSP_M = GOSSIP_MAX_M;

DEV double gsp_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Orders this wave's LDS accesses, for the compiler: the LDS serves one
// wave's operations in order.
DEV void gsp_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// y_lane = sum_j gy[j] x_j, x_j lane j's x
DEV double gsp_matvec(const double (&gy)[GSP_M], double x) {
  double y = 0.0;
#pragma unroll
  for (int j = 0; j < GSP_M; ++j) y = fma(gy[j], __shfl(x, j, 64), y);
  return y;
}

__global__ void __launch_bounds__(GSP_WAVES * 64)
gossip_solve_kernel(const float* __restrict__ G, const int* __restrict__ groups,
                    int n, int M, int m, int nnm_f, double eps, double tol2,
                    int iters, float* __restrict__ A,
                    int* __restrict__ steps_out) {
  __shared__ double tile[GSP_WAVES][GSP_M][GSP_M + 1];
  __shared__ float crow[GSP_WAVES][GRAMFP_MAX_N];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int node = blockIdx.x * GSP_WAVES + wave;
  if (node >= M) return;  // the whole wave; nothing below is block-wide

  int idx = lane < m ? groups[(long)node * m + lane] : -1;
  if (idx >= n) idx = -1;
  double gii = 0.0;
  int live = 0;
  if (idx >= 0) {
    const float gf = G[(long)idx * n + idx];
    live = fabsf(gf) < INFINITY;
    if (live) gii = (double)gf;
  }
  double gy[GSP_M];
#pragma unroll
  for (int s = 0; s < GSP_M; ++s) {
    const int is = __shfl(idx, s, 64);
    const int ls = __shfl(live, s, 64);
    float x = (live && ls) ? G[(long)idx * n + is] : 0.0f;
    if (!(fabsf(x) < INFINITY)) x = 0.0f;
    gy[s] = (double)x;
  }
  const int nlive = __popcll(__ballot(live));

  unsigned mask = 0;  // row `lane` of the mixing as bits; W = mask / k
  double inv_k = 1.0;
  if (nnm_f >= 0) {
    const int k = nlive - nnm_f > 1 ? nlive - nnm_f : 1;
    inv_k = 1.0 / (double)k;
    double dist[GSP_M];
#pragma unroll
    for (int s = 0; s < GSP_M; ++s) {
      const double gss = __shfl(gii, s, 64);
      const int ls = __shfl(live, s, 64);
      dist[s] = ls ? gii + gss - 2.0 * gy[s] : (double)INFINITY;
    }
#pragma unroll
    for (int s = 0; s < GSP_M; ++s) {
      int rank = 0;
#pragma unroll
      for (int t = 0; t < GSP_M; ++t)
        rank += (dist[t] < dist[s]) || (t < s && dist[t] == dist[s]);
      if (live && dist[s] < (double)INFINITY && rank < k) mask |= 1u << s;
    }
    // T = G W^T k: row `lane`, summed over each row j's members
#pragma unroll
    for (int j = 0; j < GSP_M; ++j) {
      const unsigned mj = (unsigned)__shfl((int)mask, j, 64);
      double t = 0.0;
#pragma unroll
      for (int s = 0; s < GSP_M; ++s)
        if ((mj >> s) & 1u) t += gy[s];
      if (lane < GSP_M) tile[wave][lane][j] = t;
    }
    gsp_fence();
#pragma unroll
    for (int j = 0; j < GSP_M; ++j) gy[j] = 0.0;
    for (int r = 0; r < GSP_M; ++r)
      if ((mask >> r) & 1u) {
#pragma unroll
        for (int j = 0; j < GSP_M; ++j) gy[j] += tile[wave][r][j];
      }
#pragma unroll
    for (int j = 0; j < GSP_M; ++j) {
      gy[j] *= inv_k * inv_k;
      if (j == lane) gii = gy[j];
    }
  }

  // K20's loop; every quantity is 0 in the lanes that own no live row
  double a = live ? 1.0 / (double)nlive : 0.0;
  double u = gsp_matvec(gy, a);
  double q = gsp_sum(a * u);
  int steps = 0;
  for (int it = 0; it < iters; ++it) {
    const double dist = fmax(sqrt(fmax(gii - 2.0 * u + q, 0.0)), eps);
    const double c = live ? 1.0 / dist : 0.0;
    const double sc = gsp_sum(c);
    const double an = sc > 0.0 ? c / sc : 0.0;
    const double da = an - a;
    const double tv = gsp_matvec(gy, da);
    u += tv;
    a = an;
    const double shift2 = gsp_sum(da * tv);
    q = gsp_sum(a * u);
    ++steps;
    // every lane holds the same shift2: the wave stops as one
    if (tol2 > 0.0 && shift2 <= tol2) break;
  }

  double c = a;  // coefficients over the rows of X: W^T a
  if (nnm_f >= 0) {
    c = 0.0;
#pragma unroll
    for (int r = 0; r < GSP_M; ++r) {
      const unsigned mr = (unsigned)__shfl((int)mask, r, 64);
      const double ar = __shfl(a, r, 64);
      if ((mr >> (lane & 31)) & 1u) c += ar;
    }
    c *= inv_k;
  }
  crow[wave][lane] = 0.0f;
  crow[wave][lane + 64] = 0.0f;
  gsp_fence();
  if (idx >= 0) crow[wave][idx] = (float)c;
  gsp_fence();
  for (int j = lane; j < n; j += 64) A[(long)node * n + j] = crow[wave][j];
  if (lane == 0) steps_out[node] = steps;
}

}  // namespace

void launch_gossip_solve(const float* G, const int* groups, int n, int M, int m,
                         int nnm_f, double eps, double tol2, int iters,
                         float* A, int* steps, hipStream_t stream) {
  hipLaunchKernelGGL(gossip_solve_kernel,
                     dim3((M + GSP_WAVES - 1) / GSP_WAVES),
                     dim3(GSP_WAVES * 64), 0, stream, G, groups, n, M, m, nnm_f,
                     eps, tol2, iters, A, steps);
}

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

void launch_caf_gram(const float* G, const float* seeds, int n, int f,
                     int power_iters, float* a, float* lam, int* rounds,
                     hipStream_t stream) {
  const int segs = (n + GFP_SEG - 1) / GFP_SEG;
  int threads = ((segs * n + 63) / 64) * 64;
  if (threads < GRAMFP_MAX_N) threads = GRAMFP_MAX_N;
  const int steps = power_iters < 1 ? 1 : power_iters;
  hipLaunchKernelGGL(caf_gram_kernel, dim3(1), dim3(threads), 0, stream, G,
                     seeds, n, f, steps, a, lam, rounds);
}
