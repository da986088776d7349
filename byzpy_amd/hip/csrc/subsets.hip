// Device-side exact subset searches for gfx950.
//
// SMEA: among C(n, m) row subsets, find the one whose centered subset
// Gram H G_sub H has the smallest max eigenvalue (reference
// smea.py:63-107 runs batched host eigvalsh). Here: ONE WAVE per subset,
// the m x m centered Gram staged in LDS, a fixed-sweep cyclic Jacobi
// eigensolve executed wave-cooperatively, and a packed (eigkey, combo)
// u64 atomicMin so ties resolve to the lexicographically-smallest combo
// index exactly like the oracle's block scan.
//
// MDA: exact minimum-diameter (n-f)-subset (reference
// minimum_diameter_average.py:267-386 runs seeded-DFS subtask batches;
// round 1 copied D2 to the host for a serial C++ branch-and-bound).
// Here the reference's seed_prefix=2 decomposition maps to workgroups:
// one workgroup per (a, b) prefix pair runs a bounded DFS over the
// remaining candidates with per-level incremental max-distance arrays in
// LDS, sharing the global best diameter through an atomicMin every
// improvement. A second bounded pass recovers the lexicographically
// smallest optimal subset (host parity: mda_host.cpp mda_search's dfs2).
#include "common.h"
#include "launchers.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

// non-negative f32 -> monotone u32 (covers tiny negative rounding too)
DEV u32 f32_key(float v) {
  u32 b = __float_as_uint(v);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// ---------------------------------------------------------------------------
// SMEA
// ---------------------------------------------------------------------------

constexpr int SMEA_SWEEPS = 10;

// one 64-lane wave per subset; LDS: A[m*m] + rows[m]
__global__ void __launch_bounds__(64)
smea_select_kernel(const float* __restrict__ G, const int* __restrict__ combos,
                   int n, int m, int C, u64* __restrict__ best) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* A = smem;                 // m*m
  float* rmean = smem + m * m;     // m
  __shared__ int rows[64];
  const int lane = threadIdx.x;

  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    if (lane < m) rows[lane] = combos[(long)c * m + lane];
    __syncthreads();
    // subset Gram
    for (int e = lane; e < m * m; e += 64) {
      const int i = e / m, j = e % m;
      A[e] = G[(long)rows[i] * n + rows[j]];
    }
    __syncthreads();
    // center: A <- A - rmean_i - rmean_j + gmean
    if (lane < m) {
      float s = 0.0f;
      for (int j = 0; j < m; ++j) s += A[lane * m + j];
      rmean[lane] = s / m;
    }
    __syncthreads();
    float gm = 0.0f;
    for (int j = 0; j < m; ++j) gm += rmean[j];
    gm /= m;
    for (int e = lane; e < m * m; e += 64) {
      const int i = e / m, j = e % m;
      A[e] = A[e] - rmean[i] - rmean[j] + gm;
    }
    __syncthreads();

    // cyclic Jacobi, fixed sweeps (quadratic convergence: ~6 sweeps is
    // machine precision at m <= 64)
    for (int sweep = 0; sweep < SMEA_SWEEPS; ++sweep) {
      for (int p = 0; p < m - 1; ++p) {
        for (int q = p + 1; q < m; ++q) {
          const float apq = A[p * m + q];
          if (fabsf(apq) < 1e-12f) continue;
          const float app = A[p * m + p];
          const float aqq = A[q * m + q];
          const float tau = (aqq - app) / (2.0f * apq);
          const float t = (tau >= 0.0f ? 1.0f : -1.0f) /
                          (fabsf(tau) + sqrtf(1.0f + tau * tau));
          const float cth = rsqrtf(1.0f + t * t);
          const float sth = t * cth;
          // rows p, q (each lane owns columns k, k+64, ...)
          for (int k = lane; k < m; k += 64) {
            const float akp = A[p * m + k];
            const float akq = A[q * m + k];
            A[p * m + k] = cth * akp - sth * akq;
            A[q * m + k] = sth * akp + cth * akq;
          }
          __syncthreads();
          // columns p, q
          for (int k = lane; k < m; k += 64) {
            const float apk = A[k * m + p];
            const float aqk = A[k * m + q];
            A[k * m + p] = cth * apk - sth * aqk;
            A[k * m + q] = sth * apk + cth * aqk;
          }
          __syncthreads();
          // exact 2x2 block (reduces accumulated error)
          if (lane == 0) {
            const float d = app - aqq;
            const float app2 =
                cth * cth * app - 2.0f * sth * cth * apq + sth * sth * aqq;
            const float aqq2 =
                sth * sth * app + 2.0f * sth * cth * apq + cth * cth * aqq;
            (void)d;
            A[p * m + p] = app2;
            A[q * m + q] = aqq2;
            A[p * m + q] = 0.0f;
            A[q * m + p] = 0.0f;
          }
          __syncthreads();
        }
      }
    }
    float lam = -3.4e38f;
    for (int j = lane; j < m; j += 64) lam = fmaxf(lam, A[j * m + j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      lam = fmaxf(lam, __shfl_down(lam, off, 64));
    if (lane == 0) {
      const u64 key = ((u64)f32_key(lam) << 32) | (u32)c;
      atomicMin(best, key);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// MDA
// ---------------------------------------------------------------------------

// One workgroup (one wave) per lexicographic P-element prefix (P=2
// pairs or P=3 triples — triples cut the slowest prefix's serial DFS
// tail by ~n and put ~C(n,3) independent searchers on the chip).
// LDS: D2[n][n] + maxd[m+1][n] level stack.
// PASS 1 (FIND=false): branch-and-bound on the shared best diameter
// (strict <, so tied subsets prune instantly).
// PASS 2 (FIND=true): bounded lex-order DFS; the FIRST completion is the
// prefix's lex-smallest subset with diameter <= bound. The dispatcher
// picks the first found prefix in lex order = the globally lex-smallest
// optimal subset (host parity: mda_host.cpp mda_search's dfs2).
template <bool FIND>
__global__ void __launch_bounds__(64)
mda_dfs_kernel(const float* __restrict__ D2g, const int* __restrict__ prefixes,
               int P, int n, int m, int npre, u32* __restrict__ best,
               int* __restrict__ out_subsets, int* __restrict__ out_found) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* D2 = smem;                  // n*n
  float* maxd = smem + n * n;        // (m+1) * n level stack
  __shared__ int chosen[66];         // chosen[level] = element pushed
  __shared__ float pdiam[66];        // diameter after level pushes
  __shared__ int cand[66];           // next candidate index per level
  __shared__ int pref[4];
  const int lane = threadIdx.x;

  for (int e = lane; e < n * n; e += 64) D2[e] = D2g[e];
  __syncthreads();

  auto read_best = [&]() -> float {
    const u32 bk = *(volatile u32*)best;
    const u32 bb = (bk & 0x80000000u) ? (bk ^ 0x80000000u) : ~bk;
    return __uint_as_float(bb);
  };
  const float bound = FIND ? read_best() : 0.0f;

  for (int pi = blockIdx.x; pi < npre; pi += gridDim.x) {
    if (lane < P) pref[lane] = prefixes[(long)pi * P + lane];
    if (FIND && lane == 0) out_found[pi] = 0;
    __syncthreads();
    // prefix diameter + level-0 max-distance row
    float diam0 = 0.0f;
    for (int i = 0; i < P; ++i)
      for (int j = i + 1; j < P; ++j)
        diam0 = fmaxf(diam0, D2[pref[i] * n + pref[j]]);
    for (int k = lane; k < n; k += 64) {
      float v = D2[pref[0] * n + k];
      for (int i = 1; i < P; ++i) v = fmaxf(v, D2[pref[i] * n + k]);
      maxd[0 * n + k] = v;
    }
    __syncthreads();
    const int need = m - P;  // elements beyond the prefix
    if (need == 0) {
      if (FIND) {
        if (lane == 0 && diam0 <= bound) {
          out_found[pi] = 1;
          for (int i = 0; i < P; ++i) out_subsets[(long)pi * m + i] = pref[i];
        }
      } else if (lane == 0) {
        atomicMin(best, f32_key(diam0));
      }
      __syncthreads();
      continue;
    }
    {
      const float cb = FIND ? bound : read_best();
      const bool dead = FIND ? (diam0 > cb) : (diam0 >= cb);
      if (dead) { __syncthreads(); continue; }
    }
    pdiam[0] = diam0;
    cand[0] = pref[P - 1] + 1;
    __syncthreads();

    int depth = 0;
    bool done = false;
    while (!done && depth >= 0) {
      // fresh shared-bound read per node: staleness was measured FAR
      // more expensive than the L2 read (8-node caching exploded the
      // node count 12x — collaborative pruning needs tight bounds)
      const float cur_best = FIND ? bound : read_best();
      const int start = cand[depth];
      const int maxj = n - (need - depth - 1);
      // WAVE-PARALLEL candidate scan: n <= 64, so one ballot evaluates
      // every remaining candidate at this level at once
      const int j = start + lane;
      bool ok = false;
      float dj = 0.0f;
      if (j < maxj) {
        dj = fmaxf(pdiam[depth], maxd[depth * n + j]);
        ok = FIND ? (dj <= cur_best) : (dj < cur_best);
      }
      const unsigned long long mask = __ballot(ok);
      if (mask == 0ull) {
        --depth;  // level exhausted: backtrack
        continue;
      }
      if (depth + 1 == need) {
        if (FIND) {
          // lex-first completion = lowest ok lane
          const int sel = __ffsll((long long)mask) - 1;
          if (lane == 0) {
            out_found[pi] = 1;
            for (int i = 0; i < P; ++i)
              out_subsets[(long)pi * m + i] = pref[i];
            for (int t2 = 0; t2 < need - 1; ++t2)
              out_subsets[(long)pi * m + P + t2] = chosen[t2];
            out_subsets[(long)pi * m + P + need - 1] = start + sel;
          }
          done = true;
          break;
        }
        // pass 1: every ok lane is a completion — fold them all in one
        // wave-reduced min and exhaust the level
        float dmin = ok ? dj : 3.4e38f;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
          dmin = fminf(dmin, __shfl_down(dmin, off, 64));
        if (lane == 0) atomicMin(best, f32_key(dmin));
        __syncthreads();
        --depth;
        continue;
      }
      // push the first viable candidate
      const int sel = __ffsll((long long)mask) - 1;
      const int jsel = start + sel;
      const float djsel = fmaxf(pdiam[depth], maxd[depth * n + jsel]);
      cand[depth] = jsel + 1;
      chosen[depth] = jsel;
      pdiam[depth + 1] = djsel;
      for (int k = lane; k < n; k += 64)
        maxd[(depth + 1) * n + k] =
            fmaxf(maxd[depth * n + k], D2[jsel * n + k]);
      __syncthreads();
      cand[depth + 1] = jsel + 1;
      ++depth;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// DnC spectral selection (K15)
// ---------------------------------------------------------------------------

// One block per iteration t. The SMEA Jacobi above is one wave rotating one
// pair at a time: n (n - 1) / 2 * SMEA_SWEEPS serial rotations is ~80,000
// barrier pairs at n = 128. DnC needs only the TOP eigenvector, so this is a
// fixed-count power iteration instead: no data-dependent trip count, two
// barriers per step.
//
// Thread (r, i) keeps A[16 r .. 16 r + 15][i] of the scaled matrix
// A = Gc / max diag in registers (A is symmetric, so that column segment is
// the row segment of y_i = sum_k A[i][k] v[k]; consecutive lanes read
// consecutive words of Gc). A step is 16 FMAs per thread against v in LDS,
// then one thread per row adds its <= 8 segment partials in segment order:
// every row is summed in the same order, so identical Gram rows give
// bitwise identical scores and ties resolve by index alone.
//
// |A_ij| <= 1 and 1 <= lambda_max(A) <= n, so v grows by at most 2^7 per
// step and never loses its top component: it is renormalised every
// DNC_NORM_EVERY steps only. The start vector is e_i0, i0 the first row at
// the largest diagonal entry (the all-ones vector is A's null vector).
// score_i = u_i^2 ranks like lambda u_i^2. With the two top eigenvalues at
// ratio rho the error left is rho^DNC_POWER_STEPS: 1e-6 at rho = 0.9.

constexpr int DNC_SEL_THREADS = 1024;
constexpr int DNC_SEG = 16;  // matrix rows per thread
constexpr int DNC_MAX_SEGS = DNC_MAX_N / DNC_SEG;
constexpr int DNC_POWER_STEPS = 128;
constexpr int DNC_NORM_EVERY = 8;
static_assert(DNC_MAX_SEGS * DNC_MAX_N <= DNC_SEL_THREADS, "one thread per (segment, row)");
static_assert(DNC_POWER_STEPS % DNC_NORM_EVERY == 0, "ends normalised");

__global__ void __launch_bounds__(DNC_SEL_THREADS)
dnc_scores_kernel(const float* __restrict__ Gc3, const int* __restrict__ bad,
                  int n, int keep, int* __restrict__ kept) {
  __shared__ float v[DNC_MAX_N];
  __shared__ float part[DNC_MAX_SEGS][DNC_MAX_N];
  __shared__ float score[DNC_MAX_N];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  const float* G = Gc3 + (long)t * n * n;
  const int segs = (n + DNC_SEG - 1) / DNC_SEG;
  const int i = tid % n, r = tid / n;
  const bool active = r < segs;

  // scale and start row from the diagonal (staged in `score`)
  if (tid < DNC_MAX_N) {
    const float g = tid < n ? G[(long)tid * n + tid] : 0.0f;
    score[tid] = (g > 0.0f && g < INFINITY) ? g : 0.0f;
    v[tid] = 0.0f;
  }
  __syncthreads();
  float dmax = 0.0f;
  int i0 = 0;
  for (int k = 0; k < n; ++k)
    if (score[k] > dmax) { dmax = score[k]; i0 = k; }
  const float scale = dmax > 0.0f ? 1.0f / dmax : 0.0f;
  float a[DNC_SEG];
#pragma unroll
  for (int m = 0; m < DNC_SEG; ++m) {
    const int k = r * DNC_SEG + m;
    float x = (active && k < n) ? G[(long)k * n + i] * scale : 0.0f;
    if (!(fabsf(x) <= 2.0f)) x = 0.0f;  // a non-finite Gram entry
    a[m] = x;
  }
  __syncthreads();
  if (tid == i0) v[tid] = 1.0f;
  __syncthreads();

  for (int step = 0; step < DNC_POWER_STEPS; ++step) {
    if (active) {
      float p = 0.0f;
#pragma unroll
      for (int m = 0; m < DNC_SEG; ++m) p = fmaf(a[m], v[r * DNC_SEG + m], p);
      part[r][i] = p;
    }
    __syncthreads();
    if (tid < n) {
      float y = 0.0f;
      for (int s = 0; s < segs; ++s) y += part[s][tid];
      v[tid] = y;
    }
    __syncthreads();
    if ((step + 1) % DNC_NORM_EVERY == 0) {
      float nrm2 = 0.0f;
      for (int k = 0; k < n; ++k) nrm2 += v[k] * v[k];
      const float inv = nrm2 > 0.0f ? rsqrtf(nrm2) : 0.0f;
      __syncthreads();
      if (tid < n) v[tid] *= inv;
      __syncthreads();
    }
  }

  if (tid < n)
    score[tid] = bad[(long)t * n + tid] != 0 ? INFINITY : v[tid] * v[tid];
  __syncthreads();
  if (tid < n) {
    const float s = score[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = score[j];
      rank += (sj < s || (sj == s && j < tid)) ? 1 : 0;
    }
    kept[(long)t * n + tid] = (rank < keep && s < INFINITY) ? 1 : 0;
  }
}

// good = AND over iterations of kept_t, compacted ascending; one block.
__global__ void __launch_bounds__(DNC_MAX_N)
dnc_intersect_kernel(const int* __restrict__ kept, int niters, int n,
                     int* __restrict__ idx, int* __restrict__ count) {
  __shared__ int good[DNC_MAX_N];
  const int tid = threadIdx.x;
  if (tid < n) {
    int g = 1;
    for (int t = 0; t < niters; ++t) g &= kept[(long)t * n + tid];
    good[tid] = g;
  }
  __syncthreads();
  if (tid < n) {
    int before = 0, total = 0;
    for (int j = 0; j < n; ++j) {
      before += j < tid ? good[j] : 0;
      total += good[j];
    }
    if (good[tid]) idx[before] = tid;
    // the bad rows fill the tail in order, so every slot is written once
    else idx[total + (tid - before)] = 0;
    if (tid == 0) *count = total;
  }
}

// ---------------------------------------------------------------------------
// AFA selection (K16)
// ---------------------------------------------------------------------------

// Adaptive Federated Averaging drops, pass after pass, the rows whose cosine
// to the weighted mean g of the rows still alive is an outlier. With w masked
// to the alive rows, u = G w and q = w^T G w give
//   cos(x_i, g) = u_i / sqrt(G_ii q),
// so the whole data-dependent loop runs on the (n, n) Gram in ONE block: the
// loop ends on a block-wide "nothing removed" vote, no host in between.
//
// Thread (r, i) keeps G[i][16 r .. 16 r + 15] in registers for every pass
// (the layout of dnc_scores_kernel, read by rows: G need not be symmetric).
// A pass is 16 f64 FMAs per thread against the masked weights in LDS, then
// one thread per row adds its <= 8 segment partials in segment order; q, the
// mean and the two-pass variance are summed the same way, 16 terms per
// segment and then the segments, always in index order. u, q, the cosines
// and their statistics are f64: at n <= 128 that costs nothing, and the
// decisions then differ from an f64 evaluation of the same Gram by rounding
// of order 1e-16 only. No atomics anywhere: the same G bits give the same
// output bits.
//
// Median by rank counting, rank_i = #{alive j : s_j < s_i or (s_j == s_i and
// j < i)}: the ranks of the alive rows are a permutation of 0 .. m - 1, so
// exactly one row writes each of the two middle values.

constexpr int AFA_SEL_THREADS = 1024;
constexpr int AFA_SEG = 16;  // Gram entries of one row per thread
constexpr int AFA_MAX_SEGS = AFA_MAX_N / AFA_SEG;
static_assert(AFA_MAX_SEGS * AFA_MAX_N <= AFA_SEL_THREADS, "one thread per (segment, row)");

__global__ void __launch_bounds__(AFA_SEL_THREADS)
afa_select_kernel(const float* __restrict__ G, const float* __restrict__ w,
                  int n, double xi, double delta_xi, int* __restrict__ idx,
                  int* __restrict__ count, int* __restrict__ rounds) {
  __shared__ double part[AFA_MAX_SEGS][AFA_MAX_N];
  __shared__ double wm[AFA_MAX_N];    // w_j where j is alive, else 0
  __shared__ double diag[AFA_MAX_N];  // G_jj
  __shared__ double s[AFA_MAX_N];     // u_j, then cos(x_j, g)
  __shared__ double mid[2];           // the two middle cosines
  __shared__ double seg[2][AFA_MAX_SEGS];  // segment sums
  __shared__ int rpart[AFA_MAX_SEGS][AFA_MAX_N];  // segment rank counts
  __shared__ int alive[AFA_MAX_N];
  const int tid = threadIdx.x;
  const int segs = (n + AFA_SEG - 1) / AFA_SEG;
  const int i = tid % n, r = tid / n;
  const bool active = r < segs;
  const bool row = tid < n;  // this thread also owns row tid

  // a non-finite entry belongs to a row that starts dead; as 0 it cannot
  // turn 0 * inf into NaN in a live row's sum
  float a[AFA_SEG];
#pragma unroll
  for (int m = 0; m < AFA_SEG; ++m) {
    const int k = r * AFA_SEG + m;
    float x = (active && k < n) ? G[(long)i * n + k] : 0.0f;
    if (!(fabsf(x) < INFINITY)) x = 0.0f;
    a[m] = x;
  }
  bool ok = false;
  if (tid < AFA_MAX_N) {
    const float g = row ? G[(long)tid * n + tid] : 0.0f;
    const float wi = row ? w[tid] : 0.0f;
    ok = row && fabsf(g) < INFINITY && wi > 0.0f && wi < INFINITY;
    alive[tid] = ok ? 1 : 0;
    diag[tid] = ok ? (double)g : 0.0;
    wm[tid] = ok ? (double)wi : 0.0;
    s[tid] = 0.0;  // entries past n stay 0: whole segments are summed
  }
  int m = __syncthreads_count(ok);  // alive rows; the same in every thread

  // Nothing in a pass walks all n rows in one thread. Sums go in two levels,
  // both in a fixed order: thread t < segs adds the 16 terms of segment t,
  // then every row thread adds the <= 8 segment sums. Ranks likewise: thread
  // (r, i) counts the rows of segment r that sort before row i.
  const bool segsum = tid < segs;
  int passes = 0;
  for (int it = 0; it < n && m > 0; ++it) {
    ++passes;
    if (active) {
      double p = 0.0;
#pragma unroll
      for (int t = 0; t < AFA_SEG; ++t)
        p = fma((double)a[t], wm[r * AFA_SEG + t], p);  // wm is 0 past n
      part[r][i] = p;
    }
    __syncthreads();
    if (row) {
      double u = 0.0;
      for (int t = 0; t < segs; ++t) u += part[t][tid];
      s[tid] = u;
    }
    __syncthreads();
    if (segsum) {  // q = sum_j w_j u_j
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < AFA_SEG; ++k)
        t += wm[tid * AFA_SEG + k] * s[tid * AFA_SEG + k];
      seg[0][tid] = t;
    }
    __syncthreads();
    if (row) {
      double q = 0.0;
      for (int t = 0; t < segs; ++t) q += seg[0][t];
      const double gii = diag[tid];
      s[tid] = (alive[tid] && gii > 0.0 && q > 0.0) ? s[tid] / sqrt(gii * q)
                                                    : 0.0;
    }
    __syncthreads();
    if (segsum) {  // the cosine of a dead row is stored as 0
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < AFA_SEG; ++k) t += s[tid * AFA_SEG + k];
      seg[0][tid] = t;
    }
    __syncthreads();
    double mean = 0.0;
    if (row || segsum) {
      for (int t = 0; t < segs; ++t) mean += seg[0][t];
      mean /= (double)m;
    }
    if (segsum) {  // two-pass variance
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < AFA_SEG; ++k) {
        const double dv = s[tid * AFA_SEG + k] - mean;
        t += alive[tid * AFA_SEG + k] ? dv * dv : 0.0;
      }
      seg[1][tid] = t;
    }
    if (active) {
      const double si = s[i];
      int c = 0;
#pragma unroll
      for (int k = 0; k < AFA_SEG; ++k) {
        const int j = r * AFA_SEG + k;
        const double sj = s[j];
        c += (alive[j] && (sj < si || (sj == si && j < i))) ? 1 : 0;
      }
      rpart[r][i] = c;
    }
    __syncthreads();
    const bool mine = row && alive[tid];
    double sd = 0.0;
    if (mine) {
      for (int t = 0; t < segs; ++t) sd += seg[1][t];
      sd = sqrt(sd / (double)m);
      const double si = s[tid];
      int rank = 0;
      for (int t = 0; t < segs; ++t) rank += rpart[t][tid];
      if (rank == (m - 1) / 2) mid[0] = si;
      if (rank == m / 2) mid[1] = si;
    }
    __syncthreads();
    int rm = 0;
    if (mine) {
      const double med = 0.5 * (mid[0] + mid[1]);
      const double si = s[tid];
      rm = mean < med ? (si < med - xi * sd) : (si > med + xi * sd);
    }
    // the barrier also orders this pass's reads of alive / wm / mid before
    // the writes below, and its count is the block-wide vote
    const int removed = __syncthreads_count(rm);
    if (removed == 0) break;
    if (rm) {
      alive[tid] = 0;
      wm[tid] = 0.0;
    }
    m -= removed;
    xi += delta_xi;
    __syncthreads();
  }

  __syncthreads();
  const int n8 = (n + 7) & ~7;  // alive is 0 past n
  if (row) {
    int before = 0;
    for (int j0 = 0; j0 < n8; j0 += 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) before += j0 + k < tid ? alive[j0 + k] : 0;
    }
    if (alive[tid]) idx[before] = tid;
    // the dead rows fill the tail in order, so every slot is written once
    else idx[m + (tid - before)] = 0;
    if (tid == 0) {
      *count = m;
      *rounds = passes;
    }
  }
}

}  // namespace

void launch_afa_select(const float* G, const float* w, int n, double xi,
                       double delta_xi, int* idx, int* count, int* rounds,
                       hipStream_t stream) {
  // one thread per (segment, row) in whole waves, and at least the AFA_MAX_N
  // threads that clear the LDS vectors
  const int segs = (n + AFA_SEG - 1) / AFA_SEG;
  int threads = ((segs * n + 63) / 64) * 64;
  if (threads < AFA_MAX_N) threads = AFA_MAX_N;
  hipLaunchKernelGGL(afa_select_kernel, dim3(1), dim3(threads), 0, stream, G,
                     w, n, xi, delta_xi, idx, count, rounds);
}

void launch_dnc_select(const float* Gc, const int* bad, int niters, int n,
                       int keep, int* kept, int* idx, int* count,
                       hipStream_t stream) {
  // one thread per (segment, row), whole waves, and at least the DNC_MAX_N
  // threads that clear the LDS vectors; no idle waves at the barriers
  // (measured: no faster than a fixed 1024 at n = 64, 65 us either way)
  const int segs = (n + DNC_SEG - 1) / DNC_SEG;
  int threads = ((segs * n + 63) / 64) * 64;
  if (threads < DNC_MAX_N) threads = DNC_MAX_N;
  hipLaunchKernelGGL(dnc_scores_kernel, dim3(niters), dim3(threads), 0, stream,
                     Gc, bad, n, keep, kept);
  hipLaunchKernelGGL(dnc_intersect_kernel, dim3(1), dim3(DNC_MAX_N), 0, stream,
                     kept, niters, n, idx, count);
}

void launch_smea_select(const float* G, const int* combos, int n, int m,
                        int C, unsigned long long* best, hipStream_t stream) {
  const int grid = C < 8192 ? C : 8192;
  const size_t lds = (size_t)(m * m + m) * sizeof(float);
  hipLaunchKernelGGL(smea_select_kernel, dim3(grid), dim3(64), lds, stream, G,
                     combos, n, m, C, best);
}

void launch_mda_pass1(const float* D2, const int* prefixes, int P, int n,
                      int m, int npre, unsigned int* best,
                      hipStream_t stream) {
  const int grid = npre < 16384 ? npre : 16384;
  const size_t lds = (size_t)(n * n + (m + 1) * n) * sizeof(float);
  hipLaunchKernelGGL(mda_dfs_kernel<false>, dim3(grid), dim3(64), lds, stream,
                     D2, prefixes, P, n, m, npre, best, nullptr, nullptr);
}

void launch_mda_pass2(const float* D2, const int* prefixes, int P, int n,
                      int m, int npre, unsigned int* best, int* out_subsets,
                      int* out_found, hipStream_t stream) {
  const int grid = npre < 16384 ? npre : 16384;
  const size_t lds = (size_t)(n * n + (m + 1) * n) * sizeof(float);
  hipLaunchKernelGGL(mda_dfs_kernel<true>, dim3(grid), dim3(64), lds, stream,
                     D2, prefixes, P, n, m, npre, best, out_subsets,
                     out_found);
}
