// Fused Krum selection: Gram (n,n) -> q winner indices.
//
// One workgroup (16 waves). Phase 1: wave w handles rows w, w+16, ...;
// for each row it materializes the squared-distance row
// D2[i][j] = G[i][i] + G[j][j] - 2 G[i][j]  (diag -> +inf), sorts it in
// its private LDS slab with a wave-synchronous bitonic (lanes of one wave
// are lockstep; no block barrier needed inside a row), and sums the
// n-f-1 smallest into scores[i]. Phase 2: one wave selects the q smallest
// scores by repeated masked min. Replaces ~8 small torch launches of
// <=0.1 ms each — fixed overhead that caps multi-GPU scaling of the
// d-sharded Krum (the (n,n) work is rank-replicated).
#include "common.h"
#include "launchers.h"

namespace {

constexpr int WAVES_K = 16;
constexpr int MAX_N = 512;
constexpr float INF = 3.0e38f;

__global__ void __launch_bounds__(WAVES_K * 64)
krum_select_kernel(const float* __restrict__ G, int n, int f, int q,
                   int* __restrict__ out_idx, float* __restrict__ out_scores) {
  __shared__ float rowbuf[WAVES_K][MAX_N];
  __shared__ float scores[MAX_N];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  int P2 = 1;
  while (P2 < n) P2 <<= 1;

  const int k = n - f - 1;  // distances summed per row
  for (int row = wave; row < n; row += WAVES_K) {
    float* buf = rowbuf[wave];
    const float gii = G[(long)row * n + row];
    for (int j = lane; j < P2; j += 64) {
      float v;
      if (j >= n || j == row) {
        v = INF;
      } else {
        const float d2 =
            gii + G[(long)j * n + j] - 2.0f * G[(long)row * n + j];
        // adversarial rows produce inf/NaN distances (inf - inf in the
        // Gram identity); NaN breaks the min/max sort's total order, so
        // clamp every non-finite distance to +inf — it then sorts last
        // and never enters a k-smallest sum that has finite candidates
        v = isfinite(d2) ? fmaxf(d2, 0.0f) : INF;
      }
      buf[j] = v;
    }
    // wave-synchronous bitonic sort of buf[0..P2)
    for (int kk = 2; kk <= P2; kk <<= 1) {
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        for (int i = lane; i < P2; i += 64) {
          const int l = i ^ jj;
          if (l > i) {
            const bool asc = (i & kk) == 0;
            const float a = buf[i], b = buf[l];
            const float lo = fminf(a, b), hi = fmaxf(a, b);
            buf[i] = asc ? lo : hi;
            buf[l] = asc ? hi : lo;
          }
        }
        // lanes of one wave run in lockstep; LDS within the wave is
        // ordered by program order — no barrier needed
      }
    }
    float acc = 0.0f;
    for (int i = lane; i < k; i += 64) acc += buf[i];
    acc = wave_reduce_sum(acc);
    if (lane == 0) scores[row] = acc;
  }
  __syncthreads();

  // phase 2: q smallest scores (first wave only), ties -> smallest index
  if (wave == 0) {
    for (int pick = 0; pick < q; ++pick) {
      float best = INF;
      int best_i = -1;
      for (int i = lane; i < n; i += 64) {
        const float s = scores[i];
        if (s < best || (s == best && i < best_i)) { best = s; best_i = i; }
      }
      // wave reduce (value, index) preferring smaller value then index
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(best, off, 64);
        const int oi = __shfl_down(best_i, off, 64);
        if (ov < best || (ov == best && oi != -1 && (best_i == -1 || oi < best_i))) {
          best = ov;
          best_i = oi;
        }
      }
      best_i = __shfl(best_i, 0, 64);
      if (lane == 0) {
        out_idx[pick] = best_i;
        if (out_scores != nullptr) out_scores[pick] = best;
        scores[best_i] = INF;  // mask out
      }
      // lane 0's LDS write is visible to the wave (lockstep)
    }
  }
}

// ---------------------------------------------------------------------------
// Iterative selection (Bulyan): q picks, each the best Krum score among the
// rows still alive, scored against alive rows only; the pick then dies.
//
// Re-sorting every alive row per pick would cost q full bitonic sorts per
// row. Instead each distance row is sorted ONCE, carrying the column index
// as payload, and kept in LDS; a pick then only rescans: the k smallest
// alive distances of row i are the first k entries of its sorted list whose
// payload is alive (and is not i), found per 64-entry chunk with one
// ballot + prefix popcount. Per pick that is n/16 rows x (n/64 chunks) per
// wave plus one masked argmin — the 34 picks of n = 64, f = 15 cost less
// than the one-off sort.
//
// LDS: n x n f32 keys + n x n u8 payloads = 80 KB at the n = 128 cap
// (KRUM_ITER_MAX_N, launchers.h); an (n, n) f32 matrix alone would not fit
// the 160 KB workgroup limit at n = 256 with its payload, let alone 512.
// Non-finite distances count as +inf (a real inf here: the sort is a
// compare-and-swap, not min/max, so it needs no finite sentinel), and a
// pick among all-inf scores is the smallest alive index.
// ---------------------------------------------------------------------------

constexpr int ITER_N = KRUM_ITER_MAX_N;

// The selection itself, written once for the Bulyan kernel below and for the
// tailored-attack evaluator further down: `dist(row, j)` is the squared
// distance of two different rows (any non-finite value counts as +inf), the
// four arrays are the caller's LDS, out_idx (global or LDS) receives the q
// picks. Called by all WAVES_K * 64 threads; ends on a block barrier.
template <typename Dist>
DEV void krum_iter_select(float (*skey)[ITER_N], unsigned char (*sidx)[ITER_N],
                          float* scores, int* alive, int n, int f, int q,
                          Dist dist, int* out_idx) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const float inf = __builtin_huge_valf();
  int P2 = 1;
  while (P2 < n) P2 <<= 1;

  for (int i = threadIdx.x; i < ITER_N; i += WAVES_K * 64)
    alive[i] = i < n ? 1 : 0;

  // phase 1: sort every distance row once, index payload alongside
  for (int row = wave; row < n; row += WAVES_K) {
    float* key = skey[row];
    unsigned char* idx = sidx[row];
    for (int j = lane; j < P2; j += 64) {
      float v = inf;  // self and pad columns: never counted (see phase 2)
      if (j < n && j != row) {
        const float d2 = dist(row, j);
        v = isfinite(d2) ? fmaxf(d2, 0.0f) : inf;
      }
      key[j] = v;
      idx[j] = (unsigned char)j;
    }
    for (int kk = 2; kk <= P2; kk <<= 1) {
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        // substeps exchange data between lanes through LDS: keep the
        // compiler from moving one substep's accesses across the next's
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < P2; i += 64) {
          const int l = i ^ jj;
          if (l > i) {
            const bool asc = (i & kk) == 0;
            const float a = key[i], b = key[l];
            if (asc ? (a > b) : (a < b)) {
              key[i] = b;
              key[l] = a;
              const unsigned char t = idx[i];
              idx[i] = idx[l];
              idx[l] = t;
            }
          }
        }
      }
    }
  }
  __syncthreads();

  // phase 2: the picks
  for (int pick = 0; pick < q; ++pick) {
    const int k = n - pick - f - 1;  // alive - f - 1 >= 1 (host-checked)
    for (int row = wave; row < n; row += WAVES_K) {
      if (!alive[row]) continue;  // wave-uniform
      float acc = 0.0f;
      int taken = 0;
      for (int base = 0; base < P2 && taken < k; base += 64) {
        const int t = base + lane;
        bool ok = false;
        float v = 0.0f;
        if (t < P2) {
          const int j = sidx[row][t];
          ok = j != row && alive[j] != 0;  // pad columns are never alive
          v = skey[row][t];
        }
        const unsigned long long m = __ballot(ok);
        const int before = taken + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && before < k) acc += v;
        taken += __popcll(m);
      }
      acc = wave_reduce_sum(acc);
      if (lane == 0) scores[row] = acc;
    }
    __syncthreads();
    if (wave == 0) {
      // smallest score among alive rows, ties -> smallest index
      float best = inf;
      int best_i = 0x7fffffff;
      for (int i = lane; i < n; i += 64) {
        if (!alive[i]) continue;
        const float s = scores[i];
        if (s < best || (s == best && i < best_i)) { best = s; best_i = i; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(best, off, 64);
        const int oi = __shfl_down(best_i, off, 64);
        if (ov < best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
      }
      if (lane == 0) {
        out_idx[pick] = best_i;
        alive[best_i] = 0;
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(WAVES_K * 64)
krum_select_iter_kernel(const float* __restrict__ G, int n, int f, int q,
                        int* __restrict__ out_idx) {
  __shared__ float skey[ITER_N][ITER_N];
  __shared__ unsigned char sidx[ITER_N][ITER_N];
  __shared__ float scores[ITER_N];
  __shared__ int alive[ITER_N];
  krum_iter_select(
      skey, sidx, scores, alive, n, f, q,
      [=](int row, int j) {
        return G[(long)row * n + row] + G[(long)j * n + j] -
               2.0f * G[(long)row * n + j];
      },
      out_idx);
}

// ---------------------------------------------------------------------------
// Aggregator-tailored attack search (K14): which trial gamma still gets the
// f copies of m(gamma) = mu + gamma p selected by Krum / Multi-Krum / Bulyan
// run on the n honest rows followed by those copies. Everything is O(n^2):
// honest-honest distances come off the honest Gram, honest-malicious ones
// are e_i(gamma) = max(a_i + 2 gamma b_i + gamma^2 c, 0) from the Min-Max
// statistics, malicious-malicious ones are 0.
//
// One workgroup per trial gamma, so one launch tests a whole grid. A search
// is three grid launches and a one-wave finish: a geometric grid (gamma = 0,
// then gamma0 2^-20 .. gamma0 2^20, gamma0 = sqrt(max a / c)), then two
// linear grids of AGR_LIN_POINTS interior points inside the gap below the
// first infeasible point of the grid before. Each launch re-derives that
// gap from the previous launch's flags (every wave on its own, from global
// memory the previous launch wrote), so no launch reads what a sibling
// block writes and nothing returns to the host. Every loop's trip count is
// fixed by n, f and the grid sizes; non-finite statistics make every point
// infeasible (gamma = 0) instead of steering a loop.
// ---------------------------------------------------------------------------

enum { AGR_LIST = 0, AGR_GEO = 1, AGR_LIN = 2 };

// Grid point k of a grid of B points. Geometric: s0 = gamma0. Linear: the
// B interior points that cut (s0, s1) into B + 1 equal gaps.
DEV float agr_point(int kind, int k, int B, float s0, float s1) {
  if (kind == AGR_GEO) return k == 0 ? 0.0f : ldexpf(s0, k - 21);
  return s0 + (s1 - s0) * ((float)(k + 1) / (float)(B + 1));
}

// The gap below the first infeasible point of the previous grid: [lo, hi]
// with lo feasible (or 0). Wave-uniform; every wave computes it for itself.
DEV void agr_resolve(int kind, const float* __restrict__ state,
                     const int* __restrict__ flags, int B, float& lo,
                     float& hi) {
  const int lane = threadIdx.x & 63;
  int j = B;
  for (int base = 0; base < B; base += 64) {
    const int t = base + lane;
    const bool no = t < B && flags[t] == 0;
    const unsigned long long m = __ballot(no);
    if (m != 0ull && j == B) j = base + __ffsll((long long)m) - 1;
  }
  const float s0 = state[0], s1 = state[1];
  if (kind == AGR_GEO) {
    // gamma = 0 infeasible, or the whole range infeasible: 0. Nothing
    // infeasible: the top of the range.
    if (j <= 1) {
      lo = hi = 0.0f;
    } else if (j == B) {
      lo = hi = agr_point(kind, B - 1, B, s0, s1);
    } else {
      lo = agr_point(kind, j - 1, B, s0, s1);
      hi = agr_point(kind, j, B, s0, s1);
    }
    return;
  }
  lo = j == 0 ? s0 : agr_point(kind, j - 1, B, s0, s1);
  hi = j == B ? s1 : agr_point(kind, j, B, s0, s1);
}

// This block's trial gamma. Block 0 records what the next launch needs to
// rebuild this grid: (gamma0, 0) for the geometric one, (lo, hi) for a
// linear one.
DEV float agr_trial_gamma(int kind, const float* __restrict__ gammas,
                          const float* __restrict__ stats, int n,
                          int prev_kind, const float* __restrict__ prev_state,
                          const int* __restrict__ prev_flags, int prev_B,
                          float* __restrict__ cur_state) {
  if (kind == AGR_LIST) return gammas[blockIdx.x];
  const int lane = threadIdx.x & 63;
  float s0, s1;
  if (kind == AGR_GEO) {
    float amax = 0.0f;
    for (int i = lane; i < n; i += 64) amax = fmaxf(amax, stats[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    const float c = stats[2 * n];
    s0 = c > 0.0f ? sqrtf(amax / c) : 0.0f;
    s1 = 0.0f;
  } else {
    agr_resolve(prev_kind, prev_state, prev_flags, prev_B, s0, s1);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cur_state[0] = s0;
    cur_state[1] = s1;
  }
  return agr_point(kind, (int)blockIdx.x, (int)gridDim.x, s0, s1);
}

// e_i(gamma) into e[0..n); returns (block-uniform) whether gamma or any
// statistic is non-finite. Ends on a block barrier.
DEV bool agr_fill_e(const float* __restrict__ stats, int n, float gamma,
                    float* e) {
  const float inf = __builtin_huge_valf();
  const float c = stats[2 * n];
  int bad = !isfinite(gamma) || !isfinite(c);
  for (int i = threadIdx.x; i < n; i += WAVES_K * 64) {
    const float a = stats[i], b = stats[n + i];
    bad |= !isfinite(a) || !isfinite(b);
    const float v = a + 2.0f * gamma * b + gamma * gamma * c;
    e[i] = isfinite(v) ? fmaxf(v, 0.0f) : inf;
  }
  return __syncthreads_or(bad) != 0;
}

// Wave-synchronous ascending bitonic sort of key[0..P2), P2 a power of two.
DEV void wave_sort(float* key, int P2) {
  const int lane = threadIdx.x & 63;
  for (int kk = 2; kk <= P2; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      __builtin_amdgcn_wave_barrier();  // as in krum_iter_select
      for (int i = lane; i < P2; i += 64) {
        const int l = i ^ jj;
        if (l > i) {
          const bool asc = (i & kk) == 0;
          const float a = key[i], b = key[l];
          if (asc ? (a > b) : (a < b)) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// Krum / Multi-Krum with q winners on N = n + f rows, parameter f: every
// score sums the n - 1 smallest distances to the other rows. An honest
// row's candidates are its n - 1 honest distances and f copies of e_i: with
// the honest ones sorted and cnt of them below e_i, the sum takes
// kD = max(cnt, n - 1 - f) honest distances and n - 1 - kD copies of e_i.
// A malicious row's are f - 1 zeros and the n - f smallest of e. Feasible
// iff at most max(q - f, 0) honest rows score no worse than a malicious
// one (an honest row wins a tie; a NaN score counts against the attack).
__global__ void __launch_bounds__(WAVES_K * 64)
agr_krum_kernel(const float* __restrict__ G, const float* __restrict__ stats,
                int n, int f, int q, int kind,
                const float* __restrict__ gammas, int prev_kind,
                const float* __restrict__ prev_state,
                const int* __restrict__ prev_flags, int prev_B,
                float* __restrict__ cur_state, int* __restrict__ flags) {
  __shared__ float rowbuf[WAVES_K][ITER_N];
  __shared__ float scores[ITER_N];
  __shared__ float e[ITER_N];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const float inf = __builtin_huge_valf();
  int P2 = 1;
  while (P2 < n) P2 <<= 1;

  const float gamma = agr_trial_gamma(kind, gammas, stats, n, prev_kind,
                                      prev_state, prev_flags, prev_B,
                                      cur_state);
  const bool bad = agr_fill_e(stats, n, gamma, e);

  float* buf = rowbuf[wave];
  for (int row = wave; row < n; row += WAVES_K) {
    __builtin_amdgcn_wave_barrier();  // the previous row's reads of buf
    const float gii = G[(long)row * n + row];
    for (int j = lane; j < P2; j += 64) {
      float v = inf;  // self and pad columns sort last
      if (j < n && j != row) {
        const float d2 =
            gii + G[(long)j * n + j] - 2.0f * G[(long)row * n + j];
        v = isfinite(d2) ? fmaxf(d2, 0.0f) : inf;
      }
      buf[j] = v;
    }
    wave_sort(buf, P2);
    const float ei = e[row];
    int cnt = 0;
    for (int base = 0; base < P2; base += 64) {
      const int t = base + lane;
      cnt += __popcll(__ballot(t < P2 && buf[t] < ei));
    }
    const int kD = min(max(cnt, n - 1 - f), n - 1);
    float acc = 0.0f;
    for (int t = lane; t < kD; t += 64) acc += buf[t];
    acc = wave_reduce_sum(acc);
    if (lane == 0)
      scores[row] = kD < n - 1 ? acc + (float)(n - 1 - kD) * ei : acc;
  }
  __syncthreads();  // every wave is done with its slab and with e

  if (wave == 0) {
    for (int j = lane; j < P2; j += 64) buf[j] = j < n ? e[j] : inf;
    wave_sort(buf, P2);
    float acc = 0.0f;
    for (int t = lane; t < n - f; t += 64) acc += buf[t];
    acc = wave_reduce_sum(acc);
    const float sm = __shfl(acc, 0, 64);
    int beaten = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      beaten += __popcll(__ballot(i < n && !(scores[i] > sm)));
    }
    if (lane == 0)
      flags[blockIdx.x] = (!bad && beaten <= max(q - f, 0)) ? 1 : 0;
  }
}

// Bulyan on the N = n + f rows, parameter f: the augmented distances feed
// the shared pick loop; feasible iff all f malicious rows (indices >= n) are
// among the N - 2f picks.
__global__ void __launch_bounds__(WAVES_K * 64)
agr_bulyan_kernel(const float* __restrict__ G, const float* __restrict__ stats,
                  int n, int f, int kind, const float* __restrict__ gammas,
                  int prev_kind, const float* __restrict__ prev_state,
                  const int* __restrict__ prev_flags, int prev_B,
                  float* __restrict__ cur_state, int* __restrict__ flags) {
  __shared__ float skey[ITER_N][ITER_N];
  __shared__ unsigned char sidx[ITER_N][ITER_N];
  __shared__ float scores[ITER_N];
  __shared__ int alive[ITER_N];
  __shared__ float e[ITER_N];
  __shared__ int picks[ITER_N];
  const int N = n + f;
  const int theta = N - 2 * f;

  const float gamma = agr_trial_gamma(kind, gammas, stats, n, prev_kind,
                                      prev_state, prev_flags, prev_B,
                                      cur_state);
  const bool bad = agr_fill_e(stats, n, gamma, e);
  const float* ev = e;
  krum_iter_select(
      skey, sidx, scores, alive, N, f, theta,
      [=](int row, int j) {
        if (row >= n) return j >= n ? 0.0f : ev[j];
        if (j >= n) return ev[row];
        return G[(long)row * n + row] + G[(long)j * n + j] -
               2.0f * G[(long)row * n + j];
      },
      picks);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int mal = 0;
    for (int base = 0; base < theta; base += 64) {
      const int t = base + lane;
      mal += __popcll(__ballot(t < theta && picks[t] >= n));
    }
    if (lane == 0) flags[blockIdx.x] = (!bad && mal == f) ? 1 : 0;
  }
}

// The end of a search: the feasible end of the last gap.
__global__ void __launch_bounds__(64)
agr_finish_kernel(int prev_kind, const float* __restrict__ prev_state,
                  const int* __restrict__ prev_flags, int prev_B,
                  float* __restrict__ gamma_out) {
  float lo, hi;
  agr_resolve(prev_kind, prev_state, prev_flags, prev_B, lo, hi);
  if (threadIdx.x == 0) gamma_out[0] = lo;
}

void agr_launch(const float* G, const float* stats, int n, int f, int q,
                int rule, int kind, const float* gammas, int B, int prev_kind,
                const float* prev_state, const int* prev_flags, int prev_B,
                float* cur_state, int* flags, hipStream_t stream) {
  if (rule == AGR_RULE_BULYAN)
    hipLaunchKernelGGL(agr_bulyan_kernel, dim3(B), dim3(WAVES_K * 64), 0,
                       stream, G, stats, n, f, kind, gammas, prev_kind,
                       prev_state, prev_flags, prev_B, cur_state, flags);
  else
    hipLaunchKernelGGL(agr_krum_kernel, dim3(B), dim3(WAVES_K * 64), 0, stream,
                       G, stats, n, f, q, kind, gammas, prev_kind, prev_state,
                       prev_flags, prev_B, cur_state, flags);
}

}  // namespace

void launch_agr_flags(const float* G, const float* stats, int n, int f, int q,
                      int rule, const float* gammas, int B, int* flags,
                      hipStream_t stream) {
  agr_launch(G, stats, n, f, q, rule, AGR_LIST, gammas, B, AGR_LIST, nullptr,
             nullptr, 0, nullptr, flags, stream);
}

void launch_agr_search(const float* G, const float* stats, int n, int f, int q,
                       int rule, float* state, int* flags, float* gamma_out,
                       hipStream_t stream) {
  constexpr int BG = AGR_GEO_POINTS, BL = AGR_LIN_POINTS;
  int* f1 = flags;
  int* f2 = flags + BG;
  int* f3 = flags + BG + BL;
  agr_launch(G, stats, n, f, q, rule, AGR_GEO, nullptr, BG, AGR_LIST, nullptr,
             nullptr, 0, state, f1, stream);
  agr_launch(G, stats, n, f, q, rule, AGR_LIN, nullptr, BL, AGR_GEO, state, f1,
             BG, state + 2, f2, stream);
  agr_launch(G, stats, n, f, q, rule, AGR_LIN, nullptr, BL, AGR_LIN, state + 2,
             f2, BL, state + 4, f3, stream);
  hipLaunchKernelGGL(agr_finish_kernel, dim3(1), dim3(64), 0, stream, AGR_LIN,
                     state + 4, f3, BL, gamma_out);
}

void launch_krum_select_iter(const float* G, int n, int f, int q,
                             int* out_idx, hipStream_t stream) {
  hipLaunchKernelGGL(krum_select_iter_kernel, dim3(1), dim3(WAVES_K * 64), 0,
                     stream, G, n, f, q, out_idx);
}

void launch_krum_select(const float* G, int n, int f, int q, int* out_idx,
                        float* out_scores, hipStream_t stream) {
  hipLaunchKernelGGL(krum_select_kernel, dim3(1), dim3(WAVES_K * 64), 0,
                     stream, G, n, f, q, out_idx, out_scores);
}
