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

__global__ void __launch_bounds__(WAVES_K * 64)
krum_select_iter_kernel(const float* __restrict__ G, int n, int f, int q,
                        int* __restrict__ out_idx) {
  __shared__ float skey[ITER_N][ITER_N];
  __shared__ unsigned char sidx[ITER_N][ITER_N];
  __shared__ float scores[ITER_N];
  __shared__ int alive[ITER_N];
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
    const float gii = G[(long)row * n + row];
    for (int j = lane; j < P2; j += 64) {
      float v = inf;  // self and pad columns: never counted (see phase 2)
      if (j < n && j != row) {
        const float d2 =
            gii + G[(long)j * n + j] - 2.0f * G[(long)row * n + j];
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

}  // namespace

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
