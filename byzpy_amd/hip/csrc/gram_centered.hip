// Column-centred MFMA Gram (K22) for gfx950:
//   Gc = (X - 1 mu^T)(X - 1 mu^T)^T,  mu_j = mean of column j's finite entries.
//
// Squared distances G_ii + G_jj - 2 G_ij do not change when one vector is
// taken off every row, but their f32 cancellation error does: it is relative
// to ||x||^2 on the raw Gram and to ||x - mu||^2 on this one. Rows that share
// a large common component (parameter vectors, momenta, late gradients) are
// resolved here and are summation noise there.
//
// Design. X is read exactly once and no mu vector ever touches memory:
//   - split-K, and ONE workgroup owns ALL n rows of its K-slab, so it holds
//     every entry of each of its columns and computes that column's mean
//     locally. n <= 128 rows are 1, 2, 4 or 8 groups of 16 (template RG);
//   - a chunk is 32 KB whatever RG is (16 RG rows x 2048 / RG bytes), so 1024
//     threads stage two 16 B pieces each and two chunks double-buffer in
//     64 KB. That LDS budget would let two workgroups share a CU, but the
//     kernels hold 61 to 100 VGPRs, and past 64 only one 1024-thread
//     workgroup is resident. One LDS image, because A == B. The 16 B
//     slots of a row are XOR-swizzled by (row & 15): a 16-lane group that
//     reads one slot column of 16 rows touches 16 distinct slots, in the
//     centring sweep and in the fragment reads alike;
//   - centring sweep, in place, between the chunk's landing and its MFMAs:
//     wave w owns the slot columns w, w + 16, ...; its lanes are 16 rows x 4
//     words of that slot. A lane adds its rows (g, g + 16, ...) in order, a
//     four-step butterfly over the 16 row lanes finishes the column sum and
//     the finite count (f32 add commutes, so every lane of a column holds the
//     same bits: one mu for all rows, which is all the invariance needs),
//     and the lane writes x - mu back into the slots it read. bf16: x - mu is
//     formed in f32 and rounded once, to nearest even;
//   - MFMA phase: the 16 x 16 tiles of the upper triangle (36 at n = 128, 10
//     at n = 64), each cut into KS k-parts where tiles are few, are dealt
//     round-robin to the 16 waves. A fragment is one ds_read_b128 for both
//     dtypes: bf16 feeds v_mfma_f32_16x16x32_bf16; f32 feeds four
//     v_mfma_f32_16x16x4_f32 with the slot's four floats (the k index is a
//     summation index, so any assignment of k to lanes that A and B share
//     is right). Diagonal tiles read one fragment;
//   - the loop has two barriers per chunk, as the uncentred LDS kernels: the
//     next chunk's registers go to the free buffer and the loads of the one
//     after are issued before the MFMAs, the sweep runs after them.
//   - combine: f32 atomics of the upper triangle into the caller-zeroed Gc,
//     then a mirror launch, so Gc is symmetric bit for bit.
//
// Finite rule: mu_j is the mean over the finite entries of column j (0 if
// there are none); inf - mu and NaN - mu stay non-finite. A row that holds
// inf or NaN therefore gets a non-finite Gc_ii and row / column of Gc, and
// no other entry changes: entry (i, j) reads rows i and j only.
//
// Ragged ends: rows n .. 16 ceil(n / 16) - 1 are loaded from row n - 1
// (clamped) and selected out of the sums; their outputs are never written.
// Row groups past that are neither staged nor read. Columns past the slab's
// end are staged as zeros in every row: mean 0, centred value 0. A d or a
// base pointer that breaks 16 B row alignment takes element loads.
#include "common.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

namespace {

constexpr int GC_THREADS = 1024;
constexpr int GC_WAVES = GC_THREADS / 64;

// raw bits of one element, in the low bits of a word
DEV unsigned int elem_bits(const float* p) { return __float_as_uint(*p); }
DEV unsigned int elem_bits(const __hip_bfloat16* p) {
  return *reinterpret_cast<const unsigned short*>(p);
}

DEV bool finite_bits(unsigned int f32_bits) {
  return (f32_bits & 0x7f800000u) != 0x7f800000u;
}

// f32 -> bf16 bits, round to nearest even; NaN stays NaN
DEV unsigned int bf16_round_bits(float v) {
  const unsigned int u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <typename T, int RG>
__global__ void __launch_bounds__(GC_THREADS)
gram_centered_kernel(const T* __restrict__ X, float* __restrict__ G, int n,
                     long d, long k_per_block, int vec) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int EPS = 16 / sizeof(T);                   // elements per slot
  constexpr int SLOTS = GRAM_CENTERED_CHUNK_BYTES / (16 * 16 * RG);
  constexpr int ROWB = SLOTS * 16;                      // bytes per LDS row
  constexpr int BK = SLOTS * EPS;                       // columns per chunk
  constexpr int NSTEPS = SLOTS / 4;   // fragment steps per chunk (4 slots)
  // k-parts per tile and work items per wave: 36 tiles at RG = 8, <= 20
  // items at RG = 4, 12 at RG = 2, 16 at RG = 1
  constexpr int KS = RG == 8 ? 1 : (RG == 4 ? 2 : (RG == 2 ? 4 : 16));
  constexpr int MAXI = RG == 8 ? 3 : (RG == 4 ? 2 : 1);
  constexpr int SPK = NSTEPS / KS;
  constexpr int NACC = BF ? 1 : 2;  // f32: two chains of dependent MFMAs
  static_assert(SLOTS >= 16 && SPK >= 1, "chunk geometry");

  __shared__ __attribute__((aligned(16))) char smem[2 * GRAM_CENTERED_CHUNK_BYTES];
  char* const buf0 = smem;
  char* const buf1 = smem + GRAM_CENTERED_CHUNK_BYTES;

  const int t = threadIdx.x;
  const int wave = t >> 6;
  const int lane = t & 63;
  const int ng = (n + 15) >> 4;  // row groups in use
  const int n16 = ng << 4;

  const long k_lo = (long)blockIdx.x * k_per_block;
  const long k_hi = min(d, k_lo + k_per_block);
  const long nchunks = (k_hi - k_lo + BK - 1) / BK;

  // -- staging: piece p = t + 1024 u is LDS row p / SLOTS, physical slot
  // p % SLOTS, whose content is global slot (physical ^ (row & 15))
  int st_row[2], st_off[2];
  long st_col[2];
  const T* st_src[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int p = t + u * GC_THREADS;
    st_row[u] = p / SLOTS;
    const int ps = p % SLOTS;
    st_off[u] = st_row[u] * ROWB + ps * 16;
    st_col[u] = (long)(ps ^ (st_row[u] & 15)) * EPS;
    st_src[u] = X + (long)min(st_row[u], n - 1) * d;
  }
  u32x4 rg[2];
  auto stage_load = [&](long c) {
    const long k0 = k_lo + c * BK;
    const bool full = vec && (k0 + BK <= k_hi);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (st_row[u] >= n16) continue;
      const long off = k0 + st_col[u];
      if (full) {
        rg[u] = *reinterpret_cast<const u32x4*>(st_src[u] + off);
      } else {
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < EPS; ++j) {
          const unsigned int b =
              (off + j < k_hi) ? elem_bits(st_src[u] + off + j) : 0u;
          if (BF) v[j >> 1] |= b << (16 * (j & 1));
          else v[j] = b;
        }
        rg[u] = v;
      }
    }
  };
  auto stage_write = [&](char* buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (st_row[u] < n16) *reinterpret_cast<u32x4*>(buf + st_off[u]) = rg[u];
  };

  // -- centring sweep: lane = (row lane g, word cw) of the wave's slot column
  const int g = lane >> 2;
  const int cw = lane & 3;
  auto sweep = [&](char* buf) {
#pragma unroll
    for (int js = 0; js < SLOTS / 16; ++js) {
      const int s = wave + 16 * js;
      char* const col = buf + g * ROWB + ((s ^ g) * 16) + cw * 4;
      unsigned int w[RG];
      float s0 = 0.0f, s1 = 0.0f;
      int cnt = 0;  // bf16: the two columns' counts in the two halves
#pragma unroll
      for (int i = 0; i < RG; ++i) {
        if (i >= ng) continue;
        w[i] = *reinterpret_cast<const unsigned int*>(col + i * 16 * ROWB);
        const bool in = i * 16 + g < n;
        if (BF) {
          const unsigned int lo = w[i] << 16, hi = w[i] & 0xffff0000u;
          const bool ok0 = in && finite_bits(lo), ok1 = in && finite_bits(hi);
          s0 += ok0 ? __uint_as_float(lo) : 0.0f;
          s1 += ok1 ? __uint_as_float(hi) : 0.0f;
          cnt += (ok0 ? 1 : 0) + (ok1 ? 0x10000 : 0);
        } else {
          const bool ok0 = in && finite_bits(w[i]);
          s0 += ok0 ? __uint_as_float(w[i]) : 0.0f;
          cnt += ok0 ? 1 : 0;
        }
      }
#pragma unroll
      for (int m = 4; m < 64; m <<= 1) {
        s0 += __shfl_xor(s0, m, 64);
        if (BF) s1 += __shfl_xor(s1, m, 64);
        cnt += __shfl_xor(cnt, m, 64);
      }
      const int c0 = cnt & 0xffff, c1 = cnt >> 16;
      const float mu0 = c0 > 0 ? s0 / (float)c0 : 0.0f;
      const float mu1 = c1 > 0 ? s1 / (float)c1 : 0.0f;
#pragma unroll
      for (int i = 0; i < RG; ++i) {
        if (i >= ng) continue;
        unsigned int out;
        if (BF) {
          const float y0 = __uint_as_float(w[i] << 16) - mu0;
          const float y1 = __uint_as_float(w[i] & 0xffff0000u) - mu1;
          out = bf16_round_bits(y0) | (bf16_round_bits(y1) << 16);
        } else {
          out = __float_as_uint(__uint_as_float(w[i]) - mu0);
        }
        *reinterpret_cast<unsigned int*>(col + i * 16 * ROWB) = out;
      }
    }
  };

  // -- MFMA work items of this wave: item = tile + NT * k-part
  const int NT = ng * (ng + 1) / 2;  // upper-triangle tiles
  const int fr = lane & 15;   // fragment row within its group
  const int grp = lane >> 4;  // slot within a fragment step
  int it_a[MAXI], it_b[MAXI], it_k[MAXI];
  bool it_on[MAXI];
  f32x4 acc[MAXI][NACC];
#pragma unroll
  for (int m = 0; m < MAXI; ++m) {
    const int item = wave + GC_WAVES * m;
    it_on[m] = item < NT * KS;
    int rem = it_on[m] ? item % NT : 0, ti = 0, len = ng;
    while (rem >= len) { rem -= len; ++ti; --len; }
    it_a[m] = ti;
    it_b[m] = ti + rem;
    it_k[m] = it_on[m] ? item / NT : 0;
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[m][a] = {0.0f, 0.0f, 0.0f, 0.0f};
  }
  auto compute = [&](const char* buf) {
#pragma unroll
    for (int m = 0; m < MAXI; ++m) {
      if (!it_on[m]) continue;
      const char* const A = buf + (it_a[m] * 16 + fr) * ROWB;
      const char* const B = buf + (it_b[m] * 16 + fr) * ROWB;
      const bool diag = it_a[m] == it_b[m];
#pragma unroll
      for (int st = 0; st < SPK; ++st) {
        const int q = (((it_k[m] * SPK + st) * 4 + grp) ^ fr) * 16;
        const u32x4 a = *reinterpret_cast<const u32x4*>(A + q);
        u32x4 b = a;
        if (!diag) b = *reinterpret_cast<const u32x4*>(B + q);
        if (BF) {
          acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
              acc[m][0], 0, 0, 0);
        } else {
          const f32x4 af = __builtin_bit_cast(f32x4, a);
          const f32x4 bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[m][j & (NACC - 1)] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                af[j], bf[j], acc[m][j & (NACC - 1)], 0, 0, 0);
        }
      }
    }
  };

  stage_load(0);
  stage_write(buf0);
  if (nchunks > 1) stage_load(1);
  __syncthreads();
  sweep(buf0);
  __syncthreads();
  for (long c = 0; c < nchunks; ++c) {
    char* const cur = (c & 1) ? buf1 : buf0;
    char* const nxt = (c & 1) ? buf0 : buf1;
    const bool more = c + 1 < nchunks;
    if (more) {
      stage_write(nxt);  // free since the barrier after compute(c - 1)
      if (c + 2 < nchunks) stage_load(c + 2);
    }
    compute(cur);
    __syncthreads();
    if (more) {
      sweep(nxt);
      __syncthreads();
    }
  }

  // C/D map for 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg. Upper
  // triangle only: the mirror launch copies it down.
#pragma unroll
  for (int m = 0; m < MAXI; ++m) {
    if (!it_on[m]) continue;
    const int out_col = it_b[m] * 16 + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out_row = it_a[m] * 16 + grp * 4 + r;
      float v = acc[m][0][r];
      if (NACC == 2) v += acc[m][NACC - 1][r];
      if (out_row <= out_col && out_col < n)
        atomicAdd(&G[(long)out_row * n + out_col], v);
    }
  }
}

__global__ void __launch_bounds__(GC_THREADS)
gram_centered_mirror_kernel(float* __restrict__ G, int n) {
  for (int e = threadIdx.x; e < n * n; e += GC_THREADS) {
    const int i = e / n, j = e - i * n;
    if (i > j) G[e] = G[j * n + i];
  }
}

}  // namespace

template <typename T>
void launch_gram_centered(const T* X, float* Gc, int n, long d,
                          hipStream_t stream) {
  int rg;
  long blocks, kpb;
  gram_centered_geometry(n, d, (int)sizeof(T), rg, blocks, kpb);
  constexpr long EPS = 16 / sizeof(T);
  const int vec =
      (d % EPS) == 0 && reinterpret_cast<unsigned long>(X) % 16 == 0;
#define GC_LAUNCH(RG)                                                        \
  hipLaunchKernelGGL((gram_centered_kernel<T, RG>), dim3((unsigned)blocks),  \
                     dim3(GC_THREADS), 0, stream, X, Gc, n, d, kpb, vec)
  if (rg == 1) GC_LAUNCH(1);
  else if (rg == 2) GC_LAUNCH(2);
  else if (rg == 4) GC_LAUNCH(4);
  else GC_LAUNCH(8);
#undef GC_LAUNCH
  hipLaunchKernelGGL(gram_centered_mirror_kernel, dim3(1), dim3(GC_THREADS), 0,
                     stream, Gc, n);
}
INSTANTIATE_LAUNCHER(launch_gram_centered)
