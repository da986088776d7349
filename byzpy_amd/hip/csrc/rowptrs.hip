// Kernels over n <= 64 rows that live in n separate device vectors (K19):
// the Gram G = X X^T, the mean of selected rows and the coefficient combine
// sum_i a_i x_i (K20; the same kernel text also serves a contiguous matrix of
// n <= 128 rows). The column-selection kernels of this layout are ROWS_PTRS
// instantiations in colsel.hip. The
// rows are named by a table of pointers passed BY VALUE as a kernel argument
// (RowPtrTable, 512 B), so nothing is stacked, nothing is allocated and
// nothing is copied to the device before the launch. Built without
// v_pk_add/mul/fma_f32, like colsel_mix.hip (hip/build.py).
//
// Gram.
// One 64 x 64 output tile, split-K across the grid. A workgroup (8 waves)
// walks its share of K in chunks of 1 KB per row (512 bf16 / 256 f32):
//  - staging: a wave owns 8 whole rows; each of its 16 B/lane loads is one
//    fully coalesced 1 KB run of ONE row stream, whose base is a scalar
//    pointer read from the kernel argument. The chunk after the current one
//    is loaded into registers before the current one is consumed (load /
//    ds_write split), so eight 1 KB runs per wave stay in flight under the
//    MFMAs. Rows past n are not read at all (the row index is wave-uniform)
//    and stage zeros;
//  - LDS image: [64 rows][64 slots of 16 B], slot s of row r stored at
//    s ^ (r & 15) as in gram_bf16_lds_kernel: the 16 rows of a fragment read
//    land on 16 different bank quads;
//  - compute: the chunk's K is split over the WAVES, not its tiles: wave w
//    takes slots [8w, 8w + 8) of every row and accumulates all 10 upper-
//    triangle 16 x 16 tile pairs (40 accumulator registers) from 4 fragment
//    reads per 4 slots. Lane (r, q) reads slot 4s + q of row 16a + r: for
//    bf16 that is one v_mfma_f32_16x16x32_bf16 operand, for f32 four
//    successive v_mfma_f32_16x16x4_f32 operands. A Gram sums over k, so which
//    k a (lane, step) names is free as long as both operands agree, and they
//    are the same registers. Tile blocks past ceil(n / 16) are skipped;
//  - ragged end: lanes whose 16 B run crosses d load element by element
//    under a predicate, lanes past d stage zeros: same kernel, last chunk;
//  - VEC = false (a row pointer that is not 16 B aligned): every lane takes
//    that element path.
// The 8 waves' partial tiles meet in a 64 x 64 f32 LDS image (ds_add_f32),
// and the block adds the upper triangle into the caller-zeroed G with f32
// atomics, as gram.hip combines its split-K partials. A second, one-block
// launch copies the upper triangle over the lower one: the two halves of G
// are the same sums, bit for bit, which two sets of atomics arriving in two
// orders would not be.
#include "common.h"
#include "launchers.h"
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 gr_bf16x8;
typedef __attribute__((ext_vector_type(4))) float gr_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int gr_u32x4;

constexpr int GR_WAVES = 8;
constexpr int GR_THREADS = GR_WAVES * 64;
constexpr int GR_TILE = 64;                         // rows of the image
constexpr int GR_ROW_BYTES = 1024;                  // one wave-wide 16 B run
constexpr int GR_SLOTS = GR_ROW_BYTES / 16;         // 64 per row
constexpr int GR_LDS_BYTES = GR_TILE * GR_ROW_BYTES;  // 65,536
constexpr int GR_OWN = GR_TILE / GR_WAVES;          // rows a wave stages
constexpr int GR_TILES = 10;                        // 16x16 blocks a <= b

constexpr int gr_tile(int a, int b) { return 4 * a - a * (a - 1) / 2 + (b - a); }

// The lane's 16 B of row `p` starting at element e0; elements at or past d
// read as zero. VEC runs that lie wholly inside the row are one load.
template <typename T, bool VEC>
DEV gr_u32x4 load_run(const char* p, long e0, long d) {
  constexpr int EPS = 16 / (int)sizeof(T);
  // raw words: the elements are only moved here
  using E = std::conditional_t<sizeof(T) == 2, unsigned short, unsigned int>;
  if (VEC && e0 + EPS <= d)
    return *reinterpret_cast<const gr_u32x4*>(p + e0 * (long)sizeof(T));
  union { gr_u32x4 v; E e[EPS]; } u;
  u.v = gr_u32x4{0u, 0u, 0u, 0u};
  const E* src = reinterpret_cast<const E*>(p);
#pragma unroll
  for (int t = 0; t < EPS; ++t)
    if (e0 + t < d) u.e[t] = src[e0 + t];
  return u.v;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(GR_THREADS, 2)
gram_rowptrs_kernel(RowPtrTable tbl, float* __restrict__ G, int n, long d,
                    long chunks_per_block) {
  constexpr int EPS = 16 / (int)sizeof(T);           // elements per slot
  constexpr int BK = GR_ROW_BYTES / (int)sizeof(T);  // elements per chunk row
  __shared__ __attribute__((aligned(16))) char img[GR_LDS_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long nchunks = (d + BK - 1) / BK;
  const long c_lo = (long)blockIdx.x * chunks_per_block;
  const long c_hi = min(nchunks, c_lo + chunks_per_block);
  const int nb = (n + 15) >> 4;  // 16-row blocks that hold a real row

  // this wave's row streams: wave-uniform, so they live in scalar registers
  const char* rp[GR_OWN];
#pragma unroll
  for (int j = 0; j < GR_OWN; ++j)
    rp[j] = reinterpret_cast<const char*>(
        tbl.p[min(wave * GR_OWN + j, n - 1)]);

  gr_u32x4 st[GR_OWN];
  auto stage_load = [&](long c) {
    const long e0 = c * BK + (long)lane * EPS;
#pragma unroll
    for (int j = 0; j < GR_OWN; ++j) {
      st[j] = gr_u32x4{0u, 0u, 0u, 0u};
      if (wave * GR_OWN + j < n) st[j] = load_run<T, VEC>(rp[j], e0, d);
    }
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int j = 0; j < GR_OWN; ++j) {
      const int row = wave * GR_OWN + j;
      *reinterpret_cast<gr_u32x4*>(img + row * GR_ROW_BYTES +
                                   ((lane ^ (row & 15)) * 16)) = st[j];
    }
  };

  gr_f32x4 acc[GR_TILES];
#pragma unroll
  for (int e = 0; e < GR_TILES; ++e) acc[e] = gr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int fr = lane & 15, fq = lane >> 4;

  stage_load(c_lo);
  for (long c = c_lo; c < c_hi; ++c) {
    stage_write();
    __syncthreads();
    if (c + 1 < c_hi) stage_load(c + 1);
#pragma unroll
    for (int s = 0; s < GR_SLOTS / GR_WAVES / 4; ++s) {
      const int slot = wave * (GR_SLOTS / GR_WAVES) + 4 * s + fq;
      gr_u32x4 f[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        f[a] = gr_u32x4{0u, 0u, 0u, 0u};
        if (a < nb)
          f[a] = *reinterpret_cast<const gr_u32x4*>(
              img + (16 * a + fr) * GR_ROW_BYTES + ((slot ^ fr) * 16));
      }
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = a; b < 4; ++b)
            if (b < nb)
              acc[gr_tile(a, b)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  __builtin_bit_cast(gr_bf16x8, f[a]),
                  __builtin_bit_cast(gr_bf16x8, f[b]), acc[gr_tile(a, b)], 0,
                  0, 0);
      } else {
        // k-step outermost: two MFMAs into one tile are nine apart, past
        // the dependent-accumulator latency
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b)
              if (b < nb)
                acc[gr_tile(a, b)] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    __builtin_bit_cast(gr_f32x4, f[a])[kk],
                    __builtin_bit_cast(gr_f32x4, f[b])[kk],
                    acc[gr_tile(a, b)], 0, 0, 0);
      }
    }
    __syncthreads();  // the image is free for the next chunk (or the sums)
  }

  // the waves' partials meet in a 64 x 64 f32 image in the (now free) LDS
  float* const red = reinterpret_cast<float*>(img);
  for (int i = tid; i < GR_TILE * GR_TILE; i += GR_THREADS) red[i] = 0.0f;
  __syncthreads();
  // C/D map for 16x16: col = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b)
      if (b < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          atomicAdd(&red[(16 * a + 4 * fq + r) * GR_TILE + 16 * b + fr],
                    acc[gr_tile(a, b)][r]);
      }
  __syncthreads();
  for (int i = tid; i < GR_TILE * GR_TILE; i += GR_THREADS) {
    const int row = i >> 6, col = i & 63;
    if (row <= col && col < n) atomicAdd(&G[(long)row * n + col], red[i]);
  }
}

// ---------------------------------------------------------------------------
// Mean of selected rows of the table: out = sum_i row[idx[i]] / k, i < k, with
// the int32 index vector on the device (the Krum winners never visit the
// host) and f32 accumulation. V = 16 B of consecutive coordinates per thread
// and grid-stride step when VEC (every row and `out` 16 B aligned), four row
// loads in flight per step and the association (x0 + x1) + (x2 + x3) of
// rowops.hip's col_wsum; the d % V coordinates past the last full vector,
// and everything when !VEC, go one element per thread. idx is clamped to
// [0, n): a bad index can misselect but never read out of bounds.
// ---------------------------------------------------------------------------

template <typename T>
DEV void unpack_run(const gr_u32x4 w, float (&o)[16 / sizeof(T)]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = __uint_as_float(w[c]);
  } else {  // a bf16 is the upper half of its f32
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      o[2 * c] = __uint_as_float(w[c] << 16);
      o[2 * c + 1] = __uint_as_float(w[c] & 0xFFFF0000u);
    }
  }
}

template <typename T>
DEV gr_u32x4 pack_run(const float (&o)[16 / sizeof(T)]) {
  gr_u32x4 w;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = __float_as_uint(o[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      union { unsigned short s; __hip_bfloat16 h; } lo, hi;
      lo.h = __float2bfloat16(o[2 * c]);
      hi.h = __float2bfloat16(o[2 * c + 1]);
      w[c] = (unsigned int)lo.s | ((unsigned int)hi.s << 16);
    }
  }
  return w;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
mean_rowptrs_kernel(RowPtrTable tbl, int n, const int* __restrict__ idx,
                    int k, T* __restrict__ out, long d) {
  constexpr int V = 16 / (int)sizeof(T);
  const float inv = 1.0f / (float)k;
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  auto row = [&](int i) {
    return reinterpret_cast<const T*>(tbl.p[min(max(idx[i], 0), n - 1)]);
  };
  const long dv = VEC ? d / V : 0;
  for (long jv = start; jv < dv; jv += stride) {
    auto run = [&](int i, float (&x)[V]) {
      unpack_run<T>(*reinterpret_cast<const gr_u32x4*>(row(i) + jv * V), x);
    };
    float acc[V] = {0};
    int i = 0;
    for (; i + 4 <= k; i += 4) {
      float x0[V], x1[V], x2[V], x3[V];
      run(i, x0);
      run(i + 1, x1);
      run(i + 2, x2);
      run(i + 3, x3);
#pragma unroll
      for (int c = 0; c < V; ++c) acc[c] += (x0[c] + x1[c]) + (x2[c] + x3[c]);
    }
    for (; i < k; ++i) {
      float x[V];
      run(i, x);
#pragma unroll
      for (int c = 0; c < V; ++c) acc[c] += x[c];
    }
#pragma unroll
    for (int c = 0; c < V; ++c) acc[c] *= inv;
    *reinterpret_cast<gr_u32x4*>(out + jv * V) = pack_run<T>(acc);
  }
  for (long j = dv * V + start; j < d; j += stride) {
    float acc = 0.0f;
    for (int i = 0; i < k; ++i) acc += to_f<T>(row(i)[j]);
    out[j] = from_f<T>(acc * inv);
  }
}

// ---------------------------------------------------------------------------
// Combine (K20): out = sum_i coef[i] x_i with the f32 coefficients on the
// device. Not a mean: nothing is normalised, coefficients may be negative or
// zero. Each block first compacts the rows with coef != 0 into LDS (pointer
// and coefficient, in row order), so a row under a zero coefficient (a dead
// row full of inf or NaN) is never read, and the column loop walks LDS only.
// One thread owns 16 B of consecutive coordinates per grid-stride step, four
// row loads in flight, and adds acc = fma(c_k, x_k, acc) strictly in row
// order. The vector loop runs when every compacted row and `out` are 16 B
// aligned (a block-wide vote); the d % V coordinates past the last full
// vector, and everything otherwise, go one element per thread through the
// same fma chain. Rows = the table or a contiguous matrix: one kernel text,
// so a list and its stacked matrix give the same bits.
// ---------------------------------------------------------------------------

constexpr int CMB_THREADS = 256;
constexpr int CMB_MAX_BLOCKS = 4096;
static_assert(CMB_THREADS >= GRAMFP_MAX_N, "one thread per row compacts");

struct TableRows {
  RowPtrTable t;
  DEV const char* row(int i) const {
    return reinterpret_cast<const char*>(t.p[i]);
  }
};
struct MatrixRows {
  const char* base;
  long row_bytes;
  DEV const char* row(int i) const { return base + (long)i * row_bytes; }
};

template <typename T, typename Rows>
__global__ void __launch_bounds__(CMB_THREADS)
combine_rows_kernel(Rows src, const float* __restrict__ coef, int n,
                    T* __restrict__ out, long d) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ const char* rowp[GRAMFP_MAX_N];
  __shared__ float cf[GRAMFP_MAX_N];
  __shared__ int nzf[GRAMFP_MAX_N];
  const int tid = threadIdx.x;

  float c = 0.0f;
  const char* p = nullptr;
  bool nz = false;
  if (tid < n) {
    c = coef[tid];
    nz = c != 0.0f;
    if (nz) p = src.row(tid);
  }
  if (tid < GRAMFP_MAX_N) nzf[tid] = nz ? 1 : 0;
  const int m = __syncthreads_count(nz);
  const bool misaligned =
      nz && reinterpret_cast<unsigned long>(p) % 16 != 0;
  const bool vec = __syncthreads_or(misaligned) == 0 &&
                   reinterpret_cast<unsigned long>(out) % 16 == 0;
  if (nz) {
    int before = 0;
    for (int j = 0; j < tid; ++j) before += nzf[j];
    rowp[before] = p;
    cf[before] = c;
  }
  __syncthreads();

  const long start = (long)blockIdx.x * CMB_THREADS + tid;
  const long stride = (long)gridDim.x * CMB_THREADS;
  const long dv = vec ? d / V : 0;
  for (long jv = start; jv < dv; jv += stride) {
    const long off = jv * 16;
    auto run = [&](int k) {
      return *reinterpret_cast<const gr_u32x4*>(rowp[k] + off);
    };
    auto add = [&](int k, const gr_u32x4 w, float (&acc)[V]) {
      float x[V];
      unpack_run<T>(w, x);
      const float ck = cf[k];
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = fmaf(ck, x[e], acc[e]);
    };
    float acc[V] = {0};
    int k = 0;
    for (; k + 4 <= m; k += 4) {
      const gr_u32x4 w0 = run(k), w1 = run(k + 1), w2 = run(k + 2),
                     w3 = run(k + 3);
      add(k, w0, acc);
      add(k + 1, w1, acc);
      add(k + 2, w2, acc);
      add(k + 3, w3, acc);
    }
    for (; k < m; ++k) add(k, run(k), acc);
    *reinterpret_cast<gr_u32x4*>(out + jv * V) = pack_run<T>(acc);
  }
  for (long j = dv * V + start; j < d; j += stride) {
    float acc = 0.0f;
    for (int k = 0; k < m; ++k)
      acc = fmaf(cf[k], to_f<T>(reinterpret_cast<const T*>(rowp[k])[j]), acc);
    out[j] = from_f<T>(acc);
  }
}

// G[i][j] = G[j][i] for i > j, once every partial has landed
__global__ void gram_rowptrs_mirror_kernel(float* __restrict__ G, int n) {
  for (int i = threadIdx.x; i < n * n; i += blockDim.x) {
    const int row = i / n, col = i - row * n;
    if (row > col) G[i] = G[(long)col * n + row];
  }
}

}  // namespace

// Split-K geometry: `blocks` workgroups of `chunks_per_block` consecutive
// 1 KB-per-row chunks, at most two workgroups per CU (what 64 KB of LDS each
// admits), none of them empty.
void gram_rowptrs_geometry(long d, int elem_bytes, int cus, long& blocks,
                           long& chunks_per_block) {
  const long bk = GR_ROW_BYTES / elem_bytes;
  const long nchunks = d > 0 ? (d + bk - 1) / bk : 1;
  const long want = 2L * (cus > 0 ? cus : 256);
  chunks_per_block = (nchunks + want - 1) / want;
  blocks = (nchunks + chunks_per_block - 1) / chunks_per_block;
}

template <typename T>
void launch_gram_rowptrs(const RowPtrTable& rows, float* G, int n, long d,
                         hipStream_t stream) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess)
    cus = 0;
  long blocks, cpb;
  gram_rowptrs_geometry(d, (int)sizeof(T), cus, blocks, cpb);
  if (rowptrs_aligned(rows, n, 16))
    hipLaunchKernelGGL((gram_rowptrs_kernel<T, true>), dim3((unsigned)blocks),
                       dim3(GR_THREADS), 0, stream, rows, G, n, d, cpb);
  else
    hipLaunchKernelGGL((gram_rowptrs_kernel<T, false>), dim3((unsigned)blocks),
                       dim3(GR_THREADS), 0, stream, rows, G, n, d, cpb);
  hipLaunchKernelGGL(gram_rowptrs_mirror_kernel, dim3(1), dim3(1024), 0, stream,
                     G, n);
}
INSTANTIATE_LAUNCHER(launch_gram_rowptrs)

template <typename T>
void launch_mean_rows_rowptrs(const RowPtrTable& rows, int n, const int* idx,
                              int k, T* out, long d, hipStream_t stream) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = rowptrs_aligned(rows, n, 16) &&
                   reinterpret_cast<unsigned long>(out) % 16 == 0;
  const long work = vec && d >= V ? d / V : d;
  const long want = (work + 255) / 256;
  const dim3 grid((unsigned)(want < 4096 ? (want > 0 ? want : 1) : 4096));
  if (vec)
    hipLaunchKernelGGL((mean_rowptrs_kernel<T, true>), grid, dim3(256), 0,
                       stream, rows, n, idx, k, out, d);
  else
    hipLaunchKernelGGL((mean_rowptrs_kernel<T, false>), grid, dim3(256), 0,
                       stream, rows, n, idx, k, out, d);
}
INSTANTIATE_LAUNCHER(launch_mean_rows_rowptrs)

template <typename T>
void launch_combine_rows(const T* X, const RowPtrTable& rows, const float* coef,
                         int n, T* out, long d, hipStream_t stream) {
  constexpr int V = 16 / (int)sizeof(T);
  const long want = (d / V + CMB_THREADS) / CMB_THREADS;
  const dim3 grid((unsigned)(want < CMB_MAX_BLOCKS ? want : CMB_MAX_BLOCKS));
  if (X == nullptr)
    hipLaunchKernelGGL((combine_rows_kernel<T, TableRows>), grid,
                       dim3(CMB_THREADS), 0, stream, TableRows{rows}, coef, n,
                       out, d);
  else
    hipLaunchKernelGGL((combine_rows_kernel<T, MatrixRows>), grid,
                       dim3(CMB_THREADS), 0, stream,
                       MatrixRows{reinterpret_cast<const char*>(X),
                                  d * (long)sizeof(T)},
                       coef, n, out, d);
}
INSTANTIATE_LAUNCHER(launch_combine_rows)
