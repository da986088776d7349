// Grouped column selection (K24): the column median / trimmed mean /
// mean-around-median of M row sets of one (N, d) matrix in ONE pass over it.
// Row i of the (M, d) result is the statistic over X[groups[i] valid], as
// colsel(X, mode, f, rows=groups[i]) defines it: a gossip round of a
// coordinate-wise rule, where node i aggregates its own row and its
// neighbours'. The per-node calls read every neighbourhood's rows again from
// HBM, (sum m_i + M) d elements; here each row of X is read once and each
// output row written once, (N + M) d.
//
// Which rows a node reads is runtime data, and a runtime-indexed register
// column spills (colsel.hip), so the strip goes through LDS and only the
// node's own values ever sit in registers, at compile-time slots.
//
// A wave owns strips of 64 columns, one column per lane, and walks them
// grid-stride. A workgroup is 4 waves, each with a PRIVATE slab of dynamic
// LDS: no wave reads what another wrote, so the strip loop has no block
// barrier, only colsel_mix.hip's wave-level fence.
//  - stage: the wave reads the N rows of its strip once, each row one
//    coalesced 128 B (bf16) / 256 B (f32) wave transaction, in batches of
//    GRP_BATCH rows through two register sets: while one batch is written to
//    the slab the next one's loads are in flight (the pinned load walk of
//    colsel_reg_kernel, one live scalar base). The raw words land as
//    [row][lane]: a later read of row g by all 64 lanes hits 64 consecutive
//    words, conflict-free. The slab is rows(N) x 64 x sizeof(T) bytes with
//    rows(N) = N padded to a whole batch, sized at launch from N so that a
//    small ring keeps its occupancy (N = 8 bf16: 2 KB a wave; N = 128 f32:
//    32 KB a wave, one workgroup per CU).
//  - per node i: lane k < m holds groups[i][k] (one coalesced read, fetched
//    one node ahead), a ballot counts the valid entries m_i, and slot k's
//    slab offset reaches the scalar unit by v_readlane with k compile-time,
//    as the indexed register kernels pass their row offsets. The lane reads
//    its m_i values into v[0..P), converts to f32, pads the slots >= m_i as
//    colsel_reg_kernel does (median: low / high pads by median_pad_split;
//    the other modes: +inf) and runs selnet.h's networks: half_sort +
//    median_select, bitonic_sort, and for mean-around-median the key-value
//    bitonic sort. The arithmetic after the network is colsel_reg_kernel's,
//    operation for operation, so median and trimmed mean agree with the
//    indexed kernel bit for bit. out[i * d + col] is one coalesced store.
//    P is max m padded to {4, 8, 16, 32}; a ragged node runs the same
//    network with more pads.
//
// Table safety: indices are clamped to [0, N), so a bad table can misselect
// but never read out of bounds; slots past m read the row's last entry again
// and are padded over. A row of `groups` with no valid entry gives an
// unspecified (in-bounds) result. Lanes past d clamp their loads and skip
// the store.
//
// Values that are not finite follow the register kernels: +-inf order as
// values and no accumulator ever holds a dropped element, so a trimmed +-inf
// or +-1e30 leaves the exact honest mean; NaN order statistics are
// unspecified.
//
// bitonic_sort_kv below repeats colsel.hip's bitonic_sort_kv_reg: it swaps on
// a comparison, so it is no selnet.h min/max network, and it lives in
// colsel.hip's unnamed namespace where this file cannot reach it.
//
// Known alternative, not built: sort the column ONCE with the row index as
// payload and let every node walk the sorted column under its membership
// mask. Cheaper for dense topologies (m near N), where this kernel's M
// sorts of m repeat most of each other's comparisons.
#include "colsel_shared.h"
#include "launchers.h"
#include "selnet.h"

namespace {

constexpr int GRP_THREADS = 256;
constexpr int GRP_WAVES = GRP_THREADS / 64;
constexpr int GRP_BATCH = 16;  // rows per register set of the stage
constexpr long GRP_LDS_PER_CU = 160 * 1024;
constexpr long GRP_MAX_BLOCKS_PER_CU = 8;

inline int grp_slab_rows(int n) {
  return (n + GRP_BATCH - 1) / GRP_BATCH * GRP_BATCH;
}

template <int P>
DEV void bitonic_sort_kv(float (&key)[P], float (&val)[P]) {
#pragma unroll
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const bool asc = (i & k) == 0;
          const float a = key[i], b = key[l];
          if (asc ? (a > b) : (a < b)) {
            key[i] = b; key[l] = a;
            const float t = val[i]; val[i] = val[l]; val[l] = t;
          }
        }
      }
    }
  }
}

// slot K of raw: the lane's word of the slab row whose byte offset lane K of
// `goff` holds. Raw reads and a pinned readlane / read alternation, as in
// colsel.hip's load_rows_indexed: left alone the compiler pulls all P offsets
// into SGPRs first and spills them.
template <int P, int K = 0, typename T>
DEV void read_slots(T (&raw)[P], const char* rd, u32 goff) {
  if constexpr (K < P) {
    const u32 o = __builtin_amdgcn_readlane(goff, K);
    raw[K] = *reinterpret_cast<const T*>(rd + o);
    __builtin_amdgcn_sched_barrier(0);
    read_slots<P, K + 1>(raw, rd, goff);
  }
}

// n: rows of X, nr: rows of a slab (grp_slab_rows(n)), groups (M, m)
template <int P, int MODE, typename T>
__global__ void __launch_bounds__(GRP_THREADS)
colsel_groups_kernel(const T* __restrict__ X, const int* __restrict__ groups,
                     T* __restrict__ out, int n, int nr, int M, int m, long d,
                     int f) {
  extern __shared__ __attribute__((aligned(16))) char grp_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  char* const slab = grp_lds + (long)wave * nr * (64 * sizeof(T));
  T* const wr = reinterpret_cast<T*>(slab) + lane;
  const char* const rd = slab + lane * sizeof(T);
  // lane k's entry of node i; lanes past m repeat the row's last entry
  const int gl = min(lane, m - 1);
  auto node_rows = [&](int i) { return groups[(long)i * m + gl]; };

  const long rowbytes = d * (long)sizeof(T);
  const long nstrips = (d + 63) >> 6;
  const long nwaves = (long)gridDim.x * GRP_WAVES;
  for (long strip = (long)blockIdx.x * GRP_WAVES + wave; strip < nstrips;
       strip += nwaves) {
    const long col = strip * 64 + lane;
    const long ccol = min(col, d - 1);  // tail lanes: clamped, not stored
    int gcur = node_rows(0);

    // stage: a wave-uniform row base on the scalar unit plus one per-lane
    // byte offset; the walk stops at row n - 1 and the slab rows past it
    // repeat that row (no node reads them)
    const char* rowp = reinterpret_cast<const char*>(X + strip * 64);
    const u32 off = (u32)(ccol - strip * 64) * (u32)sizeof(T);
    // the walk's bounds are opaque per strip, or the first batch's chosen
    // steps are hoisted out of the strip loop into SGPRs that spill
    // (colsel_mix.hip)
    int r = 0, n_walk = n;
    long rowstep = rowbytes;
    asm volatile("" : "+s"(n_walk), "+s"(rowstep));
    auto load = [&](T (&dst)[GRP_BATCH]) __attribute__((always_inline)) {
#pragma unroll
      for (int b = 0; b < GRP_BATCH; ++b) {
        dst[b] = *reinterpret_cast<const T*>(rowp + off);
        if (++r < n_walk) rowp += rowstep;
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    auto store = [&](const T (&src)[GRP_BATCH], int r0)
        __attribute__((always_inline)) {
#pragma unroll
      for (int b = 0; b < GRP_BATCH; ++b) wr[(r0 + b) * 64] = src[b];
    };
    wave_lds_fence();  // the last strip's slot reads stay above the stores
    T ra[GRP_BATCH], rb[GRP_BATCH];
    load(ra);
    for (int r0 = 0; r0 < nr; r0 += 2 * GRP_BATCH) {
      const bool more = r0 + GRP_BATCH < nr;
      if (more) load(rb);
      store(ra, r0);
      if (more) {
        if (r0 + 2 * GRP_BATCH < nr) load(ra);
        store(rb, r0 + GRP_BATCH);
      }
    }
    wave_lds_fence();  // the slab is complete for this wave's own reads

    for (int i = 0; i < M; ++i) {
      const int gnext = node_rows(min(i + 1, M - 1));  // one node ahead
      const int mi = __popcll(__ballot(lane < m && gcur >= 0));
      const u32 goff =
          (u32)min(max(gcur, 0), n - 1) * (u32)(64 * sizeof(T));
      T raw[P];
      read_slots<P>(raw, rd, goff);
      float v[P];
      // m_i in a VGPR: see vecify
      const int mv = vecify(mi);

      float result;
      if (MODE == MEDIAN) {
        // each half converted and padded right before its sort, as in
        // colsel_reg_kernel: all P pad compares at once would hold 2 P
        // lane masks in SGPRs, which spill at P = 32
        const int n_lo = vecify(selnet::median_pad_split<P>(mi));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int base = h * (P / 2);
#pragma unroll
          for (int k = base; k < base + P / 2; ++k) {
            v[k] = to_f<T>(raw[k]);
            if (k >= mv) v[k] = (k < n_lo) ? -PAD : PAD;
          }
          if (h == 0)
            selnet::half_sort<P / 2, true, F32MinMax>(selnet::half<0>(v));
          else
            selnet::half_sort<P / 2, false, F32MinMax>(selnet::half<1>(v));
        }
        float mlo, mhi;
        selnet::median_select<P, F32MinMax>(v, mlo, mhi);
        result = (mi & 1) ? mlo : 0.5f * (mlo + mhi);
      } else if (MODE == TRIMMED) {
#pragma unroll
        for (int k = 0; k < P; ++k) v[k] = to_f<T>(raw[k]);
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (k >= mv) v[k] = PAD;
        selnet::bitonic_sort<P, F32MinMax>(v);
        const int fv = vecify(f), nfv = vecify(mi - f);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (k >= fv && k < nfv) s += v[k];
        result = s / (float)(mi - 2 * f);
      } else {  // MEAMED: mean of the m_i - f values closest to the median
#pragma unroll
        for (int k = 0; k < P; ++k) {
          v[k] = to_f<T>(raw[k]);
          if (k >= mv) v[k] = PAD;
        }
        selnet::bitonic_sort<P, F32MinMax>(v);
        const int pos_lo = vecify((mi - 1) >> 1), pos_hi = vecify(mi >> 1);
        const float med = 0.5f * (selnet::extract_at(v, pos_lo) +
                                  selnet::extract_at(v, pos_hi));
        const int nfv = vecify(mi - f);
        float dev[P];
#pragma unroll
        for (int k = 0; k < P; ++k)
          dev[k] = (k < mv) ? fabsf(v[k] - med) : PAD;
        bitonic_sort_kv<P>(dev, v);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (k < nfv) s += v[k];
        result = s / (float)(mi - f);
      }
      if (col < d) out[(long)i * d + col] = from_f<T>(result);
      gcur = gnext;
    }
  }
}

}  // namespace

// Persistent grid: as many workgroups per CU as their slabs admit (8 at the
// most); the waves stride over the strips.
template <typename T>
void launch_colsel_groups(const T* X, const int* groups, T* out, int n, int M,
                          int m, long d, int mode, int f, hipStream_t stream) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  const int nr = grp_slab_rows(n);
  const size_t lds = (size_t)GRP_WAVES * nr * 64 * sizeof(T);
  long per_cu = GRP_LDS_PER_CU / (long)lds;
  per_cu = per_cu < 1 ? 1 : (per_cu > GRP_MAX_BLOCKS_PER_CU
                                 ? GRP_MAX_BLOCKS_PER_CU : per_cu);
  const long nstrips = (d + 63) / 64;
  const long need = (nstrips + GRP_WAVES - 1) / GRP_WAVES;
  const long cap = per_cu * cus;
  const unsigned blocks = (unsigned)(need < cap ? need : cap);
  auto by_width = [&](auto fn) {
    if (m <= 4) fn(std::integral_constant<int, 4>{});
    else if (m <= 8) fn(std::integral_constant<int, 8>{});
    else if (m <= 16) fn(std::integral_constant<int, 16>{});
    else fn(std::integral_constant<int, 32>{});
  };
  by_mode(mode, [&](auto md) {
    by_width([&](auto p) {
      hipLaunchKernelGGL(
          (colsel_groups_kernel<decltype(p)::value, decltype(md)::value, T>),
          dim3(blocks), dim3(GRP_THREADS), lds, stream, X, groups, out, n, nr,
          M, m, d, f);
    });
  });
}
INSTANTIATE_LAUNCHER(launch_colsel_groups)
