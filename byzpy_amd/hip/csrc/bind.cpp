// Python bindings for the byzpy_amd gfx950 kernel library.
// Built in-tree by hip/build.py with explicit hipcc (no hipify, no CUDA
// shims). Each op: validate, allocate, launch on the current stream.
#include <cstdlib>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <climits>
#include <cmath>
#include <vector>

#include "launchers.h"
#include "mda_host.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// -- argument checks --------------------------------------------------------

void check_matrix(const torch::Tensor& X) {
  TORCH_CHECK(X.is_cuda(), "expected a device tensor");
  TORCH_CHECK(X.dim() == 2, "expected (n, d)");
  TORCH_CHECK(X.is_contiguous(), "expected contiguous input");
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 ||
                  X.scalar_type() == torch::kBFloat16,
              "expected f32 or bf16");
}

void check_f32_vector(const torch::Tensor& t, int64_t len, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.is_contiguous() && t.numel() == len,
              name, ": expected an f32 contiguous device vector of length ",
              len);
}

void check_f32_scalar(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.numel() == 1,
              name, ": expected an f32 device scalar");
}

// int32 contiguous device tensor with `ndim` dimensions
void check_i32(const torch::Tensor& t, int64_t ndim, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                  t.is_contiguous() && t.dim() == ndim,
              name, ": expected an int32 contiguous device tensor with ", ndim,
              " dim(s)");
}

void check_gram(const torch::Tensor& G, const char* name) {
  TORCH_CHECK(G.is_cuda() && G.dim() == 2 && G.size(0) == G.size(1) &&
                  G.scalar_type() == torch::kFloat32 && G.is_contiguous(),
              name, ": expected a square f32 contiguous device matrix");
}

// weiszfeld_update / cc_update / caf_colsum stage one weight per row in a
// MAX_N_LDS-float LDS array; a larger n would write past it. Call before
// any allocation or launch.
void check_rows_fit_lds(int64_t n, const char* op) {
  TORCH_CHECK(n <= MAX_N_LDS, op, " supports n <= ", MAX_N_LDS, ", got ", n);
}

// -- dtype dispatch ---------------------------------------------------------

template <typename T>
struct dtype_tag { using type = T; };

// Calls fn(dtype_tag<T>) with T = float or __hip_bfloat16 after X's dtype
// (check_matrix has already rejected everything else).
template <typename F>
void by_dtype(const torch::Tensor& X, F&& fn) {
  if (X.scalar_type() == torch::kFloat32)
    fn(dtype_tag<float>{});
  else
    fn(dtype_tag<__hip_bfloat16>{});
}
#define TAG_T(tag) typename decltype(tag)::type

template <typename T>
T* ptr(const torch::Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }
float* f32(const torch::Tensor& t) { return t.data_ptr<float>(); }
int* i32(const torch::Tensor& t) { return t.data_ptr<int>(); }

torch::TensorOptions f32_like(const torch::Tensor& X) {
  return X.options().dtype(torch::kFloat32);
}
torch::TensorOptions i32_like(const torch::Tensor& X) {
  return X.options().dtype(torch::kInt32);
}

// -- ops --------------------------------------------------------------------

// mean-around-median keeps n - f values, so any f < n is meaningful
// (Bulyan runs it with 2f >= n); median and trimmed mean need 2f < n
void check_colsel_f(int64_t mode, int64_t f, int64_t n) {
  TORCH_CHECK(f >= 0 && (mode == 2 ? f < n : 2 * f < n), "bad f for colsel");
}

// Row-indexed colsel: the statistic over X[rows] without the gather. Only
// the selected count m is capped (colsel.hip register / LDS kernels, never
// the radix engine); the source matrix may have any number of rows.
torch::Tensor colsel_rows(const torch::Tensor& X, int64_t mode, int64_t f,
                          const torch::Tensor& rows) {
  check_i32(rows, 1, "rows");
  const int64_t m = rows.numel();
  TORCH_CHECK(m >= 1 && m <= COLSEL_MAX_ROWS, "colsel with rows supports 1 <= ",
              "len(rows) <= ", COLSEL_MAX_ROWS, ", got ", m);
  TORCH_CHECK(X.size(0) >= 1 && X.size(0) <= INT_MAX, "bad row count");
  check_colsel_f(mode, f, m);
  const long d = (long)X.size(1);
  auto out = torch::empty({d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_colsel<T>(ptr<T>(X), ptr<T>(out), (int)m, d, (int)mode, (int)f,
                     i32(rows), (int)X.size(0), cur_stream());
  });
  return out;
}

torch::Tensor colsel(torch::Tensor X, int64_t mode, int64_t f,
                     c10::optional<torch::Tensor> rows,
                     c10::optional<torch::Tensor> gram);

// colsel(X, 0, f, gram=G): the column median, and G overwritten with
// X X^T. One pass over X where the fused kernel applies (bf16,
// 32 < n <= 64, even d), else the median and Gram launches one after the
// other, so the call means the same for every input. The fused launcher
// checks G's diagonal on the device and reruns the median kernel if an
// entry is not finite, so G has to be zeroed and filled by THIS call.
torch::Tensor colsel_with_gram(const torch::Tensor& X, int64_t mode, int64_t f,
                               bool has_rows, const torch::Tensor& G) {
  TORCH_CHECK(mode == 0, "colsel(gram=) computes the median: expected mode 0, ",
              "got ", mode);
  TORCH_CHECK(!has_rows, "colsel(gram=) does not take rows");
  check_gram(G, "gram");
  const int64_t n = X.size(0);
  const long d = (long)X.size(1);
  TORCH_CHECK(G.size(0) == n, "gram: expected (", n, ", ", n, "), got (",
              G.size(0), ", ", G.size(1), ")");
  TORCH_CHECK(G.device() == X.device(), "gram: expected X's device");
  if (X.scalar_type() == torch::kBFloat16 && median_gram_bf16_applies(n, d)) {
    check_colsel_f(mode, f, n);
    auto out = torch::empty({d}, X.options());
    G.zero_();
    torch::Tensor ticket;
    unsigned long long* ticket_ptr = nullptr;
    // BYZPY_MEDIAN_GRAM_TICKET=1 / 0 forces the work counter on / off (the
    // tests reach the ticketed loop at small d with it)
    const char* force = std::getenv("BYZPY_MEDIAN_GRAM_TICKET");
    const bool ticketed = (force != nullptr && (force[0] == '0' || force[0] == '1'))
                              ? force[0] == '1'
                              : median_gram_bf16_ticketed(d);
    if (ticketed) {
      ticket = torch::zeros({1}, X.options().dtype(torch::kInt64));
      ticket_ptr =
          reinterpret_cast<unsigned long long*>(ticket.data_ptr<int64_t>());
    }
    launch_median_gram_bf16(ptr<__hip_bfloat16>(X), ptr<__hip_bfloat16>(out),
                            f32(G), ticket_ptr, (int)n, d, cur_stream());
    return out;
  }
  auto out = colsel(X, mode, f, c10::nullopt, c10::nullopt);
  G.zero_();
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_gram<T>(ptr<T>(X), f32(G), (int)n, d, cur_stream());
  });
  return out;
}

torch::Tensor colsel(torch::Tensor X, int64_t mode, int64_t f,
                     c10::optional<torch::Tensor> rows,
                     c10::optional<torch::Tensor> gram) {
  check_matrix(X);
  if (gram.has_value())
    return colsel_with_gram(X, mode, f, rows.has_value(), *gram);
  if (rows.has_value()) return colsel_rows(X, mode, f, *rows);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  // measured crossovers: register kernels to n = 64; past that the
  // 64-bin streaming radix engine (rsel.hip, ~5.3 TB/s per pass) beats
  // the cooperative LDS sort at every measured shape unless d is tiny
  // (launch-count-bound) — the LDS path stays for 64 < n <= 512 at
  // small d, radix is the only path above 512
  const bool radix_ok =
      n <= 65535 && (n > 512 || (n > 64 && d >= 32768));
  TORCH_CHECK(n >= 1 && (n <= 512 || radix_ok),
              "colsel supports 1 <= n <= 65535, got ", n);
  check_colsel_f(mode, f, n);
  auto out = torch::empty({d}, X.options());
  if (!radix_ok) {
    by_dtype(X, [&](auto tag) {
      using T = TAG_T(tag);
      launch_colsel<T>(ptr<T>(X), ptr<T>(out), n, d, (int)mode, (int)f,
                       nullptr, n, cur_stream());
    });
    return out;
  }
  // generic multi-pass engine (rsel.hip): per-column state scratch, plus
  // a median buffer for mean-around-median
  auto state = torch::zeros({d * 4}, i32_like(X));
  torch::Tensor med;
  if (mode == 2) med = torch::empty({d}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_rsel<T>((int)mode, ptr<T>(X), ptr<T>(out), ptr<unsigned int>(state),
                   mode == 2 ? f32(med) : nullptr, n, d, (int)f, cur_stream());
  });
  return out;
}

// colsel(X, mode, f, mu=, p=, gammas=): the objective of the coordinate-wise
// tailored attack (colsel.hip). X holds the n <= 64 honest rows, f >= 1 is
// the number of copies of mu + gamma p appended to every column, mode 0 the
// median and mode 1 the f-trimmed mean of those n + f values. Returns the
// f64 (T,) vector D[t] = sum_j (mu_j - A_j(gammas[t]))^2. mu is an input and
// need not be X's column mean. Values that are not finite rank as
// torch.sort ranks them (NaN last): D is non-finite where the rule keeps one.
// No host sync.
torch::Tensor colsel_objective(torch::Tensor X, int64_t mode, int64_t f,
                               torch::Tensor mu, torch::Tensor p,
                               torch::Tensor gammas) {
  check_matrix(X);
  TORCH_CHECK(mode == 0 || mode == 1,
              "colsel(mu=, p=, gammas=): expected mode 0 (median) or 1 "
              "(trimmed mean), got ", mode);
  const int64_t n = X.size(0), d = X.size(1);
  TORCH_CHECK(n >= 1 && n <= COORD_MAX_N, "colsel(mu=, p=, gammas=) supports ",
              "1 <= n <= ", COORD_MAX_N, ", got ", n);
  TORCH_CHECK(d >= 1, "colsel(mu=, p=, gammas=): expected d >= 1");
  TORCH_CHECK(f >= 1 && f <= INT_MAX / 2 && (mode == 0 || f < n),
              "colsel(mu=, p=, gammas=) needs f >= 1, and f < n for the "
              "trimmed mean, got n=", n, ", f=", f);
  TORCH_CHECK(mu.dim() == 1 && p.dim() == 1 && gammas.dim() == 1,
              "mu, p, gammas: expected vectors");
  check_f32_vector(mu, d, "mu");
  check_f32_vector(p, d, "p");
  const int64_t T = gammas.numel();
  TORCH_CHECK(T >= 1 && T <= COORD_MAX_TRIALS, "gammas: expected 1 to ",
              COORD_MAX_TRIALS, " values, got ", T);
  check_f32_vector(gammas, T, "gammas");
  TORCH_CHECK(mu.device() == X.device() && p.device() == X.device() &&
                  gammas.device() == X.device(),
              "mu, p, gammas: expected X's device");
  const int blocks = coord_objective_blocks((long)d);
  auto f64 = X.options().dtype(torch::kFloat64);
  auto part = torch::empty({(int64_t)blocks * COORD_MAX_TRIALS}, f64);
  auto out = torch::empty({T}, f64);
  by_dtype(X, [&](auto tag) {
    using T_ = TAG_T(tag);
    launch_coord_objective<T_>(ptr<T_>(X), f32(mu), f32(p), f32(gammas),
                               part.data_ptr<double>(), out.data_ptr<double>(),
                               (int)n, (long)d, (int)mode, (int)f, (int)T,
                               cur_stream());
  });
  return out;
}

torch::Tensor row_sqnorms(torch::Tensor X) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  auto out = torch::zeros({n}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_row_sqnorms<T>(ptr<T>(X), f32(out), n, d, cur_stream());
  });
  return out;
}

torch::Tensor row_center_sqdists(torch::Tensor X, torch::Tensor z) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_f32_vector(z, d, "z");
  auto out = torch::zeros({n}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_row_center_sqdists<T>(ptr<T>(X), f32(z), f32(out), n, d,
                                 cur_stream());
  });
  return out;
}

torch::Tensor row_scale(torch::Tensor X, torch::Tensor s) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_f32_vector(s, n, "s");
  auto out = torch::empty_like(X);
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_row_scale<T>(ptr<T>(X), f32(s), ptr<T>(out), n, d, cur_stream());
  });
  return out;
}

torch::Tensor mean_rows(torch::Tensor X, torch::Tensor idx) {
  check_matrix(X);
  check_i32(idx, 1, "idx");
  TORCH_CHECK(idx.numel() >= 1, "idx: expected at least one row");
  const long d = (long)X.size(1);
  const int k = (int)idx.numel();
  auto out = torch::empty({d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_mean_rows<T>(ptr<T>(X), i32(idx), k, ptr<T>(out), d, cur_stream());
  });
  return out;
}

// mean_rows(X, idx, count=c): the mean of rows idx[:c] with c an int32
// device scalar read by the kernel (no host sync); zeros when c is 0.
torch::Tensor mean_rows_counted(torch::Tensor X, torch::Tensor idx,
                                torch::Tensor count) {
  check_matrix(X);
  check_i32(idx, 1, "idx");
  TORCH_CHECK(idx.numel() >= 1 && idx.numel() <= INT_MAX,
              "idx: expected at least one row");
  TORCH_CHECK(count.is_cuda() && count.scalar_type() == torch::kInt32 &&
                  count.numel() == 1,
              "count: expected an int32 device scalar");
  TORCH_CHECK(idx.device() == X.device() && count.device() == X.device(),
              "idx, count: expected X's device");
  const long d = (long)X.size(1);
  const int k = (int)idx.numel();
  auto out = torch::empty({d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_mean_rows_counted<T>(ptr<T>(X), i32(idx), k, i32(count),
                                ptr<T>(out), d, cur_stream());
  });
  return out;
}

// mean_rows(X, idx, count=c, weights=w): the weighted mean
// sum_k w[idx[k]] x[idx[k]] / sum_k w[idx[k]] over k < c, w an f32 device
// vector with one weight per row of X; zeros when c or the weight sum is 0.
torch::Tensor mean_rows_counted_weighted(torch::Tensor X, torch::Tensor idx,
                                         torch::Tensor count,
                                         torch::Tensor weights) {
  check_matrix(X);
  check_i32(idx, 1, "idx");
  TORCH_CHECK(idx.numel() >= 1 && idx.numel() <= MAX_N_LDS,
              "mean_rows(weights=) supports 1 <= len(idx) <= ", MAX_N_LDS,
              ", got ", idx.numel());
  TORCH_CHECK(count.is_cuda() && count.scalar_type() == torch::kInt32 &&
                  count.numel() == 1,
              "count: expected an int32 device scalar");
  TORCH_CHECK(X.size(0) >= 1 && X.size(0) <= INT_MAX, "bad row count");
  check_f32_vector(weights, X.size(0), "weights");
  TORCH_CHECK(idx.device() == X.device() && count.device() == X.device() &&
                  weights.device() == X.device(),
              "idx, count, weights: expected X's device");
  const long d = (long)X.size(1);
  const int k = (int)idx.numel();
  auto out = torch::empty({d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_mean_rows_counted_weighted<T>(ptr<T>(X), i32(idx), k, i32(count),
                                         f32(weights), (int)X.size(0),
                                         ptr<T>(out), d, cur_stream());
  });
  return out;
}

torch::Tensor group_mean_rows(torch::Tensor X, torch::Tensor idx) {
  check_matrix(X);
  check_i32(idx, 2, "idx");
  const long d = (long)X.size(1);
  const int g = (int)idx.size(0);
  const int k = (int)idx.size(1);
  auto out = torch::empty({g, d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_group_mean_rows<T>(ptr<T>(X), i32(idx), g, k, ptr<T>(out), d,
                              cur_stream());
  });
  return out;
}

torch::Tensor bucket_mean(torch::Tensor X, torch::Tensor perm,
                          int64_t bucket) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_i32(perm, 1, "perm");
  TORCH_CHECK(perm.numel() == n, "perm: expected one entry per row");
  TORCH_CHECK(bucket >= 1);
  const int nb = (int)((n + bucket - 1) / bucket);
  auto out = torch::empty({nb, d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_bucket_mean<T>(ptr<T>(X), i32(perm), n, (int)bucket, nb,
                          ptr<T>(out), d, cur_stream());
  });
  return out;
}

torch::Tensor gram(torch::Tensor X) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  auto G = torch::zeros({n, n}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_gram<T>(ptr<T>(X), f32(G), n, d, cur_stream());
  });
  return G;
}

// gram(X, cols=c): the sampled centred Grams of DnC (gram.hip). cols is an
// int32 (niters, b) device tensor of column indices (clamped to [0, d));
// returns (Gc f32 (niters, n, n), bad int32 (niters, n)). Bitwise repeatable.
std::vector<torch::Tensor> gram_sampled(torch::Tensor X, torch::Tensor cols) {
  check_matrix(X);
  check_i32(cols, 2, "cols");
  TORCH_CHECK(cols.device() == X.device(), "cols: expected X's device");
  const int64_t n = X.size(0);
  const long d = (long)X.size(1);
  const int64_t niters = cols.size(0), b = cols.size(1);
  TORCH_CHECK(n >= 1 && n <= DNC_MAX_N, "gram(cols) supports 1 <= n <= ",
              DNC_MAX_N, ", got ", n);
  TORCH_CHECK(d >= 1, "gram(cols) needs at least one column");
  TORCH_CHECK(niters >= 1 && niters <= 65535 && b >= 1 && b <= (1 << 30),
              "cols: expected (niters, b) with 1 <= niters <= 65535 and ",
              "1 <= b <= 2^30, got (", niters, ", ", b, ")");
  int nchunks, tpc;
  dnc_gram_chunks((int)b, (int)niters, nchunks, tpc);
  auto part = torch::empty({niters * nchunks, n, n}, f32_like(X));
  auto badpart = torch::empty({niters * nchunks, n}, i32_like(X));
  auto Gc = torch::empty({niters, n, n}, f32_like(X));
  auto bad = torch::empty({niters, n}, i32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_gram_sampled<T>(ptr<T>(X), i32(cols), (int)n, d, (int)niters,
                           (int)b, f32(part), i32(badpart), f32(Gc), i32(bad),
                           cur_stream());
  });
  return {Gc, bad};
}

// Fused Krum selection: Gram -> q winner indices (one kernel, replaces
// the D2-build + two topk torch chains whose launch overhead caps the
// d-sharded multi-GPU scaling).
// iterative = true: the q picks of the Bulyan selection instead (each pick
// rescored among the rows still alive, then removed), int32 (q,) in pick
// order; every pick needs k = alive - f - 1 >= 1.
torch::Tensor krum_select(torch::Tensor G, int64_t f, int64_t q,
                          bool iterative) {
  check_gram(G, "G");
  const int n = (int)G.size(0);
  if (iterative) {
    TORCH_CHECK(n <= KRUM_ITER_MAX_N, "krum_select(iterative) supports n <= ",
                KRUM_ITER_MAX_N, ", got ", n);
    TORCH_CHECK(q >= 1 && f >= 0 && n - q - f >= 1,
                "krum_select(iterative) needs q >= 1, f >= 0, n - q - f >= 1");
    auto picks = torch::empty({q}, i32_like(G));
    launch_krum_select_iter(f32(G), n, (int)f, (int)q, i32(picks),
                            cur_stream());
    return picks;
  }
  TORCH_CHECK(n <= 512, "krum_select supports n <= 512");
  TORCH_CHECK(q >= 1 && q <= n && f >= 0 && n - f - 1 >= 1);
  auto idx = torch::empty({q}, i32_like(G));
  launch_krum_select(f32(G), n, (int)f, (int)q, i32(idx), nullptr,
                     cur_stream());
  return idx;
}

// krum_select(G, f, q, stats=, rule=[, gammas=]): the aggregator-tailored
// attack search (krumsel.hip). G is the f32 Gram of the n honest rows, stats
// the 2n + 1 statistics of little_fused(X, z, perturb), f >= 1 the number of
// copies of m(gamma) = mu + gamma p appended; rule 0 is Krum / Multi-Krum
// with q winners, rule 1 Bulyan (q ignored). With gammas (f32 device vector
// of B trial values): int32 (B,) flags, 1 where the rule still selects the
// malicious rows. Without: the f32 0-dim gamma found by the device grid
// search. No host sync either way.
torch::Tensor agr_search(torch::Tensor G, int64_t f, int64_t q,
                         torch::Tensor stats, int64_t rule,
                         c10::optional<torch::Tensor> gammas) {
  check_gram(G, "G");
  const int64_t n = G.size(0);
  TORCH_CHECK(rule == AGR_RULE_KRUM || rule == AGR_RULE_BULYAN,
              "rule: expected 0 (Krum / Multi-Krum) or 1 (Bulyan), got ", rule);
  TORCH_CHECK(f >= 1 && n >= 2 && f <= n,
              "krum_select(stats) needs f >= 1, n >= 2, f <= n, got n=", n,
              ", f=", f);
  TORCH_CHECK(n + f <= KRUM_ITER_MAX_N, "krum_select(stats) supports n + f <= ",
              KRUM_ITER_MAX_N, ", got ", n + f);
  if (rule == AGR_RULE_BULYAN) {
    TORCH_CHECK(n >= 3 * f + 3, "Bulyan needs n + f >= 4f + 3, got n=", n,
                ", f=", f);
  } else {
    TORCH_CHECK(q >= 1 && q <= n + f, "q: expected 1 <= q <= n + f, got ", q);
  }
  check_f32_vector(stats, 2 * n + 1, "stats");
  TORCH_CHECK(stats.device() == G.device(), "stats: expected G's device");
  if (gammas.has_value()) {
    const int64_t B = gammas->numel();
    TORCH_CHECK(B >= 1 && B <= 65535, "gammas: expected 1 to 65535 values");
    check_f32_vector(*gammas, B, "gammas");
    TORCH_CHECK(gammas->device() == G.device(), "gammas: expected G's device");
    auto flags = torch::empty({B}, i32_like(G));
    launch_agr_flags(f32(G), f32(stats), (int)n, (int)f, (int)q, (int)rule,
                     f32(*gammas), (int)B, i32(flags), cur_stream());
    return flags;
  }
  auto state = torch::empty({AGR_STATE_FLOATS}, f32_like(G));
  auto flags =
      torch::empty({AGR_GEO_POINTS + 2 * AGR_LIN_POINTS}, i32_like(G));
  auto gamma = torch::empty({}, f32_like(G));
  launch_agr_search(f32(G), f32(stats), (int)n, (int)f, (int)q, (int)rule,
                    f32(state), i32(flags), f32(gamma), cur_stream());
  return gamma;
}

// Sharded form of the Weiszfeld update: `dist2` holds the global squared
// distances (multi-GPU d-sharding: all-reduced over RCCL). Accumulates
// ||dz||^2 into `shift` (callers poll it every few iterations — no
// per-iteration sync).
torch::Tensor weiszfeld_apply(torch::Tensor X, torch::Tensor z,
                              torch::Tensor dist2, double eps,
                              torch::Tensor shift) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_rows_fit_lds(n, "weiszfeld_apply");
  check_f32_vector(z, d, "z");
  check_f32_vector(dist2, n, "dist2");
  check_f32_scalar(shift, "shift");
  auto z_new = torch::empty_like(z);
  shift.zero_();
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_weiszfeld_update<T>(ptr<T>(X), f32(z), f32(dist2), f32(z_new),
                               f32(shift), n, d, (float)eps, cur_stream());
  });
  return z_new;
}

// One Weiszfeld iteration: distance pass + the fused update above.
torch::Tensor weiszfeld_iter(torch::Tensor X, torch::Tensor z, double eps,
                             torch::Tensor shift) {
  check_matrix(X);
  check_rows_fit_lds(X.size(0), "weiszfeld_iter");
  check_f32_scalar(shift, "shift");
  return weiszfeld_apply(X, z, row_center_sqdists(X, z), eps, shift);
}

// Grouped Weiszfeld iteration: G independent (m, d) problems, one kernel
// pair per iteration for ALL groups (gossip rounds: every node's geomed
// advances together — no per-node streams, no launch storms).
torch::Tensor weiszfeld_iter_grouped(torch::Tensor X3, torch::Tensor Z,
                                     double eps) {
  TORCH_CHECK(X3.is_cuda() && X3.dim() == 3 && X3.is_contiguous() &&
              (X3.scalar_type() == torch::kFloat32 ||
               X3.scalar_type() == torch::kBFloat16),
              "expected contiguous (G, m, d) f32/bf16");
  const int G = (int)X3.size(0);
  const int m = (int)X3.size(1);
  const long d = (long)X3.size(2);
  TORCH_CHECK(m >= 1 && m <= 32, "grouped weiszfeld supports m <= 32");
  check_f32_vector(Z, (int64_t)G * d, "Z");
  TORCH_CHECK(Z.dim() == 2 && Z.size(0) == G, "Z: expected (G, d)");
  auto dist2 = torch::zeros({G, m}, f32_like(X3));
  auto Z_new = torch::empty_like(Z);
  by_dtype(X3, [&](auto tag) {
    using T = TAG_T(tag);
    launch_grouped_weiszfeld<T>(ptr<T>(X3), f32(Z), f32(dist2), f32(Z_new), G,
                                m, d, (float)eps, cur_stream());
  });
  return Z_new;
}

// Sharded form of the centered-clipping update (dist2 reduced externally).
torch::Tensor cc_apply(torch::Tensor X, torch::Tensor v, torch::Tensor dist2,
                       double c_tau, double eps) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_rows_fit_lds(n, "cc_apply");
  check_f32_vector(v, d, "v");
  check_f32_vector(dist2, n, "dist2");
  auto v_new = torch::empty_like(v);
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_cc_update<T>(ptr<T>(X), f32(v), f32(dist2), f32(v_new), n, d,
                        (float)c_tau, (float)eps, cur_stream());
  });
  return v_new;
}

torch::Tensor cc_iter(torch::Tensor X, torch::Tensor v, double c_tau,
                      double eps) {
  check_matrix(X);
  check_rows_fit_lds(X.size(0), "cc_iter");
  return cc_apply(X, v, row_center_sqdists(X, v), c_tau, eps);
}

// Little attack fused: per-column mu + z*sigma in one streaming pass.
torch::Tensor little_fused(torch::Tensor X, double z) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  auto out = torch::empty({d}, X.options());
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_little<T>(ptr<T>(X), ptr<T>(out), n, d, (float)z, cur_stream());
  });
  return out;
}

// little_fused(X, z, perturb): the statistics pass of the Min-Max / Min-Sum
// attacks instead. perturb: 0 unit, 1 std, 2 sign; z is unused. Returns
// (mu, p, stats), all f32: the column mean, the perturbation direction and
// stats = [a_0..a_{n-1}, b_0..b_{n-1}, c] (launchers.h).
std::vector<torch::Tensor> little_fused_stats(torch::Tensor X, double /*z*/,
                                              int64_t perturb) {
  check_matrix(X);
  const int64_t n = X.size(0);
  const long d = (long)X.size(1);
  TORCH_CHECK(n >= 1, "little_fused(perturb) needs at least one row");
  check_rows_fit_lds(n, "little_fused(perturb)");
  TORCH_CHECK(perturb >= 0 && perturb <= 2,
              "perturb: expected 0 (unit), 1 (std) or 2 (sign), got ", perturb);
  auto mu = torch::empty({d}, f32_like(X));
  auto p = torch::empty({d}, f32_like(X));
  auto stats = torch::zeros({2 * n + 1}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_attack_stats<T>(ptr<T>(X), f32(mu), f32(p), f32(stats), (int)n, d,
                           (int)perturb, cur_stream());
  });
  return {mu, p, stats};
}

// Philox4x32-10 + Box-Muller N(mu, sigma^2) fill (no torch RNG).
torch::Tensor gaussian_fill(int64_t d, int64_t seed, double mu, double sigma,
                            torch::Tensor like) {
  TORCH_CHECK(like.is_cuda(), "gaussian_fill needs a device template");
  TORCH_CHECK(like.scalar_type() == torch::kFloat32 ||
                  like.scalar_type() == torch::kBFloat16,
              "expected f32 or bf16");
  TORCH_CHECK(d >= 1);
  auto out = torch::empty({d}, like.options());
  by_dtype(like, [&](auto tag) {
    using T = TAG_T(tag);
    launch_gaussian_fill<T>(ptr<T>(out), d, (unsigned long long)seed,
                            (float)mu, (float)sigma, cur_stream());
  });
  return out;
}

// SMEA subset selection fully on device (subsets.hip): returns the
// winning combo INDEX packed in the low 32 bits of a u64 key tensor.
torch::Tensor smea_select(torch::Tensor G, torch::Tensor combos) {
  check_gram(G, "G");
  check_i32(combos, 2, "combos");
  const int n = (int)G.size(0);
  const int C = (int)combos.size(0);
  const int m = (int)combos.size(1);
  TORCH_CHECK(m >= 1 && m <= 64 && C >= 1);
  auto best = torch::full({1}, -1, G.options().dtype(torch::kInt64));
  launch_smea_select(f32(G), i32(combos), n, m, C,
                     ptr<unsigned long long>(best), cur_stream());
  return best;
}

// smea_select(Gc3, bad, keep): the DnC spectral selection (subsets.hip) on
// the (niters, n, n) sampled centred Grams and their (niters, n) bad flags.
// Returns (idx int32 (n,), count int32 ()): idx[:count] are the ascending
// indices kept by every iteration, the rest is padding. No host sync.
std::vector<torch::Tensor> dnc_select(torch::Tensor Gc3, torch::Tensor bad,
                                      int64_t keep) {
  TORCH_CHECK(Gc3.is_cuda() && Gc3.dim() == 3 && Gc3.size(1) == Gc3.size(2) &&
                  Gc3.scalar_type() == torch::kFloat32 && Gc3.is_contiguous(),
              "Gc3: expected an f32 contiguous device tensor (niters, n, n)");
  const int64_t niters = Gc3.size(0), n = Gc3.size(1);
  TORCH_CHECK(niters >= 1 && niters <= 65535, "Gc3: expected 1 <= niters <= ",
              "65535, got ", niters);
  TORCH_CHECK(n >= 1 && n <= DNC_MAX_N, "smea_select(Gc3, bad, keep) supports ",
              "1 <= n <= ", DNC_MAX_N, ", got ", n);
  check_i32(bad, 2, "bad");
  TORCH_CHECK(bad.size(0) == niters && bad.size(1) == n &&
                  bad.device() == Gc3.device(),
              "bad: expected (", niters, ", ", n, ") on Gc3's device");
  TORCH_CHECK(keep >= 1 && keep <= n, "keep: expected 1 <= keep <= ", n,
              ", got ", keep);
  auto kept = torch::empty({niters, n}, i32_like(Gc3));
  auto idx = torch::empty({n}, i32_like(Gc3));
  auto count = torch::empty({}, i32_like(Gc3));
  launch_dnc_select(f32(Gc3), i32(bad), (int)niters, (int)n, (int)keep,
                    i32(kept), i32(idx), i32(count), cur_stream());
  return {idx, count};
}

// smea_select(G, weights=w, xi=, delta_xi=): the AFA selection (subsets.hip)
// on the f32 Gram G (n, n) with row weights w (n,), one launch for the whole
// data-dependent loop. Returns (idx int32 (n,), count int32 (), rounds int32
// ()): idx[:count] are the ascending indices still alive, the rest is
// padding; rounds is the number of loop passes. No host sync.
std::vector<torch::Tensor> afa_select(torch::Tensor G, torch::Tensor weights,
                                      double xi, double delta_xi) {
  check_gram(G, "G");
  const int64_t n = G.size(0);
  TORCH_CHECK(n >= 1 && n <= AFA_MAX_N, "smea_select(G, weights=) supports ",
              "1 <= n <= ", AFA_MAX_N, ", got ", n);
  TORCH_CHECK(weights.dim() == 1, "weights: expected one dimension, got ",
              weights.dim());
  check_f32_vector(weights, n, "weights");
  TORCH_CHECK(weights.device() == G.device(), "weights: expected G's device");
  TORCH_CHECK(xi >= 0.0 && xi < INFINITY, "xi: expected a finite value >= 0, ",
              "got ", xi);
  TORCH_CHECK(delta_xi >= 0.0 && delta_xi < INFINITY,
              "delta_xi: expected a finite value >= 0, got ", delta_xi);
  auto idx = torch::empty({n}, i32_like(G));
  auto count = torch::empty({}, i32_like(G));
  auto rounds = torch::empty({}, i32_like(G));
  launch_afa_select(f32(G), f32(weights), (int)n, xi, delta_xi, i32(idx),
                    i32(count), i32(rounds), cur_stream());
  return {idx, count, rounds};
}

// MDA two-pass device search: returns (found[npairs], subsets[npairs, m]);
// the first found prefix (pair-lex order) holds the lex-smallest optimal
// subset. No host sync anywhere.
// (A centrality-permuted pass-1 variant measured 15x SLOWER — central-first
// lex order wanders near-optimal subtrees B&B cannot prune — so pass 1
// walks prefixes in plain index order.)
std::vector<torch::Tensor> mda_select(torch::Tensor D2, int64_t f,
                                      c10::optional<torch::Tensor> ub) {
  check_gram(D2, "D2");
  const int n = (int)D2.size(0);
  const int m = n - (int)f;
  TORCH_CHECK(n <= 64, "mda_select supports n <= 64");
  TORCH_CHECK(m >= 2 && m <= n, "mda_select needs 2 <= n - f <= n");
  // P-element lexicographic prefixes: triples when the subset is deep
  // enough (finer decomposition = shorter serial DFS tails), else pairs
  const int P = (m >= 3 && n >= 8) ? 3 : 2;
  long npre = 0;
  if (P == 2) {
    npre = (long)n * (n - 1) / 2;
  } else {
    npre = (long)n * (n - 1) * (n - 2) / 6;
  }
  auto pre_cpu = torch::empty({npre, (long)P}, torch::kInt32);
  {
    auto acc = pre_cpu.accessor<int, 2>();
    long k = 0;
    if (P == 2) {
      for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
          acc[k][0] = a;
          acc[k][1] = b;
          ++k;
        }
    } else {
      for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
          for (int c = b + 1; c < n; ++c) {
            acc[k][0] = a;
            acc[k][1] = b;
            acc[k][2] = c;
            ++k;
          }
    }
  }
  auto prefixes = pre_cpu.to(D2.device());
  // init = monotone key of +inf (0xFF800000), NOT 0xFFFFFFFF: the
  // all-ones pattern decodes to NaN and every comparison goes false.
  // An optional achievable upper bound seeds the key so pass 1 prunes
  // from the start (one ulp up so strict < can re-find an exact tie).
  torch::Tensor best;
  if (ub.has_value()) {
    check_f32_scalar(*ub, "ub");
    auto bits = torch::nan_to_num(ub.value(), 0.0, 3.0e38, 0.0)
                    .view(torch::kInt32);
    best = (bits + 1).bitwise_or((int)0x80000000).contiguous();
  } else {
    best = torch::full({1}, (int)0xFF800000, i32_like(D2));
  }
  auto subsets = torch::zeros({npre, (long)m}, i32_like(D2));
  auto found = torch::zeros({npre}, i32_like(D2));
  auto* bp = ptr<unsigned int>(best);
  launch_mda_pass1(f32(D2), i32(prefixes), P, n, m, (int)npre, bp,
                   cur_stream());
  launch_mda_pass2(f32(D2), i32(prefixes), P, n, m, (int)npre, bp,
                   i32(subsets), i32(found), cur_stream());
  return {found, subsets};
}

// -- CAF fused power-iteration pair --------------------------

torch::Tensor caf_matvec(torch::Tensor X, torch::Tensor mu, torch::Tensor v) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_f32_vector(mu, d, "mu");
  check_f32_vector(v, d, "v");
  auto out = torch::zeros({n}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_caf_matvec<T>(ptr<T>(X), f32(mu), f32(v), f32(out), n, d,
                         cur_stream());
  });
  return out;
}

torch::Tensor caf_colsum(torch::Tensor X, torch::Tensor a,
                         c10::optional<torch::Tensor> mu,
                         c10::optional<torch::Tensor> scale) {
  check_matrix(X);
  const int n = (int)X.size(0);
  const long d = (long)X.size(1);
  check_rows_fit_lds(n, "caf_colsum");
  check_f32_vector(a, n, "a");
  if (mu.has_value()) check_f32_vector(*mu, d, "mu");
  if (scale.has_value()) check_f32_scalar(*scale, "scale");
  const float* mu_p = mu.has_value() ? f32(*mu) : nullptr;
  const float* sc_p = scale.has_value() ? f32(*scale) : nullptr;
  auto out = torch::empty({d}, f32_like(X));
  by_dtype(X, [&](auto tag) {
    using T = TAG_T(tag);
    launch_caf_colsum<T>(ptr<T>(X), f32(a), mu_p, sc_p, f32(out), n, d,
                         cur_stream());
  });
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("colsel", &colsel, "columnwise median/trimmed-mean/meamed",
        py::arg("X"), py::arg("mode"), py::arg("f"),
        py::arg("rows") = c10::nullopt, py::kw_only(),
        py::arg("gram") = c10::nullopt);
  m.def("colsel", &colsel_objective,
        "coordinate-wise tailored attack objective: f64 D per trial gamma",
        py::arg("X"), py::arg("mode"), py::arg("f"), py::kw_only(),
        py::arg("mu"), py::arg("p"), py::arg("gammas"));
  m.def("row_sqnorms", &row_sqnorms);
  m.def("row_center_sqdists", &row_center_sqdists);
  m.def("row_scale", &row_scale);
  m.def("mean_rows", &mean_rows);
  m.def("mean_rows", &mean_rows_counted,
        "mean of rows idx[:count], count an int32 device scalar (K15)",
        py::arg("X"), py::arg("idx"), py::kw_only(), py::arg("count"));
  m.def("mean_rows", &mean_rows_counted_weighted,
        "weighted mean of rows idx[:count], one f32 weight per row of X (K16)",
        py::arg("X"), py::arg("idx"), py::kw_only(), py::arg("count"),
        py::arg("weights"));
  m.def("group_mean_rows", &group_mean_rows);
  m.def("bucket_mean", &bucket_mean);
  m.def("gram", &gram);
  m.def("gram", &gram_sampled,
        "sampled centred Grams of DnC (K15): (Gc, bad)", py::arg("X"),
        py::kw_only(), py::arg("cols"));
  m.def("krum_select", &krum_select, py::arg("G"), py::arg("f"), py::arg("q"),
        py::arg("iterative") = false);
  m.def("krum_select", &agr_search,
        "aggregator-tailored attack search (K14): flags, or gamma",
        py::arg("G"), py::arg("f"), py::arg("q"), py::kw_only(),
        py::arg("stats"), py::arg("rule"), py::arg("gammas") = c10::nullopt);
  m.def("caf_matvec", &caf_matvec);
  m.def("caf_colsum", &caf_colsum, py::arg("X"), py::arg("a"),
        py::arg("mu") = c10::nullopt, py::arg("scale") = c10::nullopt);
  m.def("weiszfeld_iter", &weiszfeld_iter);
  m.def("weiszfeld_iter_grouped", &weiszfeld_iter_grouped,
        "one Weiszfeld iteration for G independent (m, d) groups");
  m.def("weiszfeld_apply", &weiszfeld_apply);
  m.def("cc_iter", &cc_iter);
  m.def("cc_apply", &cc_apply);
  m.def("mda_search", &mda_search, "exact min-diameter subset (host DFS)");
  m.def("smea_select", &smea_select, "device SMEA subset selection (K11)");
  m.def("smea_select", &dnc_select,
        "DnC spectral selection (K15): (idx, count)", py::arg("Gc3"),
        py::arg("bad"), py::arg("keep"));
  m.def("smea_select", &afa_select,
        "AFA selection (K16): (idx, count, rounds)", py::arg("G"),
        py::kw_only(), py::arg("weights"), py::arg("xi"), py::arg("delta_xi"));
  m.def("little_fused", &little_fused, "fused Little attack (K14)");
  m.def("little_fused", &little_fused_stats,
        "Min-Max / Min-Sum statistics pass (K14): (mu, p, stats)",
        py::arg("X"), py::arg("z"), py::arg("perturb"));
  m.def("gaussian_fill", &gaussian_fill, "philox gaussian fill (K14)");
  m.def("mda_select", &mda_select, "device MDA two-pass B&B search (K11)",
        py::arg("D2"), py::arg("f"), py::arg("ub") = c10::nullopt);
}
