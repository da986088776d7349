// Host side of the MDA subset search: the exact
// branch-and-bound fallback that runs on the CPU copy of the distance
// matrix. No device code; bound as _hip_ops.mda_search by bind.cpp.
#include "mda_host.h"

#include <algorithm>
#include <functional>
#include <limits>
#include <vector>

// Exact minimum-diameter (n-f)-subset search (MDA) — HOST code: the n x n
// squared-distance matrix is tiny; the combinatorial DFS belongs in native
// C++, not Python (reference ran a seeded-DFS process pool for this,
// minimum_diameter_average.py:267-386). Branch-and-bound over candidates
// ordered by greedy insertion cost, seeded with a greedy upper bound.
torch::Tensor mda_search(torch::Tensor D2in, int64_t f) {
  TORCH_CHECK(!D2in.is_cuda(), "mda_search runs on the host copy of D2");
  auto D2 = D2in.to(torch::kFloat64).contiguous();
  const int n = (int)D2.size(0);
  const int m = n - (int)f;
  TORCH_CHECK(m >= 1 && D2.size(1) == n);
  auto D = D2.accessor<double, 2>();

  // greedy seed: for each anchor row, grow the subset by min-added-diameter
  double best_diam = std::numeric_limits<double>::infinity();
  std::vector<int> best;
  std::vector<int> cur;
  std::vector<double> maxd(n);
  for (int a = 0; a < n; ++a) {
    cur.assign(1, a);
    std::fill(maxd.begin(), maxd.end(), 0.0);
    std::vector<char> used(n, 0);
    used[a] = 1;
    for (int j = 0; j < n; ++j) maxd[j] = D[a][j];
    double diam = 0.0;
    for (int step = 1; step < m; ++step) {
      int pick = -1;
      double pick_cost = std::numeric_limits<double>::infinity();
      for (int j = 0; j < n; ++j)
        if (!used[j] && (pick < 0 || maxd[j] < pick_cost)) {
          pick_cost = maxd[j];  // pick < 0: rows at +inf are candidates too
          pick = j;
        }
      used[pick] = 1;
      cur.push_back(pick);
      diam = std::max(diam, pick_cost);
      for (int j = 0; j < n; ++j) maxd[j] = std::max(maxd[j], D[pick][j]);
    }
    if (diam < best_diam) { best_diam = diam; best = cur; }
  }

  // exact DFS with prefix-max pruning (candidates in greedy-friendly order)
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  // order by row-sum of distances: central rows first
  std::vector<double> rowsum(n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) rowsum[i] += D[i][j];
  std::sort(order.begin(), order.end(),
            [&](int a, int b) { return rowsum[a] < rowsum[b]; });

  // A node lists its viable candidates first: those compatible with every
  // chosen row at the current bound. A completion needs `need` of them, so
  // fewer ends the node. Counting positions alone (oi <= n - need) lets the
  // search wander through subsets of a tight cluster that has too few rows
  // left, which is exponential when the rows it cannot use sort last.
  std::vector<int> chosen;
  chosen.reserve(m);
  std::vector<std::vector<std::pair<int, double>>> viable(m + 1);
  std::function<void(int, double)> dfs = [&](int start, double diam) {
    if ((int)chosen.size() == m) {
      if (diam < best_diam) { best_diam = diam; best = chosen; }
      return;
    }
    const int need = m - (int)chosen.size();
    auto& cands = viable[chosen.size()];
    cands.clear();
    for (int oi = start; oi < n; ++oi) {
      const int j = order[oi];
      double dj = diam;
      for (int c : chosen) dj = std::max(dj, D[c][j]);
      if (dj < best_diam) cands.emplace_back(oi, dj);
    }
    for (int k = 0; k + need <= (int)cands.size(); ++k) {
      const double dj = cands[k].second;
      if (dj >= best_diam) continue;  // the bound fell since the listing
      chosen.push_back(order[cands[k].first]);
      dfs(cands[k].first + 1, dj);
      chosen.pop_back();
    }
  };
  dfs(0, 0.0);

  // Canonicalize: among all subsets achieving best_diam, return the
  // lexicographically smallest (optimal subsets are generically non-unique
  // — every subset containing the binding edge ties). Pure index-order DFS
  // with the now-tight bound; the first complete subset found is the
  // lexicographic minimum.
  const double bound = best_diam;
  std::vector<int> lex;
  lex.reserve(m);
  bool found = false;
  std::vector<std::vector<int>> viable2(m + 1);
  std::function<void(int)> dfs2 = [&](int start) {
    if (found) return;
    if ((int)lex.size() == m) { best = lex; found = true; return; }
    const int need = m - (int)lex.size();
    auto& cands = viable2[lex.size()];
    cands.clear();
    for (int j = start; j < n; ++j) {
      bool ok = true;
      for (int c : lex)
        if (!(D[c][j] <= bound)) { ok = false; break; }
      if (ok) cands.push_back(j);
    }
    for (int k = 0; k + need <= (int)cands.size() && !found; ++k) {
      lex.push_back(cands[k]);
      dfs2(cands[k] + 1);
      lex.pop_back();
    }
  };
  dfs2(0);

  std::sort(best.begin(), best.end());
  auto out = torch::empty({(long)best.size()}, torch::kInt64);
  auto acc = out.accessor<int64_t, 1>();
  for (size_t i = 0; i < best.size(); ++i) acc[i] = best[i];
  return out;
}
