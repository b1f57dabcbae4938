// csrc/dendrogram_plan.h on its own (tests/test_dendrogram_cuts_cpu.py builds this with -fsanitize=address,undefined):
// the plan of a chain of depth n - 1, of the two-leaf tree and of a random tree is a permutation of the nodes with
// every position in range, cuts made from it by the two scans agree with a direct walk of the tree, and matrices that
// are no tree are refused without touching memory they should not.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dendrogram_plan.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("line %d: %s\n", __LINE__, #cond);                   \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// fcluster(Z, t, "distance") the slow way: SciPy's cluster_monocrit written recursively (small trees only)
struct Walk {
  const double* Z;
  int n;
  std::vector<double> md;
  std::vector<int> label;
  int count = 0;
  double md_of(int i) {
    double m = Z[4 * i + 2];
    for (int s = 0; s < 2; ++s) {
      const int c = (int)Z[4 * i + s];
      if (c >= n && md[c - n] > m) m = md[c - n];
    }
    return m;
  }
  void visit(int i, double t, bool inside) {
    if (!inside && md[i] <= t) {
      inside = true;
      ++count;
    }
    const int a = (int)Z[4 * i], b = (int)Z[4 * i + 1];
    if (a >= n) visit(a - n, t, inside);
    if (b >= n) visit(b - n, t, inside);
    if (a < n) label[a] = inside ? count : ++count;
    if (b < n) label[b] = inside ? count : ++count;
  }
  std::vector<int> cut(double t) {
    md.assign(n - 1, 0.0);
    for (int i = 0; i < n - 1; ++i) md[i] = md_of(i);
    label.assign(n, 0);
    count = 0;
    visit(n - 2, t, false);
    return label;
  }
};

static std::vector<int> cut_from_plan(int n, const std::vector<double>& own, const std::vector<double>& parent,
                                      const std::vector<int32_t>& lo, const std::vector<int32_t>& leaf_lo, double t) {
  std::vector<int> pos(n, 0), out(n);
  int number = 0;
  for (int s = 0; s < 2 * n - 1; ++s)
    if (own[s] <= t && t < parent[s]) pos[lo[s]] = ++number;
  for (int p = 1; p < n; ++p)
    if (pos[p] == 0) pos[p] = pos[p - 1];
  for (int l = 0; l < n; ++l) out[l] = pos[leaf_lo[l]];
  return out;
}

static void check_tree(const std::vector<double>& Z, int n, bool walk) {
  std::vector<double> own(2 * n - 1), parent(2 * n - 1);
  std::vector<int32_t> lo(2 * n - 1), leaf_lo(n);
  EXPECT(pa::dendrogram_plan(Z.data(), n, own.data(), parent.data(), lo.data(), leaf_lo.data()) == 0);
  std::vector<char> seen(n, 0);
  for (int l = 0; l < n; ++l) {
    EXPECT(leaf_lo[l] >= 0 && leaf_lo[l] < n && !seen[leaf_lo[l]]);
    if (leaf_lo[l] >= 0 && leaf_lo[l] < n) seen[leaf_lo[l]] = 1;
  }
  int leaves = 0;
  for (int s = 0; s < 2 * n - 1; ++s) {
    EXPECT(lo[s] >= 0 && lo[s] < n);
    EXPECT(own[s] <= parent[s]);
    leaves += isinf(own[s]) && own[s] < 0;
  }
  EXPECT(leaves == n);
  EXPECT(own[0] >= Z[4 * (n - 2) + 2] && isinf(parent[0]) && lo[0] == 0);   // the root comes first
  if (!walk) return;
  Walk w{Z.data(), n};
  for (int i = -1; i < n - 1; ++i) {
    const double h = i < 0 ? -1.0 : Z[4 * i + 2];
    for (double t : {h, nextafter(h, -INFINITY), h + 0.5}) {
      EXPECT(cut_from_plan(n, own, parent, lo, leaf_lo, t) == w.cut(t));
    }
  }
}

int main() {
  // the two-leaf tree
  check_tree({0, 1, 0.25, 2}, 2, true);
  // a chain: merge i joins leaf i + 1 to everything so far, alternately as the left and the right child
  for (int n : {3, 64, 200000}) {
    std::vector<double> Z(4 * (size_t)(n - 1));
    for (int i = 0; i < n - 1; ++i) {
      const double big = i == 0 ? 0 : n + i - 1, leaf = i + 1;
      Z[4 * (size_t)i] = (i & 1) ? leaf : big;
      Z[4 * (size_t)i + 1] = (i & 1) ? big : leaf;
      Z[4 * (size_t)i + 2] = 1.0 + i;
      Z[4 * (size_t)i + 3] = i + 2;
    }
    check_tree(Z, n, n <= 64);
  }
  // random trees with inversions (heights are not sorted) and ties
  srand(7);
  for (int n : {5, 33, 130}) {
    std::vector<double> Z(4 * (size_t)(n - 1));
    std::vector<int> roots(n);
    for (int l = 0; l < n; ++l) roots[l] = l;
    for (int i = 0; i < n - 1; ++i) {
      const int a = rand() % roots.size();
      const int va = roots[a];
      roots.erase(roots.begin() + a);
      const int b = rand() % roots.size();
      const int vb = roots[b];
      roots[b] = n + i;
      Z[4 * (size_t)i] = va;
      Z[4 * (size_t)i + 1] = vb;
      Z[4 * (size_t)i + 2] = (rand() % 16) * 0.25;
      Z[4 * (size_t)i + 3] = 0;     // (the sizes are counted from the tree)
    }
    check_tree(Z, n, true);
  }
  // no trees
  {
    std::vector<double> own(5), parent(5);
    std::vector<int32_t> lo(5), leaf_lo(3);
    const double used_twice[] = {0, 1, 1.0, 2, 0, 2, 2.0, 3};
    const double not_formed[] = {0, 4, 1.0, 2, 1, 2, 2.0, 3};
    const double fraction[] = {0, 1.5, 1.0, 2, 3, 2, 2.0, 3};
    const double negative[] = {0, -1, 1.0, 2, 3, 2, 2.0, 3};
    const double huge[] = {0, 1e300, 1.0, 2, 3, 2, 2.0, 3};
    const double not_a_number[] = {0, NAN, 1.0, 2, 3, 2, 2.0, 3};
    for (const double* Z : {used_twice, not_formed, fraction, negative, huge, not_a_number})
      EXPECT(pa::dendrogram_plan(Z, 3, own.data(), parent.data(), lo.data(), leaf_lo.data()) == 3);
    EXPECT(pa::dendrogram_plan(used_twice, 1, own.data(), parent.data(), lo.data(), leaf_lo.data()) == 3);
    EXPECT(pa::dendrogram_plan(nullptr, 3, own.data(), parent.data(), lo.data(), leaf_lo.data()) == 3);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
