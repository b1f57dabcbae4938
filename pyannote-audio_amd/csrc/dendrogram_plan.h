// Everything about a dendrogram that every flat cut of it shares (host, plain C++: this header is also compiled on
// its own by tests/native/dendrogram_plan_harness.cpp).
//
// scipy.cluster.hierarchy.fcluster(Z, t, "distance") = cluster_monocrit(Z, MD, t) with MD[i] the largest merge height
// in the subtree of merge i (get_max_dist_for_each_cluster; with the inversions of centroid / median linkage MD is
// monotone along a path to the root where Z[:, 2] is not).  cluster_monocrit walks the tree depth first -- left
// internal child, right internal child, then the node's own leaves, left before right -- and hands out a new number
//   * when it ENTERS an internal node i with MD[i] <= t and no ancestor has started a cluster, and
//   * when it reaches a leaf (which is when it LEAVES the leaf's parent) and no ancestor has started a cluster.
// So a node v starts a flat cluster iff own_md[v] <= t < parent_md[v] (own_md = -inf for a leaf, parent_md = +inf
// for the root), and its number is the count of starting nodes up to and including v on the TIMELINE of those
// 2n - 1 events.  The timeline is not the left-to-right leaf order: a leaf is numbered after the whole internal
// sibling subtree even when it is the left child.  The plan lists the nodes in timeline order with the two heights
// and `lo`, the first position of the node's leaves in left-first leaf order (a subtree's leaves are contiguous
// there); a cut is then two prefix scans (csrc/dendrogram.hip, clustering.Dendrogram.cuts).
#pragma once
#include <stdint.h>

#include <limits>
#include <new>
#include <vector>

namespace pa {

// Z: (n - 1, 4) float64 SciPy linkage matrix, n >= 2.  Outputs, all written in full:
//   tl_own, tl_parent (2n - 1) float64 and tl_lo (2n - 1) int32, indexed by timeline slot;  leaf_lo (n) int32, by leaf.
// Every tl_lo / leaf_lo value lies in 0..n-1 (sizes are counted from the tree, Z[:, 3] is not trusted).
// Returns 0, 2 (out of memory) or 3 (not a tree: a child id that is no integer, out of range, not yet formed or
// used twice).  The depth-first walk keeps its own stack: a single-linkage chain is n - 1 deep.
inline int dendrogram_plan(const double* Z, int n, double* tl_own, double* tl_parent, int32_t* tl_lo,
                           int32_t* leaf_lo) {
  if (Z == nullptr || n < 2) return 3;
  const int m = n - 1, nodes = 2 * n - 1;
  const double inf = std::numeric_limits<double>::infinity();
  try {
    std::vector<int32_t> child(2 * (size_t)m), size(nodes, 1), lo(nodes), slot(nodes), stack(m);
    std::vector<double> own(nodes, -inf), parent(nodes, inf);
    std::vector<uint8_t> used(nodes, 0), state(m, 0);
    // bottom up (a child is formed before its parent): validity, sizes, MD
    for (int i = 0; i < m; ++i) {
      double md = Z[4 * (size_t)i + 2];
      for (int side = 0; side < 2; ++side) {
        const double c = Z[4 * (size_t)i + side];
        if (!(c >= 0.0 && c < (double)(n + i))) return 3;
        const int32_t v = (int32_t)c;
        if ((double)v != c || used[v]) return 3;
        used[v] = 1;
        child[2 * (size_t)i + side] = v;
        if (v >= n && own[v] > md) md = own[v];   // (SciPy's comparison: a NaN height never wins)
      }
      own[n + i] = md;
      size[n + i] = size[child[2 * (size_t)i]] + size[child[2 * (size_t)i + 1]];
    }
    // top down: the parent's MD and the first leaf position
    lo[nodes - 1] = 0;
    for (int i = m - 1; i >= 0; --i) {
      const int32_t a = child[2 * (size_t)i], b = child[2 * (size_t)i + 1];
      parent[a] = parent[b] = own[n + i];
      lo[a] = lo[n + i];
      lo[b] = lo[n + i] + size[a];
    }
    // the timeline
    int k = 0, next = 0;
    stack[0] = nodes - 1;
    while (k >= 0) {
      const int32_t v = stack[k], i = v - n;
      const int32_t a = child[2 * (size_t)i], b = child[2 * (size_t)i + 1];
      if (state[i] == 0) {
        slot[v] = next++;
        state[i] = 1;
        if (a >= n) {
          stack[++k] = a;
          continue;
        }
      }
      if (state[i] == 1) {
        state[i] = 2;
        if (b >= n) {
          stack[++k] = b;
          continue;
        }
      }
      if (a < n) slot[a] = next++;
      if (b < n) slot[b] = next++;
      --k;
    }
    if (next != nodes) return 3;
    for (int v = 0; v < nodes; ++v) {
      const int32_t s = slot[v];
      tl_own[s] = own[v];
      tl_parent[s] = parent[v];
      tl_lo[s] = lo[v];
    }
    for (int l = 0; l < n; ++l) leaf_lo[l] = lo[l];
  } catch (const std::bad_alloc&) {
    return 2;
  }
  return 0;
}

}  // namespace pa
