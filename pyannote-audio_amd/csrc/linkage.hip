// Centroid-linkage dendrogram on gfx950, bit-identical to scipy.cluster.hierarchy.linkage(y, "centroid")
// (SciPy 1.15.3 `_hierarchy.fast_linkage` = Muellner's "generic clustering algorithm" with a
//  nearest-neighbour candidate per row and a binary min-heap of lower bounds), which is what
//  AgglomerativeClustering.cluster calls (reference: pipelines/clustering.py:374-382).
//
// Why a kernel: the merge loop is inherently serial (N-1 dependent merges) but every merge does O(N)
// independent work -- Lance-Williams update of one row/column of the distance matrix, two
// nearest-neighbour row scans, the lower-bound refresh -- which SciPy walks on one host core
// (0.8 s for N = 7 000, the Amdahl term of the whole pipeline).  Here ONE persistent 1024-thread
// workgroup keeps the condensed matrix in HBM/L2 (it is produced there by k_pdist_f64 and never
// crosses PCIe), runs the O(N) parts data-parallel and leaves only the heap sifts (O(log N)) to lane 0.
//
// ONE kernel, k_linkage_centroid<IT, LDS_HEAP>: a single workgroup, plain loads and stores, __syncthreads
// between the phases of a merge; nothing in it waits for another workgroup.  Heap + neighbour candidates
// live in LDS with 16-bit keys up to N = 11 054, in global memory with int keys above.  The heap-free
// merge of linkage_fast.hip runs in front of it and completes tie-free inputs on several workgroups; this
// kernel is its gated fallback, the exact replay of SciPy's heap for inputs with exact ties.
//
// Exactness contract (tests/test_pipeline_gpu.py::test_linkage_*): same merge order, same float64
// heights, same tie behaviour as SciPy, because
//   * the distance update is SciPy's expression evaluated left to right in double with separately
//     rounded operations (lk_centroid_dist; this file is compiled with -ffp-contract=off);
//   * row scans return the FIRST index attaining the minimum (SciPy scans with a strict `<`);
//   * all heap operations (build, change_value, remove_min, sift_up/down) are executed by one lane in
//     exactly SciPy's order, including the ascending-z order of the lower-bound refresh.
// hipcc-flags: -ffp-contract=off
#include "common.h"

namespace pa {

constexpr int LK_T = 1024;  // threads (16 waves)
constexpr int LK_W = LK_T / 64;

__device__ __forceinline__ long cidx(long n, long i, long j) {
  // scipy condensed_index(n, i, j)
  return i < j ? n * i - (i * (i + 1) / 2) + (j - i - 1) : n * j - (j * (j + 1) / 2) + (i - j - 1);
}

// SciPy's Heap (scipy/cluster/_structures.pxi) with "hole" sifts: the moving element is held in
// registers and written once at its final position.  The final arrays are identical to the
// swap-by-swap version (same comparisons, same order), at ~1/3 of the dependent LDS traffic.
template <typename IT>
struct Heap {
  double* v;  // values by heap position
  IT* kbi;    // key_by_index
  IT* ibk;    // index_by_key
  int size;
  __device__ __forceinline__ void place(int index, double val, IT key) {
    v[index] = val;
    kbi[index] = key;
    ibk[key] = (IT)index;
  }
  __device__ void sift_up(int index, double val, IT key) {
    while (index > 0) {
      const int parent = (index - 1) >> 1;
      const double pv = v[parent];
      const IT pk = kbi[parent];
      if (!(pv > val)) break;
      place(index, pv, pk);
      index = parent;
    }
    place(index, val, key);
  }
  __device__ void sift_down(int index, double val, IT key) {
    int child = 2 * index + 1;
    while (child < size) {
      double cv = v[child];
      if (child + 1 < size) {
        const double cv1 = v[child + 1];
        if (cv1 < cv) {
          child += 1;
          cv = cv1;
        }
      }
      if (!(val > cv)) break;
      place(index, cv, kbi[child]);
      index = child;
      child = 2 * index + 1;
    }
    place(index, val, key);
  }
  __device__ void build() {  // Heap.__init__: sift_down from the last parent to the root
    for (int i = size / 2 - 1; i >= 0; --i) sift_down(i, v[i], kbi[i]);
  }
  __device__ void change_value(int key, double value) {
    const int index = ibk[key];
    const double old = v[index];
    if (value < old) sift_up(index, value, (IT)key);
    else sift_down(index, value, (IT)key);
  }
  __device__ void remove_min() {
    const int last = size - 1;
    const double lv = v[last];
    const IT lk = kbi[last];
    place(last, v[0], kbi[0]);  // swap(0, size - 1): the removed root parks behind the heap
    size -= 1;
    if (size > 0) sift_down(0, lv, lk);
  }
};

// first minimum over the 64 lanes of a wave, valid in every lane
__device__ __forceinline__ MinPair wave_min_pair(MinPair best) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MinPair other;
    other.d = __shfl_xor(best.d, o, 64);
    other.i = __shfl_xor(best.i, o, 64);
    best = min_pair(best, other);
  }
  return best;
}

// first minimum of `count` MinPairs in memory (one lane)
__device__ __forceinline__ MinPair lk_min_of(const MinPair* a, int count) {
  MinPair r{a[0].d, a[0].i};
  for (int q = 1; q < count; ++q) r = min_pair(r, MinPair{a[q].d, a[q].i});
  return r;
}

// find_min_dist(n, D, size, x): nearest active neighbour of x among indices > x.  All threads call;
// result valid in every thread.  `red` = LK_W MinPairs of LDS.
__device__ MinPair block_find_min(const double* __restrict__ D, const int* __restrict__ size, int n,
                                  int x, MinPair* red) {
  MinPair best{__builtin_inf(), -1};
  const long base = (long)n * x - ((long)x * (x + 1) / 2) - x - 1;  // cidx(n, x, i) = base + i
  for (int i0 = x + 1 + threadIdx.x; i0 < n; i0 += 4 * LK_T) {
    // 4 row elements per thread in flight (ascending i, so the strict `<` keeps the first minimum)
    double d[4];
    bool act[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * LK_T;
      act[u] = i < n && size[i] != 0;
      d[u] = act[u] ? D[base + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (act[u] && d[u] < best.d) {
        best.d = d[u];
        best.i = i0 + u * LK_T;
      }
  }
  best = wave_min_pair(best);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = best;
  __syncthreads();
  MinPair r = lk_min_of(red, LK_W);
  if (r.i < 0) r.d = __builtin_inf();
  return r;
}

// Initial nearest neighbour of row x among the indices > x, scanned by one wave; valid in every lane, i = -1 for
// the last row.
__device__ __forceinline__ MinPair wave_row_min(const double* __restrict__ D, int n, int x) {
  MinPair best{__builtin_inf(), -1};
  const long base = (long)n * x - ((long)x * (x + 1) / 2) - x - 1;
  for (int i = x + 1 + (threadIdx.x & 63); i < n; i += 64) {
    const double d = D[base + i];
    if (d < best.d) {
      best.d = d;
      best.i = i;
    }
  }
  return wave_min_pair(best);
}

// SciPy's centroid update of the distance between cluster i and the merger of x (nx points) and y (ny points).
// THE OPERATION ORDER IS THE CONTRACT: this is SciPy's expression, evaluated left to right in double, every
// operation rounded on its own (-ffp-contract=off) -- any regrouping changes heights in the last bit and, through
// ties, the merge order.
__device__ __forceinline__ double lk_centroid_dist(double d_xi, double d_yi, double dist, int nx, int ny) {
  return sqrt((((nx * d_xi * d_xi) + (ny * d_yi * d_yi)) - ((nx * ny) * dist * dist) / (nx + ny)) / (nx + ny));
}

constexpr int LK_PU = 8;    // clusters per thread and trip of the z pass
constexpr int LK_PEND = 256;  // lower-bound drops buffered per merge (more -> re-read from D)

// =============================================================================================
// One merge.  The O(N) part -- the Lance-Williams update of column y, the neighbour fix-ups, the lower-bound
// candidates and the nearest-neighbour scan of row y -- is independent per cluster z except for SciPy's heap,
// which lane 0 alone keeps and updates in SciPy's order, so the dendrogram stays bit-identical:
//     find the closest pair (lower-bound repairs by the whole workgroup), lane 0 records the merge and
//     leaves (nx, ny) in the mailbox
//     -- __syncthreads --   the z pass; refreshed rows appended to the pending list, per-wave nearest
//                           neighbour of y
//     -- __syncthreads --   rank-sort the pending rows, heap updates by lane 0, neighbour of y
// Mailbox, pending list and the per-wave minima of row y live in LDS.
// =============================================================================================
struct LkMail {  // one merge, from lane 0 to the z pass and back
  int x, y, nx, ny;
  double dist;
  int npend;  // rows the z pass appended to the pending list
  int ok;     // (find loop) the heap's minimum is a true distance
};

template <typename IT, bool LDS_HEAP>
__global__ __launch_bounds__(LK_T) void k_linkage_centroid(double* __restrict__ D, int n,
                                                            double* __restrict__ Z,
                                                            int* __restrict__ size,
                                                            int* __restrict__ cluster_id,
                                                            double* __restrict__ g_hv,
                                                            int* __restrict__ g_kbi,
                                                            int* __restrict__ g_ibk,
                                                            int* __restrict__ g_nb,
                                                            long long* __restrict__ stats,
                                                            const int* __restrict__ gate) {
  // `gate`: status word of the fast path (linkage_fast.hip) that ran in front of this launch on the same stream;
  // 0 = the dendrogram is already complete
  if (gate != nullptr && *gate == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ MinPair red[LK_W];  // per-wave minima: block_find_min, nearest neighbour of row y
  __shared__ LkMail mail;        // lane 0's broadcast of the find loop and of the recorded merge
  __shared__ int pend_z[LK_PEND], sort_z[LK_PEND];
  __shared__ double pend_d[LK_PEND], sort_d[LK_PEND];
  const int tid = threadIdx.x;
  const int hn = n - 1;  // heap capacity = rows that own a nearest-neighbour candidate

  // per-row state: heap (values = SciPy's min_dist, kept in sync with it), neighbour candidates, bitmap of rows
  // whose lower bound dropped in this merge (always in LDS)
  constexpr IT NONE = (IT) ~(IT)0;  // "no neighbour" (-1)
  Heap<IT> heap;
  IT* nb;
  unsigned int* cand;
  if (LDS_HEAP) {
    heap.v = reinterpret_cast<double*>(lds_raw);
    heap.kbi = reinterpret_cast<IT*>(heap.v + hn);
    heap.ibk = heap.kbi + hn;
    nb = heap.ibk + hn;
    cand = reinterpret_cast<unsigned int*>(lds_raw + (((size_t)hn * (8 + 3 * sizeof(IT)) + 15) & ~(size_t)15));
  } else {
    heap.v = g_hv;
    heap.kbi = reinterpret_cast<IT*>(g_kbi);
    heap.ibk = reinterpret_cast<IT*>(g_ibk);
    nb = reinterpret_cast<IT*>(g_nb);
    cand = reinterpret_cast<unsigned int*>(lds_raw);
  }
  heap.size = hn;
  const int cand_words = (n + 31) / 32;

  // ---- initialisation: sizes, ids, candidate bitmap, nearest neighbours
  for (int i = tid; i < n; i += LK_T) {
    size[i] = 1;
    cluster_id[i] = i;
  }
  for (int i = tid; i < cand_words; i += LK_T) cand[i] = 0u;
  for (int x = tid >> 6; x < n - 1; x += LK_W) {  // (one wave per row)
    const MinPair best = wave_row_min(D, n, x);
    if ((tid & 63) == 0) {
      const double bound = best.i < 0 ? __builtin_inf() : best.d;
      nb[x] = best.i < 0 ? NONE : (IT)best.i;
      heap.v[x] = bound;  // heap position x holds key x for now
      heap.kbi[x] = (IT)x;
      heap.ibk[x] = (IT)x;
    }
  }
  __syncthreads();
  if (tid == 0) heap.build();
  __syncthreads();

  // development counters (lane 0): [0] lower-bound repairs, [1] heap updates of the refresh,
  // [2] refreshes that overflowed the pending buffer, [3..6] cycles in find / record / pass / replay
  long long st_retry = 0, st_cand = 0, st_ovf = 0, st_c0 = 0, st_c1 = 0, st_c2 = 0, st_c3 = 0;
  long long tc;
  auto lap = [&](long long& acc) {
    const long long t2 = __builtin_readcyclecounter();
    acc += t2 - tc;
    tc = t2;
  };
  for (int k = 0; k < n - 1; ++k) {
    tc = __builtin_readcyclecounter();
    int x = 0, y = 0;
    double dist = 0.0;
    // ---- find the two closest clusters: at most n - k lower-bound repairs
    for (int it = 0; it < n - k; ++it) {
      if (tid == 0) {
        const int hx = heap.kbi[0];
        const double hd = heap.v[0];
        const IT hyr = nb[hx];
        const int hy = hyr == NONE ? -1 : (int)hyr;
        mail.x = hx;
        mail.y = hy;
        mail.dist = hd;
        mail.ok = (hy >= 0 && hd == D[cidx(n, hx, hy)]) ? 1 : 0;
      }
      __syncthreads();
      x = mail.x;
      y = mail.y;
      dist = mail.dist;
      const int ok = mail.ok;
      if (ok) break;
      const MinPair p = block_find_min(D, size, n, x, red);  // (barriers inside)
      y = p.i;
      dist = p.d;
      if (tid == 0) {
        nb[x] = y < 0 ? NONE : (IT)y;
        heap.change_value(x, dist);
        ++st_retry;
      }
      __syncthreads();
    }
    lap(st_c0);
    // ---- record the merge and hand it to the z pass (x, y, dist: every thread holds them since the find loop)
    if (tid == 0) {
      heap.remove_min();
      int id_x = cluster_id[x], id_y = cluster_id[y];
      const int nx = size[x], ny = size[y];
      if (id_x > id_y) {
        const int t = id_x;
        id_x = id_y;
        id_y = t;
      }
      Z[4 * (long)k + 0] = (double)id_x;
      Z[4 * (long)k + 1] = (double)id_y;
      Z[4 * (long)k + 2] = dist;
      Z[4 * (long)k + 3] = (double)(nx + ny);
      size[x] = 0;
      size[y] = nx + ny;
      cluster_id[y] = n + k;
      mail.nx = nx;
      mail.ny = ny;
      mail.npend = 0;
    }
    __syncthreads();
    lap(st_c1);
    const int nx = mail.nx, ny = mail.ny;
    // ---- ONE pass over all clusters z (SciPy's four loops are independent per z except for the heap,
    // which is replayed afterwards): Lance-Williams (centroid) update of D[z,y]; neighbour
    // reassignment x -> y for z < x; lower-bound refresh for z < y; nearest neighbour of y among z > y.
    // LK_PU clusters per thread with all distance loads issued before the first use (one audio-hour = 7 176
    // clusters = ONE trip: the pass is a latency chain, a second trip doubles it).
    MinPair best{__builtin_inf(), -1};
    for (int z0 = tid; z0 < n; z0 += LK_PU * LK_T) {
      bool act[LK_PU];
      long izy[LK_PU];
      double d_xi[LK_PU], d_yi[LK_PU];
#pragma unroll
      for (int u = 0; u < LK_PU; ++u) {
        const int z = z0 + u * LK_T;
        act[u] = z < n && z != y && size[z] != 0;
        izy[u] = act[u] ? cidx(n, z, y) : 0;
        d_xi[u] = act[u] ? D[cidx(n, z, x)] : 0.0;
        d_yi[u] = act[u] ? D[izy[u]] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LK_PU; ++u) {
        if (!act[u]) continue;
        const int z = z0 + u * LK_T;
        const double nd = lk_centroid_dist(d_xi[u], d_yi[u], dist, nx, ny);
        D[izy[u]] = nd;
        if (z < y) {
          if (z < x && nb[z] == (IT)x) nb[z] = (IT)y;
          const double bound = heap.v[heap.ibk[z]];  // SciPy's min_dist[z]: the heap value of key z
          if (nd < bound) {
            nb[z] = (IT)y;
            atomicOr(&cand[z >> 5], 1u << (z & 31));
            const int slot = atomicAdd(&mail.npend, 1);
            if (slot < LK_PEND) {
              pend_z[slot] = z;
              pend_d[slot] = nd;
            }
          }
        } else if (nd < best.d) {  // z > y, ascending per thread: first minimum
          best.d = nd;
          best.i = z;
        }
      }
    }
    best = wave_min_pair(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    lap(st_c2);
    // ---- replay the heap updates in SciPy's order: ascending z < y, then row y.  The (few) refreshed
    // rows are rank-sorted by z in parallel; lane 0 then only sifts.
    const int np = mail.npend;  // (reset by lane 0 when it records the next merge)
    if (np <= LK_PEND && tid < np) {
      const int z = pend_z[tid];
      int rank = 0;
      for (int q = 0; q < np; ++q) rank += pend_z[q] < z ? 1 : 0;
      sort_z[rank] = z;
      sort_d[rank] = pend_d[tid];
      cand[z >> 5] = 0u;  // (racing writers all store 0)
    }
    __syncthreads();
    if (tid == 0) {
      st_cand += np;
      if (np <= LK_PEND) {
        for (int q = 0; q < np; ++q) heap.change_value(sort_z[q], sort_d[q]);
      } else {
        ++st_ovf;
        const int words = (y + 31) / 32;
        for (int wi = 0; wi < words; ++wi) {
          unsigned int m = cand[wi];
          if (!m) continue;
          cand[wi] = 0u;
          while (m) {
            const int bit = __builtin_ctz(m);
            m &= m - 1;
            const int z = wi * 32 + bit;
            heap.change_value(z, D[cidx(n, z, y)]);
          }
        }
      }
      if (y < n - 1) {
        const MinPair r = lk_min_of(red, LK_W);
        if (r.i != -1) {
          nb[y] = (IT)r.i;
          heap.change_value(y, r.d);
        }
      }
    }
    __syncthreads();
    st_c3 += __builtin_readcyclecounter() - tc;
  }
  if (tid == 0 && stats != nullptr) {
    stats[0] = st_retry;
    stats[1] = st_cand;
    stats[2] = st_ovf;
    stats[3] = st_c0;
    stats[4] = st_c1;
    stats[5] = st_c2;
    stats[6] = st_c3;
    stats[7] = n;
  }
}

constexpr size_t LK_LDS_MAX = 160 * 1024 - 7680;  // dynamic LDS budget (static part: ~6.5 KB)

// The workspace of pa_linkage_centroid_f64 in 256-byte-aligned blocks: the heap kernel's state (the three heap arrays
// are used only when the heap does not fit into LDS), the fast path's when it is wanted (linkage_fast.hip), then 16
// int64 development counters, 8 + 8: the LAST 128 bytes, where distance.linkage_centroid reads them.
struct LkState {
  int *size, *cid, *nb, *kbi, *ibk;
  double* hv;
  bool fast;
  LfState lf;
  long long* stats;
};
static LkState lk_layout(Carver& c, int n) {
  LkState s;
  s.size = c.take<int>(n);
  s.cid = c.take<int>(n);
  s.nb = c.take<int>(n);
  s.kbi = c.take<int>(n);
  s.ibk = c.take<int>(n);
  s.hv = c.take<double>(n);
  s.fast = lf_wanted(n);
  if (s.fast) lf_layout(c, n, s.lf);
  s.stats = c.take<long long>(16, 128);
  return s;
}
// dynamic LDS of the candidate bitmap (one bit per row)
inline size_t lk_cand_bytes(int n) { return 4 * (size_t)((n + 31) / 32) + 16; }

}  // namespace pa

extern "C" {

size_t pa_linkage_workspace_bytes(int n) {
  if (n < 2) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::lk_layout(c, n); });
}

// D: condensed distance matrix (n*(n-1)/2 doubles), OVERWRITTEN.  Z: (n-1, 4) doubles, SciPy layout.
int pa_linkage_centroid_f64(double* D, int n, double* Z, void* workspace, size_t workspace_bytes,
                            void* stream) {
  if (n < 2) return 0;
  pa::Carver carver(workspace);
  const pa::LkState s = pa::lk_layout(carver, n);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_linkage_centroid_f64: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  // the merge loop is O(N^2) memory traffic in total; algorithmic bytes ~ 3 rows of 8*N per merge
  pa::ProfScope prof("k_linkage_centroid", stream, 9.0 * n * (double)n, 24.0 * n * (double)n);
  if (pa::fill_async(s.stats, 0, 128, st) != hipSuccess) return 1;
  // ---- the heap-free merge first (linkage_fast.hip); its status word gates the exact heap replay below
  int* gate = nullptr;
  if (s.fast) {
    if (const int rc = pa::lf_launch(D, n, Z, s.lf, s.stats + 8, st)) return rc;
    gate = s.lf.status;
    PA_CHECK_LAUNCH("pa_linkage_centroid_f64 (fast path)");
  }
  auto launch = [&](auto kernel, size_t lds) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(pa::LK_T), lds, st, D, n, Z, s.size, s.cid, s.hv, s.kbi, s.ibk, s.nb,
                       s.stats, gate);
  };
  // 16-bit keys: heap values, kbi, ibk and neighbours (14 bytes per row) + the candidate bitmap in LDS
  const size_t cand_bytes = pa::lk_cand_bytes(n);
  const size_t lds16 = (((size_t)(n - 1) * 14 + 15) & ~(size_t)15) + cand_bytes;
  const bool in_lds = n <= 65535 && lds16 <= pa::LK_LDS_MAX;   // the heap in dynamic LDS beyond the default limit
  if (in_lds) PA_ALLOW_LDS("pa_linkage_centroid_f64", (pa::k_linkage_centroid<unsigned short, true>), pa::LK_LDS_MAX);
  if (in_lds) launch(pa::k_linkage_centroid<unsigned short, true>, lds16);
  else launch(pa::k_linkage_centroid<int, false>, cand_bytes);
  PA_CHECK_LAUNCH("pa_linkage_centroid_f64");
  return 0;
}

}  // extern "C"
