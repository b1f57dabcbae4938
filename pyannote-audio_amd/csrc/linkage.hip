// Centroid-linkage dendrogram on gfx950, bit-identical to scipy.cluster.hierarchy.linkage(y, "centroid")
// (SciPy 1.15.3 `_hierarchy.fast_linkage` = Muellner's "generic clustering algorithm" with a
//  nearest-neighbour candidate per row and a binary min-heap of lower bounds), which is what
//  AgglomerativeClustering.cluster calls (reference: pipelines/clustering.py:374-382).
//
// Why a kernel: the merge loop is inherently serial (N-1 dependent merges) but every merge does O(N)
// independent work -- Lance-Williams update of one row/column of the distance matrix, two
// nearest-neighbour row scans, the lower-bound refresh -- which SciPy walks on one host core
// (0.8 s for N = 7 000, the Amdahl term of the whole pipeline).  Here persistent 1024-thread
// workgroups keep the condensed matrix in HBM/L2 (it is produced there by k_pdist_f64 and never
// crosses PCIe), run the O(N) parts data-parallel and leave only the heap sifts (O(log N)) to lane 0.
//
// ONE kernel, k_linkage_centroid<IT, LDS_HEAP, MULTI>, with ONE merge loop and two forms:
//   * MULTI = false (the default): a single workgroup, heap + neighbour candidates in LDS (global memory
//     above ~11 600 points), plain loads and stores, __syncthreads only;
//   * MULTI = true (opt-in, PA_LINKAGE_WGS): G workgroups of one XCD split the O(N) pass of a merge and
//     meet at two grid barriers per merge; workgroup 0 alone keeps the heap.  See "Multi-workgroup form".
// The forms differ in how shared data is accessed (lk_ld / lk_st), where the neighbour candidates live,
// where the lower bound of a row is read (heap / `mind` mirror), the phase boundary (lk_phase) and where
// the per-merge mailbox, pending list and row-y minima live (LDS / LkShared) -- and nowhere else.
//
// Exactness contract (tests/test_pipeline_gpu.py::test_linkage_*): same merge order, same float64
// heights, same tie behaviour as SciPy, because
//   * the distance update is SciPy's expression evaluated left to right in double with separately
//     rounded operations (lk_centroid_dist; this file is compiled with -ffp-contract=off);
//   * row scans return the FIRST index attaining the minimum (SciPy scans with a strict `<`);
//   * all heap operations (build, change_value, remove_min, sift_up/down) are executed by one lane in
//     exactly SciPy's order, including the ascending-z order of the lower-bound refresh.
// hipcc-flags: -ffp-contract=off
#include <stdlib.h>

#include <type_traits>

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

struct MinPair {
  double d;
  int i;
};
// lexicographic "first minimum": smaller value wins, equal values -> smaller index; NaN never wins
__device__ __forceinline__ MinPair min_pair(MinPair a, MinPair b) {
  if (b.i >= 0 && (a.i < 0 || b.d < a.d || (b.d == a.d && b.i < a.i))) return b;
  return a;
}
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

// Accesses to data that ANOTHER workgroup of the multi-workgroup form writes or reads (COH): relaxed agent-scope
// atomics = `global_load / global_store ... sc1`: loads are served by L2 (never by this CU's L1, which no other
// CU's store refreshes), stores go through to memory.  With sc1 on BOTH sides no fence is needed and the protocol
// does not depend on where the workgroups run (MI355X_MICROARCH.md, "inter-workgroup visibility"); a
// __threadfence() per barrier instead costs 3.5-10 us (L2 write-back + L1 invalidate) -- measured here: the
// fenced version of this kernel was SLOWER than one workgroup at every size.  The single-workgroup form (COH =
// false) uses plain loads and stores.
template <bool COH, typename T>
__device__ __forceinline__ T lk_ld(const T* p) {
  if (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}
template <bool COH, typename T>
__device__ __forceinline__ void lk_st(T* p, T v) {
  if (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
// first minimum of `count` MinPairs in memory (one lane)
template <bool COH>
__device__ __forceinline__ MinPair lk_min_of(const MinPair* a, int count) {
  MinPair r{lk_ld<COH>(&a[0].d), lk_ld<COH>(&a[0].i)};
  for (int q = 1; q < count; ++q) r = min_pair(r, MinPair{lk_ld<COH>(&a[q].d), lk_ld<COH>(&a[q].i)});
  return r;
}

// find_min_dist(n, D, size, x): nearest active neighbour of x among indices > x.  All threads call;
// result valid in every thread.  `red` = LK_W MinPairs of LDS.
template <bool COH>
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
      act[u] = i < n && lk_ld<COH>(size + i) != 0;
      d[u] = act[u] ? lk_ld<COH>(D + base + i) : 0.0;
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
  MinPair r = lk_min_of<false>(red, LK_W);
  if (r.i < 0) r.d = __builtin_inf();
  return r;
}

// Initial nearest neighbour of row x among the indices > x, scanned by one wave; valid in every lane, i = -1 for
// the last row.  (D was written by k_pdist_f64, a previous kernel: plain loads in both forms.)
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

constexpr int LK_PU = 8;    // clusters per thread and trip of the single-workgroup z pass
constexpr int LK_PEND = 256;  // lower-bound drops buffered per merge (more -> re-read from D)

// =============================================================================================
// Multi-workgroup form.  The O(N) part of a merge -- the Lance-Williams update of column y, the neighbour
// fix-ups, the lower-bound candidates and the nearest-neighbour scan of row y -- reads ~2 N scattered
// distances; one CU sustains only ~60-100 GB/s of such traffic, which is what made the single workgroup take
// 240 us per merge at N = 57 k (13.9 s for the joint clustering of 8 audio-hours).  Here G workgroups, all on
// ONE XCD (workgroup w runs on XCD w mod 8: the launch has 8 G workgroups and only every 8th works, so the
// matrix stays coherent in one L2), split that pass; workgroup 0 alone keeps SciPy's heap and replays its
// updates in SciPy's order, so the dendrogram stays bit-identical.  Two grid barriers per merge (fence +
// atomic counter + generation word, ~2 us each inside an XCD):
//     WG0: find the closest pair (lower-bound repairs on its own), record the merge, publish (x, y, sizes)
//     -- barrier --   all: one slice of the z pass; refreshed rows appended to a global pending list,
//                     per-workgroup nearest neighbour of y
//     -- barrier --   WG0: rank-sort the pending rows, heap updates by lane 0, neighbour of y
// Everything two workgroups share is read and written with sc1 accesses (lk_ld / lk_st): no fences.
// `mind[z]` mirrors the heap value of key z (SciPy's min_dist[z]) in global memory for the other workgroups.
// The single-workgroup form is the same schedule with G = 1, __syncthreads for the barriers and LDS for LkShared.
// =============================================================================================
struct LkMail {  // one merge, from lane 0 of workgroup 0 to the z pass and back
  int x, y, nx, ny;
  double dist;
  int npend;  // rows the z pass appended to the pending list
  int ok;     // (find loop, LDS copy only) the heap's minimum is a true distance
};
struct LkShared {          // global memory, zero-initialised by the launcher
  int bar_count, bar_gen;
  LkMail mail;
  MinPair red[32];
  int pend_z[LK_PEND];
  double pend_d[LK_PEND];
};

// Grid barrier over the G participating workgroups: every thread waits for its own (sc1) stores to be
// acknowledged, lane 0 arrives on an agent-scope counter and polls the generation word.  No fence: all shared
// data is accessed with sc1 loads / stores (see lk_ld / lk_st).
__device__ __forceinline__ void lk_grid_barrier(LkShared* sh, int G) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int gen = __hip_atomic_load(&sh->bar_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_fetch_add(&sh->bar_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) {
      __hip_atomic_store(&sh->bar_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_fetch_add(&sh->bar_gen, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      while (__hip_atomic_load(&sh->bar_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen)
        __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
}
// phase boundary of the merge loop
template <bool MULTI>
__device__ __forceinline__ void lk_phase(LkShared* sh, int G) {
  if constexpr (MULTI) lk_grid_barrier(sh, G);
  else __syncthreads();
}

template <typename IT, bool LDS_HEAP, bool MULTI>
__global__ __launch_bounds__(LK_T) void k_linkage_centroid(double* __restrict__ D, int n,
                                                            double* __restrict__ Z,
                                                            int* __restrict__ size,
                                                            int* __restrict__ cluster_id,
                                                            double* __restrict__ g_hv,
                                                            int* __restrict__ g_kbi,
                                                            int* __restrict__ g_ibk,
                                                            int* __restrict__ g_nb,
                                                            double* __restrict__ mind,
                                                            unsigned int* __restrict__ g_cand,
                                                            LkShared* __restrict__ sh, int g_workgroups,
                                                            long long* __restrict__ stats,
                                                            const int* __restrict__ gate) {
  // `gate`: status word of the fast path (linkage_fast.hip) that ran in front of this launch on the same stream;
  // 0 = the dendrogram is already complete
  if (gate != nullptr && *gate == 0) return;
  if (MULTI && (blockIdx.x & 7) != 0) return;  // only the workgroups of one XCD take part
  const int wg = MULTI ? blockIdx.x >> 3 : 0, G = MULTI ? g_workgroups : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ MinPair red[LK_W];
  __shared__ LkMail lds_mail;  // lane 0's broadcast of the find loop; the single form's mailbox
  __shared__ int lds_pend_z[LK_PEND], sort_z[LK_PEND];
  __shared__ double lds_pend_d[LK_PEND], sort_d[LK_PEND];
  LkMail* const mail = MULTI ? &sh->mail : &lds_mail;
  int* const pend_z = MULTI ? sh->pend_z : lds_pend_z;
  double* const pend_d = MULTI ? sh->pend_d : lds_pend_d;
  const MinPair* const y_min = MULTI ? sh->red : red;  // nearest neighbour of row y per workgroup / per wave
  const int y_mins = MULTI ? G : LK_W;
  const int tid = threadIdx.x;
  const int hn = n - 1;  // heap capacity = rows that own a nearest-neighbour candidate

  // per-row state: heap (values = SciPy's min_dist, kept in sync with it), neighbour candidates (in global
  // memory, as int, when every workgroup writes them), bitmap of rows whose lower bound dropped in this merge
  using NT = std::conditional_t<MULTI, int, IT>;
  constexpr NT NONE = (NT) ~(NT)0;  // "no neighbour" (-1)
  Heap<IT> heap;
  NT* nb;
  unsigned int* cand;
  if (LDS_HEAP) {
    heap.v = reinterpret_cast<double*>(lds_raw);
    heap.kbi = reinterpret_cast<IT*>(heap.v + hn);
    heap.ibk = heap.kbi + hn;
  } else {
    heap.v = g_hv;
    heap.kbi = reinterpret_cast<IT*>(g_kbi);
    heap.ibk = reinterpret_cast<IT*>(g_ibk);
  }
  if constexpr (MULTI) {
    nb = g_nb;
    cand = g_cand;
  } else if (LDS_HEAP) {
    nb = heap.ibk + hn;
    cand = reinterpret_cast<unsigned int*>(lds_raw + (((size_t)hn * (8 + 3 * sizeof(IT)) + 15) & ~(size_t)15));
  } else {
    nb = reinterpret_cast<IT*>(g_nb);
    cand = reinterpret_cast<unsigned int*>(lds_raw);
  }
  heap.size = hn;
  const int cand_words = (n + 31) / 32;
  // lane 0's heap update; the multi form mirrors the new lower bound for the other workgroups
  auto change_value = [&](int key, double value) {
    heap.change_value(key, value);
    if constexpr (MULTI) lk_st<true>(mind + key, value);
  };

  // ---- initialisation, split over the workgroups: sizes, ids, candidate bitmap, nearest neighbours
  for (int i = wg * LK_T + tid; i < n; i += G * LK_T) {
    lk_st<MULTI>(size + i, 1);
    lk_st<MULTI>(cluster_id + i, i);
  }
  for (int i = wg * LK_T + tid; i < cand_words; i += G * LK_T) lk_st<MULTI>(cand + i, 0u);
  for (int x = wg * LK_W + (tid >> 6); x < n - 1; x += G * LK_W) {  // (one wave per row)
    const MinPair best = wave_row_min(D, n, x);
    if ((tid & 63) == 0) {
      const double bound = best.i < 0 ? __builtin_inf() : best.d;
      lk_st<MULTI>(nb + x, best.i < 0 ? NONE : (NT)best.i);
      if constexpr (MULTI) {
        lk_st<true>(mind + x, bound);
      } else {  // heap position x holds key x for now
        heap.v[x] = bound;
        heap.kbi[x] = (IT)x;
        heap.ibk[x] = (IT)x;
      }
    }
  }
  lk_phase<MULTI>(sh, G);
  if (wg == 0) {
    if constexpr (MULTI) {
      for (int x = tid; x < hn; x += LK_T) {
        heap.v[x] = lk_ld<true>(mind + x);
        heap.kbi[x] = (IT)x;
        heap.ibk[x] = (IT)x;
      }
      __syncthreads();
    }
    if (tid == 0) heap.build();
    __syncthreads();
  }

  // development counters (lane 0 of workgroup 0): [0] lower-bound repairs, [1] heap updates of the refresh,
  // [2] refreshes that overflowed the pending buffer, [3..6] cycles in find / record / pass / replay (multi form:
  // find + record / barrier wait / pass / barrier wait + replay)
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
    if (wg == 0) {
      // ---- find the two closest clusters: at most n - k lower-bound repairs
      for (int it = 0; it < n - k; ++it) {
        if (tid == 0) {
          const int hx = heap.kbi[0];
          const double hd = heap.v[0];
          const NT hyr = lk_ld<MULTI>(nb + hx);
          const int hy = hyr == NONE ? -1 : (int)hyr;
          lds_mail.x = hx;
          lds_mail.y = hy;
          lds_mail.dist = hd;
          lds_mail.ok = (hy >= 0 && hd == lk_ld<MULTI>(D + cidx(n, hx, hy))) ? 1 : 0;
        }
        __syncthreads();
        x = lds_mail.x;
        y = lds_mail.y;
        dist = lds_mail.dist;
        const int ok = lds_mail.ok;
        if (ok) break;
        const MinPair p = block_find_min<MULTI>(D, size, n, x, red);  // (barriers inside)
        y = p.i;
        dist = p.d;
        if (tid == 0) {
          lk_st<MULTI>(nb + x, y < 0 ? NONE : (NT)y);
          change_value(x, dist);
          ++st_retry;
        }
        __syncthreads();
      }
      lap(st_c0);
      // ---- record the merge and hand it to the z pass
      if (tid == 0) {
        heap.remove_min();
        int id_x = lk_ld<MULTI>(cluster_id + x), id_y = lk_ld<MULTI>(cluster_id + y);
        const int nx = lk_ld<MULTI>(size + x), ny = lk_ld<MULTI>(size + y);
        if (id_x > id_y) {
          const int t = id_x;
          id_x = id_y;
          id_y = t;
        }
        Z[4 * (long)k + 0] = (double)id_x;
        Z[4 * (long)k + 1] = (double)id_y;
        Z[4 * (long)k + 2] = dist;
        Z[4 * (long)k + 3] = (double)(nx + ny);
        lk_st<MULTI>(size + x, 0);
        lk_st<MULTI>(size + y, nx + ny);
        lk_st<MULTI>(cluster_id + y, n + k);
        if constexpr (MULTI) {  // (single form: every thread holds them since the find loop)
          lk_st<true>(&mail->x, x);
          lk_st<true>(&mail->y, y);
          lk_st<true>(&mail->dist, dist);
        }
        lk_st<MULTI>(&mail->nx, nx);
        lk_st<MULTI>(&mail->ny, ny);
        lk_st<MULTI>(&mail->npend, 0);
      }
      if constexpr (MULTI) lap(st_c0);  // (multi form: [3] takes the record too, [4] is the barrier wait alone)
    }
    lk_phase<MULTI>(sh, G);
    lap(st_c1);
    if constexpr (MULTI) {
      x = lk_ld<true>(&mail->x);
      y = lk_ld<true>(&mail->y);
      dist = lk_ld<true>(&mail->dist);
    }
    const int nx = lk_ld<MULTI>(&mail->nx), ny = lk_ld<MULTI>(&mail->ny);
    // ---- ONE pass over all clusters z (SciPy's four loops are independent per z except for the heap,
    // which is replayed afterwards): Lance-Williams (centroid) update of D[z,y]; neighbour
    // reassignment x -> y for z < x; lower-bound refresh for z < y; nearest neighbour of y among z > y.
    // Single form: all of [0, n), LK_PU clusters per thread with all distance loads issued before the first use
    // (one audio-hour = 7 176 clusters = ONE trip: the pass is a latency chain, a second trip doubles it).
    // Multi form: contiguous slices of ~n / G clusters (at n = 7 k and 8 workgroups every thread owns ONE cluster --
    // the pass is bound by the f64 division / square root throughput of a CU, so it has to be spread evenly).
    constexpr int PU = MULTI ? 4 : LK_PU;
    int z_begin = 0, z_end = n;
    if constexpr (MULTI) {
      const int slice = (((n + G - 1) / G) + 63) & ~63;
      z_begin = wg * slice;
      z_end = min(n, z_begin + slice);
    }
    MinPair best{__builtin_inf(), -1};
    for (int z0 = z_begin + tid; z0 < z_end; z0 += PU * LK_T) {
      bool act[PU];
      long izy[PU];
      double d_xi[PU], d_yi[PU];
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const int z = z0 + u * LK_T;
        act[u] = z < z_end && z != y && lk_ld<MULTI>(size + z) != 0;
        izy[u] = act[u] ? cidx(n, z, y) : 0;
        d_xi[u] = act[u] ? lk_ld<MULTI>(D + cidx(n, z, x)) : 0.0;
        d_yi[u] = act[u] ? lk_ld<MULTI>(D + izy[u]) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        if (!act[u]) continue;
        const int z = z0 + u * LK_T;
        const double nd = lk_centroid_dist(d_xi[u], d_yi[u], dist, nx, ny);
        lk_st<MULTI>(D + izy[u], nd);
        if (z < y) {
          if (z < x && lk_ld<MULTI>(nb + z) == (NT)x) lk_st<MULTI>(nb + z, (NT)y);
          // SciPy's min_dist[z]: the heap value of key z / its mirror
          const double bound = MULTI ? lk_ld<true>(mind + z) : heap.v[heap.ibk[z]];
          if (nd < bound) {
            lk_st<MULTI>(nb + z, (NT)y);
            atomicOr(&cand[z >> 5], 1u << (z & 31));
            const int slot = atomicAdd(&mail->npend, 1);
            if (slot < LK_PEND) {
              lk_st<MULTI>(pend_z + slot, z);
              lk_st<MULTI>(pend_d + slot, nd);
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
    if constexpr (MULTI) {
      if (tid == 0) {
        const MinPair r = lk_min_of<false>(red, LK_W);
        lk_st<true>(&sh->red[wg].d, r.d);
        lk_st<true>(&sh->red[wg].i, r.i);
      }
    }
    lap(st_c2);
    if constexpr (MULTI) lk_grid_barrier(sh, G);
    if (wg == 0) {
      // ---- replay the heap updates in SciPy's order: ascending z < y, then row y.  The (few) refreshed
      // rows are rank-sorted by z in parallel; lane 0 then only sifts.
      const int np = lk_ld<MULTI>(&mail->npend);  // (reset by lane 0 when it records the next merge)
      if (np <= LK_PEND && tid < np) {
        const int z = lk_ld<MULTI>(pend_z + tid);
        int rank = 0;
        for (int q = 0; q < np; ++q) rank += lk_ld<MULTI>(pend_z + q) < z ? 1 : 0;
        sort_z[rank] = z;
        sort_d[rank] = lk_ld<MULTI>(pend_d + tid);
        lk_st<MULTI>(cand + (z >> 5), 0u);  // (racing writers all store 0)
      }
      __syncthreads();
      if (tid == 0) {
        st_cand += np;
        if (np <= LK_PEND) {
          for (int q = 0; q < np; ++q) change_value(sort_z[q], sort_d[q]);
        } else {
          ++st_ovf;
          const int words = (y + 31) / 32;
          for (int wi = 0; wi < words; ++wi) {
            unsigned int m = lk_ld<MULTI>(cand + wi);
            if (!m) continue;
            lk_st<MULTI>(cand + wi, 0u);
            while (m) {
              const int bit = __builtin_ctz(m);
              m &= m - 1;
              const int z = wi * 32 + bit;
              change_value(z, lk_ld<MULTI>(D + cidx(n, z, y)));
            }
          }
        }
        if (y < n - 1) {
          const MinPair r = lk_min_of<MULTI>(y_min, y_mins);
          if (r.i != -1) {
            lk_st<MULTI>(nb + y, (NT)r.i);
            change_value(y, r.d);
          }
        }
      }
      __syncthreads();
    }
    st_c3 += __builtin_readcyclecounter() - tc;
  }
  if (wg == 0 && tid == 0 && stats != nullptr) {
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

inline size_t lk_align(size_t v) { return (v + 255) & ~(size_t)255; }

// linkage_fast.hip: the heap-free merge that runs first; the kernel of this file is its gated fallback
bool lf_wanted(int n);
size_t lf_workspace_bytes(int n);
int lf_launch(const double* cond, int n, double* Z, void* workspace, long long* stats, int** gate_out,
              hipStream_t st);

// Byte offsets of the heap kernel's state in the workspace: size (at 0), cluster_id, neighbour, kbi, ibk (int) +
// heap values, min_dist mirror (double) + candidate bitmap + the multi-workgroup mailbox
struct LkLayout {
  size_t cid, nb, kbi, ibk, hv, mind, cand, shared, end;
  size_t cand_bytes;
};
inline LkLayout lk_layout(int n) {
  const size_t ni = lk_align(sizeof(int) * (size_t)n), nd = lk_align(sizeof(double) * (size_t)n);
  LkLayout l;
  l.cand_bytes = 4 * (size_t)((n + 31) / 32) + 16;
  l.cid = ni;
  l.nb = l.cid + ni;
  l.kbi = l.nb + ni;
  l.ibk = l.kbi + ni;
  l.hv = l.ibk + ni;
  l.mind = l.hv + nd;
  l.cand = l.mind + nd;
  l.shared = l.cand + lk_align(l.cand_bytes);
  l.end = l.shared + lk_align(sizeof(LkShared));
  return l;
}

}  // namespace pa

extern "C" {

// layout: [heap kernel state][fast path: square matrix + row state][16 int64 counters: 8 heap kernel, 8 fast path]
size_t pa_linkage_workspace_bytes(int n) {
  if (n < 2) return 0;
  return pa::lk_layout(n).end + pa::lf_workspace_bytes(n) + 128;
}

// number of workgroups of the heap kernel.  ONE unless PA_LINKAGE_WGS asks for more: the multi-workgroup form
// synchronises with a hand-rolled spin barrier between workgroups that are launched non-cooperatively and each pin a
// whole CU's LDS; it is only safe when the caller owns the GPU (nothing else resident on XCD 0), which a library
// cannot know.  Since round 4 the heap kernel is the FALLBACK (exact ties) behind linkage_fast.hip, so the
// default never needs it; the opt-in stays for experiments (tools/time_linkage.py).
static int lk_num_workgroups() {
  const char* e = getenv("PA_LINKAGE_WGS");
  if (e != nullptr && atoi(e) >= 1) return atoi(e) > 32 ? 32 : atoi(e);
  return 1;
}

// D: condensed distance matrix (n*(n-1)/2 doubles), OVERWRITTEN.  Z: (n-1, 4) doubles, SciPy layout.
int pa_linkage_centroid_f64_ex(double* D, int n, double* Z, void* workspace, size_t workspace_bytes, int alone,
                               void* stream);

int pa_linkage_centroid_f64(double* D, int n, double* Z, void* workspace, size_t workspace_bytes,
                            void* stream) {
  return pa_linkage_centroid_f64_ex(D, n, Z, workspace, workspace_bytes, 0, stream);
}

int pa_linkage_centroid_f64_ex(double* D, int n, double* Z, void* workspace, size_t workspace_bytes, int alone,
                               void* stream) {
  (void)alone;
  if (n < 2) return 0;
  PA_REQUIRE(workspace_bytes >= pa_linkage_workspace_bytes(n), "pa_linkage_centroid_f64: workspace too small");
  const pa::LkLayout l = pa::lk_layout(n);
  unsigned char* w = (unsigned char*)workspace;
  int* size = (int*)w;
  int* cid = (int*)(w + l.cid);
  int* nb = (int*)(w + l.nb);
  int* kbi = (int*)(w + l.kbi);
  int* ibk = (int*)(w + l.ibk);
  double* hv = (double*)(w + l.hv);
  double* mind = (double*)(w + l.mind);
  unsigned int* cand = (unsigned int*)(w + l.cand);
  pa::LkShared* shared = (pa::LkShared*)(w + l.shared);
  long long* stats = (long long*)(w + pa_linkage_workspace_bytes(n) - 128);
  hipStream_t st = (hipStream_t)stream;
  // the merge loop is O(N^2) memory traffic in total; algorithmic bytes ~ 3 rows of 8*N per merge
  pa::ProfScope prof("k_linkage_centroid", stream, 9.0 * n * (double)n, 24.0 * n * (double)n);
  if (hipMemsetAsync(stats, 0, 128, st) != hipSuccess) return 1;
  // ---- the heap-free merge first (linkage_fast.hip); its status word gates the exact heap replay below
  int* gate = nullptr;
  if (pa::lf_wanted(n)) {
    if (pa::lf_launch(D, n, Z, w + l.end, stats + 8, &gate, st) != 0) return 1;
    PA_CHECK_LAUNCH("pa_linkage_centroid_f64 (fast path)");
  }
  const int G = lk_num_workgroups();
  // `big_lds`: the instantiation keeps its heap in dynamic LDS beyond the default limit (the attribute is set on
  // every call: it belongs to the current device, not to the process)
  auto launch = [&](auto kernel, int grid, size_t lds, bool big_lds) {
    if (big_lds)
      (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)pa::LK_LDS_MAX);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(pa::LK_T), lds, st, D, n, Z, size, cid, hv, kbi, ibk, nb, mind,
                       cand, shared, G, stats, gate);
  };
  if (G > 1) {
    if (hipMemsetAsync(shared, 0, sizeof(pa::LkShared), st) != hipSuccess) return 1;
    const size_t lds_heap = ((size_t)(n - 1) * 12 + 15) & ~(size_t)15;
    if (n <= 65535 && lds_heap <= pa::LK_LDS_MAX)
      launch(pa::k_linkage_centroid<unsigned short, true, true>, 8 * G, lds_heap, true);
    else
      launch(pa::k_linkage_centroid<int, false, true>, 8 * G, 0, false);
  } else {
    const size_t lds16 = (((size_t)(n - 1) * 14 + 15) & ~(size_t)15) + l.cand_bytes;
    if (n <= 65535 && lds16 <= pa::LK_LDS_MAX)
      launch(pa::k_linkage_centroid<unsigned short, true, false>, 1, lds16, true);
    else
      launch(pa::k_linkage_centroid<int, false, false>, 1, l.cand_bytes, false);
  }
  PA_CHECK_LAUNCH("pa_linkage_centroid_f64");
  return 0;
}

}  // extern "C"
