// scipy.spatial.distance.cdist(., ., "cosine") in float64, bit for bit: the device functions shared by the
// clustering distances (cluster.hip) and the verification trials (verification.hip).  A translation unit that
// includes this header is compiled with -ffp-contract=off (see cluster.hip): the products and sums below round
// separately, as SciPy's do.
#pragma once
#include "common.h"

namespace pa {

// SciPy's cdist "cosine" kernels (distance_impl.h: dot_product / _row_norms) are compiled 2-way
// vectorised in the x86-64 wheel (SSE2, two doubles per register): even and odd k accumulate
// separately, the two lanes are added, then an odd tail element is added last.  Pinned against
// scipy 1.15.3 for even and odd D (tools/diag_pdist.py, tests/test_pipeline_gpu.py).
__device__ __forceinline__ double dot2way(const double* __restrict__ u, const double* __restrict__ v,
                                          int D) {
  double s0 = 0.0, s1 = 0.0;
  const int m = D & ~1;
  for (int k = 0; k < m; k += 2) {
    s0 = s0 + u[k] * v[k];
    s1 = s1 + u[k + 1] * v[k + 1];
  }
  double t = s0 + s1;
  if (D & 1) t = t + u[D - 1] * v[D - 1];
  return t;
}

// dot2way of rows kept in other types (float32 embeddings against float64 sums: online.hip): every element is
// converted to double first, which is exact, then the same products and sums in the same order
template <typename TU, typename TV>
__device__ __forceinline__ double dot2way_as_f64(const TU* __restrict__ u, const TV* __restrict__ v, int D) {
  double s0 = 0.0, s1 = 0.0;
  const int m = D & ~1;
  for (int k = 0; k < m; k += 2) {
    s0 = s0 + (double)u[k] * (double)v[k];
    s1 = s1 + (double)u[k + 1] * (double)v[k + 1];
  }
  double t = s0 + s1;
  if (D & 1) t = t + (double)u[D - 1] * (double)v[D - 1];
  return t;
}

// |x| of one row, as _row_norms takes it
__device__ __forceinline__ double row_norm_f64(const double* __restrict__ x, int D) {
  return __dsqrt_rn(dot2way(x, x, D));
}

// 1 - clip(s / (na nb)) for the dot product s of two rows with norms na and nb
__device__ __forceinline__ double cosine_distance_f64(double s, double na, double nb) {
  double c = s / (na * nb);
  if (fabs(c) > 1.0) c = copysign(1.0, c);
  return 1.0 - c;
}

}  // namespace pa
