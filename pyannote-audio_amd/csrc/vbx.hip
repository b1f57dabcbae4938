// VBx clustering (variational Bayes HMM-free x-vector clustering) and the PLDA projection on gfx950, fp64.
// Replaces the numpy loops of utils/vbx.py:27-140 (VBx), core/plda.py:47-60 + utils/vbx.py:205-217 (the
// x-vector -> PLDA transform), called from pipelines/clustering.py:606-617.
//
// Sizes: N = training embeddings of a file (<= ~10^4; 6 x 10^4 for a joint clustering), D = 128 PLDA
// dimensions, S = clusters of the AHC initialisation (tens).  One VB iteration is O(N S D) fp64 FMAs --
// far below any roofline: the kernels are written for a short dependent chain (3 launches per
// iteration, one 8-byte read-back for the convergence test) and for DETERMINISTIC reductions (fixed
// trees, no atomics), so that a run is reproducible bit for bit.  Data layout: gamma [N][S], rho [N][D],
// speaker models alpha / invL [S][D]; all double.
// hipcc-flags: -ffp-contract=off
#include "common.h"

#include <algorithm>

namespace pa {

constexpr int VB_T = 256;

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < VB_T / 64; ++i) s += red[i];
  return s;
}
__device__ __forceinline__ double block_max_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < VB_T / 64; ++i) s = fmax(s, red[i]);
  return s;
}

// x (N, DIN) fp32 -> fea (N, DOUT) fp64:
//   y = sqrt(DMID) * l2( lda^T ( sqrt(DIN) * l2(x - mean1) ) - mean2 );  fea = (y - mu) tr^T [:, :DOUT]
// one workgroup per embedding; lda [DIN][DMID], trT [DMID][DOUT] (column k of trT = row k of tr).
__global__ __launch_bounds__(VB_T) void k_plda_transform(const float* __restrict__ X, int DIN, int DMID,
                                                        int DOUT, const double* __restrict__ mean1,
                                                        const double* __restrict__ lda,
                                                        const double* __restrict__ mean2,
                                                        const double* __restrict__ mu,
                                                        const double* __restrict__ trT,
                                                        double* __restrict__ fea) {
  extern __shared__ double sm[];  // DIN + DMID doubles
  __shared__ double red[VB_T / 64];
  double* xs = sm;
  double* ys = sm + DIN;
  const long n = blockIdx.x;
  double ss = 0.0;
  for (int i = threadIdx.x; i < DIN; i += VB_T) {
    const double v = (double)X[n * DIN + i] - mean1[i];
    xs[i] = v;
    ss += v * v;
  }
  const double sc1 = sqrt((double)DIN) / sqrt(block_sum_d(ss, red));
  double ss2 = 0.0;
  for (int j = threadIdx.x; j < DMID; j += VB_T) {
    double a = 0.0;
    for (int i = 0; i < DIN; ++i) a += lda[(long)i * DMID + j] * (xs[i] * sc1);
    a -= mean2[j];
    ys[j] = a;
    ss2 += a * a;
  }
  const double sc2 = sqrt((double)DMID) / sqrt(block_sum_d(ss2, red));
  __syncthreads();
  for (int k = threadIdx.x; k < DOUT; k += VB_T) {
    double a = 0.0;
    for (int j = 0; j < DMID; ++j) a += (ys[j] * sc2 - mu[j]) * trT[(long)j * DOUT + k];
    fea[n * DOUT + k] = a;
  }
}

// rho = fea * sqrt(Phi) (18);  G[n] = -0.5 (sum_d fea^2 + D log 2 pi)  (constant term of (23))
__global__ __launch_bounds__(VB_T) void k_vbx_prepare(const double* __restrict__ fea, int N, int D,
                                                     const double* __restrict__ Phi,
                                                     double* __restrict__ rho, double* __restrict__ G) {
  __shared__ double red[VB_T / 64];
  const long n = blockIdx.x;
  double ss = 0.0;
  for (int d = threadIdx.x; d < D; d += VB_T) {
    const double v = fea[n * D + d];
    rho[n * D + d] = v * sqrt(Phi[d]);
    ss += v * v;
  }
  ss = block_sum_d(ss, red);
  if (threadIdx.x == 0) G[n] = -0.5 * (ss + D * 1.8378770664093453 /* log(2 pi) */);
}

// M step for speaker s = blockIdx.x: Nk = sum_n gamma[n,s]; invL (17), alpha (16);
// cterm[s] = 0.5 sum_d (invL + alpha^2) Phi;  eterm[s] = sum_d (log invL - invL - alpha^2 + 1)  (25)
// (one body for the per-file kernel and the batched one below: the two must agree bit for bit)
__device__ __forceinline__ void vbx_mstep_body(int s, const double* __restrict__ gamma,
                                               const double* __restrict__ rho, int N, int S, int D,
                                               const double* __restrict__ Phi, double FaFb,
                                               double* __restrict__ alpha, double* __restrict__ invL,
                                               double* __restrict__ Nk, double* __restrict__ cterm,
                                               double* __restrict__ eterm, double* part_sm, double* red) {
  double part = 0.0;
  for (int n = threadIdx.x; n < N; n += VB_T) part += gamma[(long)n * S + s];
  const double nk = block_sum_d(part, red);
  // (gamma^T rho)[s, :]: the N rows are split over the VB_T / 128 thread groups, 4 independent partial
  // sums per thread; partials are combined in a fixed order (deterministic, not numpy's BLAS order)
  // part_sm: [VB_T / 128][D]
  constexpr int DP = 128, NP = VB_T / DP;
  const int p = threadIdx.x / DP, dl = threadIdx.x % DP;
  const int n0 = (int)((long)N * p / NP), n1 = (int)((long)N * (p + 1) / NP);
  for (int d = dl; d < D; d += DP) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int n = n0;
    for (; n + 3 < n1; n += 4) {
      a0 += gamma[(long)n * S + s] * rho[(long)n * D + d];
      a1 += gamma[(long)(n + 1) * S + s] * rho[(long)(n + 1) * D + d];
      a2 += gamma[(long)(n + 2) * S + s] * rho[(long)(n + 2) * D + d];
      a3 += gamma[(long)(n + 3) * S + s] * rho[(long)(n + 3) * D + d];
    }
    for (; n < n1; ++n) a0 += gamma[(long)n * S + s] * rho[(long)n * D + d];
    part_sm[p * D + d] = (a0 + a1) + (a2 + a3);
  }
  __syncthreads();
  double c = 0.0, e = 0.0;
  for (int d = threadIdx.x; d < D; d += VB_T) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) acc += part_sm[q * D + d];
    const double il = 1.0 / (1.0 + FaFb * nk * Phi[d]);
    const double al = FaFb * il * acc;
    invL[(long)s * D + d] = il;
    alpha[(long)s * D + d] = al;
    c += (il + al * al) * Phi[d];
    e += log(il) - il - al * al + 1.0;
  }
  c = block_sum_d(c, red);
  e = block_sum_d(e, red);
  if (threadIdx.x == 0) {
    Nk[s] = nk;
    cterm[s] = 0.5 * c;
    eterm[s] = e;
  }
}

__global__ __launch_bounds__(VB_T) void k_vbx_mstep(const double* __restrict__ gamma,
                                                   const double* __restrict__ rho, int N, int S, int D,
                                                   const double* __restrict__ Phi, double FaFb,
                                                   double* __restrict__ alpha, double* __restrict__ invL,
                                                   double* __restrict__ Nk, double* __restrict__ cterm,
                                                   double* __restrict__ eterm) {
  __shared__ double red[VB_T / 64];
  extern __shared__ double part_sm[];  // [VB_T / 128][D]
  vbx_mstep_body(blockIdx.x, gamma, rho, N, S, D, Phi, FaFb, alpha, invL, Nk, cterm, eterm, part_sm, red);
}

// E step for frame n = blockIdx.x: log_p[s] = Fa (rho_n . alpha_s - cterm[s] + G[n]) (23);
// lpi[s] = log(pi[s] + 1e-8) with pi = Nk / sum Nk (uniform in the first iteration);
// log_p_x = logsumexp_s(log_p + lpi);  gamma[n,s] = exp(log_p + lpi - log_p_x)
__device__ __forceinline__ void vbx_estep_body(long n, const double* __restrict__ rho,
                                               const double* __restrict__ alpha,
                                               const double* __restrict__ cterm,
                                               const double* __restrict__ G,
                                               const double* __restrict__ Nk, int uniform_pi, int S, int D,
                                               double Fa, double* __restrict__ gamma,
                                               double* __restrict__ logpx, double* sm, double* red) {
  double* r = sm;  // D (rho_n) + S (scores)
  double* sc = sm + D;
  for (int d = threadIdx.x; d < D; d += VB_T) r[d] = rho[n * D + d];
  double tot = 0.0;
  for (int s = threadIdx.x; s < S; s += VB_T) tot += Nk[s];
  tot = block_sum_d(tot, red);  // (also the barrier that publishes r[])
  double mx = -__builtin_inf();
  for (int s = threadIdx.x; s < S; s += VB_T) {
    double dot = 0.0;
    for (int d = 0; d < D; ++d) dot += r[d] * alpha[(long)s * D + d];
    const double pi = uniform_pi ? 1.0 / S : Nk[s] / tot;
    const double v = Fa * (dot - cterm[s] + G[n]) + log(pi + 1e-8);
    sc[s] = v;
    mx = fmax(mx, v);
  }
  mx = block_max_d(mx, red);
  double se = 0.0;
  for (int s = threadIdx.x; s < S; s += VB_T) se += exp(sc[s] - mx);
  se = block_sum_d(se, red);
  const double lse = mx + log(se);
  for (int s = threadIdx.x; s < S; s += VB_T) gamma[n * S + s] = exp(sc[s] - lse);
  if (threadIdx.x == 0) logpx[n] = lse;
}

__global__ __launch_bounds__(VB_T) void k_vbx_estep(const double* __restrict__ rho,
                                                   const double* __restrict__ alpha,
                                                   const double* __restrict__ cterm,
                                                   const double* __restrict__ G,
                                                   const double* __restrict__ Nk, int uniform_pi, int N,
                                                   int S, int D, double Fa, double* __restrict__ gamma,
                                                   double* __restrict__ logpx) {
  extern __shared__ double sm[];  // D (rho_n) + S (scores)
  __shared__ double red[VB_T / 64];
  vbx_estep_body(blockIdx.x, rho, alpha, cterm, G, Nk, uniform_pi, S, D, Fa, gamma, logpx, sm, red);
}

// ELBO (25) = sum_n log_p_x[n] + 0.5 Fb sum_s eterm[s]: one workgroup, fixed summation tree
// (every thread returns the value)
__device__ __forceinline__ double vbx_elbo_body(const double* __restrict__ logpx, int N,
                                                const double* __restrict__ eterm, int S, double Fb,
                                                double* red) {
  double a = 0.0, b = 0.0;
  for (int n = threadIdx.x; n < N; n += VB_T) a += logpx[n];
  for (int s = threadIdx.x; s < S; s += VB_T) b += eterm[s];
  a = block_sum_d(a, red);
  b = block_sum_d(b, red);
  return a + Fb * 0.5 * b;
}

__global__ __launch_bounds__(VB_T) void k_vbx_elbo(const double* __restrict__ logpx, int N,
                                                  const double* __restrict__ eterm, int S, double Fb,
                                                  double* __restrict__ out) {
  __shared__ double red[VB_T / 64];
  const double v = vbx_elbo_body(logpx, N, eterm, S, Fb, red);
  if (threadIdx.x == 0) out[0] = v;
}

// ---- a batch of VB inferences over the same features (pa_vbx_run_batch) ----------------------------------
// A job is (initial responsibilities, S_j, Fa_j, Fb_j); rho and G are shared.  Every round is the three steps
// above with the job as blockIdx.y; a job's ELBO workgroup applies the convergence test and raises the job's
// `done` flag, after which all of its workgroups return at entry.  Per-job buffers sit at a common stride
// (sized for the largest S of the call); inside its slab a job uses its own S_j as the row length, so the
// index arithmetic -- and with it every sum -- is the per-file kernels'.
struct VbxJob {
  long gamma0;  // offset of the job's initial responsibilities (N, S) in the gamma0 buffer, in doubles
  int S;        // 0: the job table names responsibilities outside the buffer or more clusters than Smax
  double Fa, Fb;
};

struct VbxBatch {
  const int64_t* job_init;  // [J][2]: offset into gamma0, S
  const double* job_f;      // [J][2]: Fa, Fb
  long gamma0_len;
  double* gamma;    // [J][N * Smax]
  double* logpx;    // [J][N]
  double* alpha;    // [J][Smax * D]
  double* invL;     // [J][Smax * D]
  double* Nk;       // [J][Smax] (also cterm, eterm)
  double* cterm;
  double* eterm;
  double* elbo;     // [J][max_iterations]
  int* iterations;  // [J]
  int* done;        // [J]
  int N, D, Smax, max_iterations;
};

// a job the kernels must not touch (its iteration count stays 0) comes back with S = 0
__device__ __forceinline__ VbxJob vbx_job(const VbxBatch& b, int j) {
  VbxJob job;
  job.gamma0 = b.job_init[2 * j];
  const int64_t S = b.job_init[2 * j + 1];
  const bool ok = S >= 1 && S <= b.Smax && job.gamma0 >= 0 && job.gamma0 + (long)b.N * S <= b.gamma0_len;
  job.S = ok ? (int)S : 0;
  job.Fa = b.job_f[2 * j];
  job.Fb = b.job_f[2 * j + 1];
  return job;
}

__global__ __launch_bounds__(VB_T) void k_vbx_batch_begin(VbxBatch b, const double* __restrict__ gamma0) {
  const int j = blockIdx.y;
  const VbxJob job = vbx_job(b, j);
  const long count = (long)b.N * job.S;
  const double* src = gamma0 + job.gamma0;
  double* dst = b.gamma + (long)j * b.N * b.Smax;
  for (long i = (long)blockIdx.x * VB_T + threadIdx.x; i < count; i += (long)gridDim.x * VB_T) dst[i] = src[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    b.done[j] = job.S == 0;
    b.iterations[j] = 0;
  }
}

__global__ __launch_bounds__(VB_T) void k_vbx_batch_mstep(VbxBatch b, const double* __restrict__ rho,
                                                         const double* __restrict__ Phi) {
  __shared__ double red[VB_T / 64];
  extern __shared__ double part_sm[];
  const int j = blockIdx.y;
  if (b.done[j]) return;
  const VbxJob job = vbx_job(b, j);
  if ((int)blockIdx.x >= job.S) return;
  const long sd = (long)j * b.Smax * b.D, ss = (long)j * b.Smax;
  vbx_mstep_body(blockIdx.x, b.gamma + (long)j * b.N * b.Smax, rho, b.N, job.S, b.D, Phi, job.Fa / job.Fb,
                 b.alpha + sd, b.invL + sd, b.Nk + ss, b.cterm + ss, b.eterm + ss, part_sm, red);
}

__global__ __launch_bounds__(VB_T) void k_vbx_batch_estep(VbxBatch b, const double* __restrict__ rho,
                                                         const double* __restrict__ G, int first) {
  __shared__ double red[VB_T / 64];
  extern __shared__ double sm[];
  const int j = blockIdx.y;
  if (b.done[j]) return;
  const VbxJob job = vbx_job(b, j);
  const long sd = (long)j * b.Smax * b.D, ss = (long)j * b.Smax;
  vbx_estep_body(blockIdx.x, rho, b.alpha + sd, b.cterm + ss, G, b.Nk + ss, first, job.S, b.D, job.Fa,
                 b.gamma + (long)j * b.N * b.Smax, b.logpx + (long)j * b.N, sm, red);
}

// the test of the host loop (clustering.py: `it > 0 and elbo[it] - elbo[it - 1] < epsilon`), in double
__global__ __launch_bounds__(VB_T) void k_vbx_batch_elbo(VbxBatch b, int it, double epsilon) {
  __shared__ double red[VB_T / 64];
  const int j = blockIdx.x;
  if (b.done[j]) return;
  const VbxJob job = vbx_job(b, j);
  const double v = vbx_elbo_body(b.logpx + (long)j * b.N, b.N, b.eterm + (long)j * b.Smax, job.S, job.Fb, red);
  if (threadIdx.x == 0) {
    double* history = b.elbo + (long)j * b.max_iterations;
    history[it] = v;
    b.iterations[j] = it + 1;
    if (it > 0 && v - history[it - 1] < epsilon) b.done[j] = 1;
  }
}

// The workspace of pa_vbx_iteration: the arrays back to back and 64 spare bytes
struct VbxFile {
  double *rho, *G, *logpx, *alpha, *invL, *Nk, *cterm, *eterm;   // (n, d), (n), (n), (s, d) x 2, (s) x 3
};
static VbxFile vbx_file_layout(Carver& c, int n, int s, int d) {
  const size_t N = n, S = s, D = d, packed = sizeof(double);
  VbxFile f;
  f.rho = c.take<double>(N * D, packed);
  f.G = c.take<double>(N, packed);
  f.logpx = c.take<double>(N, packed);
  f.alpha = c.take<double>(S * D, packed);
  f.invL = c.take<double>(S * D, packed);
  f.Nk = c.take<double>(S, packed);
  f.cterm = c.take<double>(S, packed);
  f.eterm = c.take<double>(S, packed);
  c.take<char>(64, packed);
  return f;
}

// The workspace of pa_vbx_run_batch in 256-byte-aligned blocks: rho and G, shared by the jobs, in one block; then per
// array the slabs of all jobs, at the common stride of the largest S of the call; the `done` flags last.  Fills the
// workspace pointers of `b` and returns rho; G follows its n x d doubles.
static double* vbx_batch_layout(Carver& c, int jobs, int n, int smax, int d, VbxBatch& b) {
  const size_t J = jobs, N = n, S = smax, D = d;
  double* rho = c.take<double>(N * D + N);
  b.logpx = c.take<double>(J * N);
  b.alpha = c.take<double>(J * S * D);
  b.invL = c.take<double>(J * S * D);
  b.Nk = c.take<double>(J * S);
  b.cterm = c.take<double>(J * S);
  b.eterm = c.take<double>(J * S);
  b.done = c.take<int>(J);
  return rho;
}

}  // namespace pa

extern "C" {

int pa_plda_transform(const float* X, int n, int din, int dmid, int dout, const double* mean1,
                      const double* lda, const double* mean2, const double* mu, const double* trT,
                      double* fea, void* stream) {
  if (n <= 0) return 0;
  PA_REQUIRE(dout <= dmid && (size_t)(din + dmid) * 8 <= 64 * 1024, "pa_plda_transform: bad dimensions");
  pa::ProfScope prof("k_plda_transform", stream, 2.0 * n * ((double)din * dmid + (double)dmid * dout),
                     4.0 * n * din + 8.0 * n * dout);
  hipLaunchKernelGGL(pa::k_plda_transform, dim3(n), dim3(pa::VB_T), (size_t)(din + dmid) * 8,
                     (hipStream_t)stream, X, din, dmid, dout, mean1, lda, mean2, mu, trT, fea);
  PA_CHECK_LAUNCH("pa_plda_transform");
  return 0;
}

size_t pa_vbx_workspace_bytes(int n, int s, int d) {
  return pa::carved_bytes([&](pa::Carver& c) { pa::vbx_file_layout(c, n, s, d); });
}

// One VB iteration (utils/vbx.py:106-133) on device buffers.  `gamma` (n, s) is read by the M step and
// overwritten by the E step; `elbo_out` receives the value of (25) for the convergence test on the host.
// `first` != 0: first iteration (rho / G are derived from `fea`, speaker priors are uniform).
int pa_vbx_iteration(const double* fea, const double* Phi, int n, int s, int d, double Fa, double Fb,
                     int first, double* gamma, double* elbo_out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  if (n <= 0 || s <= 0) return 0;
  pa::Carver carver(workspace);
  const pa::VbxFile f = pa::vbx_file_layout(carver, n, s, d);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_vbx_iteration: workspace too small");
  PA_REQUIRE((size_t)(d + s) * 8 <= 64 * 1024, "pa_vbx_iteration: too many clusters for one workgroup");
  hipStream_t st = (hipStream_t)stream;
  pa::ProfScope prof("k_vbx_iteration", stream, 4.0 * n * (double)s * d, 8.0 * (2.0 * n * s + 2.0 * n * d));
  if (first) hipLaunchKernelGGL(pa::k_vbx_prepare, dim3(n), dim3(pa::VB_T), 0, st, fea, n, d, Phi, f.rho, f.G);
  hipLaunchKernelGGL(pa::k_vbx_mstep, dim3(s), dim3(pa::VB_T), (size_t)(pa::VB_T / 128) * d * 8, st, gamma, f.rho, n,
                     s, d, Phi, Fa / Fb, f.alpha, f.invL, f.Nk, f.cterm, f.eterm);
  hipLaunchKernelGGL(pa::k_vbx_estep, dim3(n), dim3(pa::VB_T), (size_t)(d + s) * 8, st, f.rho, f.alpha, f.cterm, f.G,
                     f.Nk, first, n, s, d, Fa, gamma, f.logpx);
  hipLaunchKernelGGL(pa::k_vbx_elbo, dim3(1), dim3(pa::VB_T), 0, st, f.logpx, n, f.eterm, s, Fb, elbo_out);
  PA_CHECK_LAUNCH("pa_vbx_iteration");
  return 0;
}

size_t pa_vbx_batch_workspace_bytes(int jobs, int n, int smax, int d) {
  if (jobs <= 0 || n <= 0 || smax <= 0 || d <= 0) return 0;
  pa::VbxBatch b;
  return pa::carved_bytes([&](pa::Carver& c) { pa::vbx_batch_layout(c, jobs, n, smax, d, b); });
}

// Whole VB inferences of `jobs` jobs over the same features `fea` (n, d), no read-back and no host
// synchronisation: job j starts from the (n, S_j) responsibilities at gamma0 + job_init[2 j] (read-only; several
// jobs may name the same ones), S_j = job_init[2 j + 1] <= smax, and runs with Fa = job_f[2 j], Fb = job_f[2 j + 1]
// (both tables on the device).  `max_iterations` rounds are enqueued; a job whose ELBO gain falls below `epsilon`
// stops taking part.  gamma (jobs, n * smax): job j's final (n, S_j) responsibilities, contiguous at the start
// of its slab; elbo (jobs, max_iterations): the history, valid up to iterations[j] (int32, jobs; 0 for a job
// whose table entry is out of range, which is left alone).  Per job, bit for bit what `max_iterations` calls
// of pa_vbx_iteration with the host's test give.
int pa_vbx_run_batch(const double* fea, const double* Phi, int n, int d, int jobs, const double* gamma0,
                     long gamma0_len, const int64_t* job_init, const double* job_f, int smax,
                     int max_iterations, double epsilon, double* gamma, double* elbo, int32_t* iterations,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (n <= 0 || jobs <= 0) return 0;
  PA_REQUIRE(d == 128, "pa_vbx_run_batch: the PLDA space has 128 dimensions");
  PA_REQUIRE(jobs <= 65535 && max_iterations >= 1, "pa_vbx_run_batch: bad job or iteration count");
  PA_REQUIRE(smax >= 1 && (size_t)(d + smax) * 8 <= 64 * 1024,
             "pa_vbx_run_batch: too many clusters for one workgroup");
  pa::Carver carver(workspace);
  pa::VbxBatch b;
  double* rho = pa::vbx_batch_layout(carver, jobs, n, smax, d, b);
  double* G = rho + (size_t)n * d;
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_vbx_run_batch: workspace too small");
  b.job_init = job_init;
  b.job_f = job_f;
  b.gamma0_len = gamma0_len;
  b.gamma = gamma;
  b.elbo = elbo;
  b.iterations = iterations;
  b.N = n, b.D = d, b.Smax = smax, b.max_iterations = max_iterations;
  hipStream_t st = (hipStream_t)stream;
  pa::ProfScope prof("k_vbx_run_batch", stream, 4.0 * n * (double)smax * d * jobs * max_iterations,
                     8.0 * jobs * max_iterations * (2.0 * n * smax + 2.0 * n * d));
  hipLaunchKernelGGL(pa::k_vbx_prepare, dim3(n), dim3(pa::VB_T), 0, st, fea, n, d, Phi, rho, G);
  const int copy_blocks = (int)std::min<size_t>(64, ((size_t)n * smax + pa::VB_T - 1) / pa::VB_T);
  hipLaunchKernelGGL(pa::k_vbx_batch_begin, dim3(copy_blocks, jobs), dim3(pa::VB_T), 0, st, b, gamma0);
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(pa::k_vbx_batch_mstep, dim3(smax, jobs), dim3(pa::VB_T), (size_t)(pa::VB_T / 128) * d * 8,
                       st, b, rho, Phi);
    hipLaunchKernelGGL(pa::k_vbx_batch_estep, dim3(n, jobs), dim3(pa::VB_T), (size_t)(d + smax) * 8, st, b, rho,
                       G, (int)(it == 0));
    hipLaunchKernelGGL(pa::k_vbx_batch_elbo, dim3(jobs), dim3(pa::VB_T), 0, st, b, it, epsilon);
  }
  PA_CHECK_LAUNCH("pa_vbx_run_batch");
  return 0;
}

}  // extern "C"
