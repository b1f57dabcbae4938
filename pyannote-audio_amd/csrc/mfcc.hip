// torchaudio.transforms.MFCC, the front end of XVectorMFCC (models/embedding/xvector.py:42-60, 198), on gfx950.
// What it computes (torchaudio's MFCC with n_fft = win_length = 400, power 2, onesided, not normalized):
//   frames of 400 samples every `hop` samples, reflect-padded by 200 on each side of the chunk when centred (the
//   chunk alone: samples of the neighbouring audio are never used; samples past the end of the waveform read as
//   zero BEFORE the reflection, as the reference zero-pads the last chunk) -> window -> |rfft|^2 -> mel filter bank
//   -> 10 log10(max(x, 1e-10)) clamped from below at (max over the chunk) - 80 dB, or log(x + 1e-6) -> DCT.
//
//   k_mfcc_mel   one wave per frame: gather + window, 400-point real DFT as a 200-point complex Stockham FFT
//                (radices 8, 5, 5) in LDS + real unpack, power, sparse mel projection over the non-zero range of
//                each filter, dB (or log).  The largest mel energy of each chunk goes to an atomicMax on its bit
//                pattern (non-negative floats order like their bits; dB is monotonic in the energy, so the
//                chunk's largest dB value is the dB of that energy).
//   k_mfcc_dct   top_db clamp, DCT-II (dct_mat [n_mels][64], zero past n_mfcc), written as the TDNN input rows
//                [(tile, t, b16)][64] (columns n_mfcc..63 and chunks >= B written as zero) or as (B, T, n_mfcc).
#include "common.h"

namespace pa {

constexpr int MF_NFFT = 400, MF_HALF = 200, MF_NBIN = 201, MF_FPB = 4, MF_MAXMEL = 256, MF_DCT_LD = 64;
constexpr int MF_DCT_TT = 16;   // frames per k_mfcc_dct block

__device__ __forceinline__ float2 mf_cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// one radix-R pass of the 200-point Stockham FFT (Ns = product of the radices already done); butterfly j = lane.
// tw[m] = exp(-2 pi i m / 200): the inter-pass twiddle exp(-2 pi i r k / (Ns R)) and the DFT-R kernel
// exp(-2 pi i r q / R) are both entries of it (Ns R divides 200).
template <int R, int Ns>
__device__ __forceinline__ void mf_pass(const float2* src, float2* dst, const float2* tw, int lane) {
  constexpr int NB = MF_HALF / R;
  if (lane < NB) {
    const int j = lane, k = j % Ns;
    float2 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = src[j + r * NB];
      if (r > 0 && Ns > 1) v[r] = mf_cmul(v[r], tw[(r * k * (MF_HALF / (Ns * R))) % MF_HALF]);
    }
    const int j0 = (j / Ns) * Ns * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float2 y = v[0];
#pragma unroll
      for (int r = 1; r < R; ++r) {
        const float2 c = mf_cmul(v[r], tw[((r * q) % R) * (MF_HALF / R)]);
        y.x += c.x;
        y.y += c.y;
      }
      dst[j0 + q * Ns] = y;
    }
  }
}

// grid = (ceil(T / 4), B), block = 256 (4 waves, one frame each).  mel_out: (B, T, nmel) dB or log values;
// chunk_max: B uints, zeroed by the caller (only written when !log_mels).
__global__ __launch_bounds__(256) void k_mfcc_mel(const float* __restrict__ wav, long wav_len, long chunk_stride,
                                                  int N, int T, int hop, int center, int log_mels,
                                                  const float* __restrict__ window, const float2* __restrict__ tw200,
                                                  const float2* __restrict__ tw400, const float* __restrict__ mel_w,
                                                  const int* __restrict__ mel_lo, const int* __restrict__ mel_hi,
                                                  int nmel, float* __restrict__ mel_out,
                                                  unsigned int* __restrict__ chunk_max) {
  __shared__ float2 bufA[MF_FPB][MF_HALF];
  __shared__ float2 bufB[MF_FPB][MF_HALF];
  __shared__ float2 s_tw[MF_HALF];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y;
  const int t = blockIdx.x * MF_FPB + wv;
  const bool active = t < T;
  for (int i = tid; i < MF_HALF; i += 256) s_tw[i] = tw200[i];
  float2 w400[4];   // twiddles of the real unpack: fetched now, used after the FFT
#pragma unroll
  for (int i = 0; i < 4; ++i) w400[i] = lane + 64 * i < MF_NBIN ? tw400[lane + 64 * i] : make_float2(0.f, 0.f);

  // ---- gather + window, packed as 200 complex z[n] = x[2n] + i x[2n + 1]
  const long base = (long)b * chunk_stride;
  const long f0 = (long)t * hop - (center ? MF_NFFT / 2 : 0);   // first sample of the frame, before reflection
  float2* A = bufA[wv];
  float2* Bf = bufB[wv];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = lane + 64 * i;
    if (n < MF_HALF) {
      float v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        long j = f0 + 2 * n + h;
        if (j < 0) j = -j;                      // reflection (only centred frames start before 0; N > 200)
        if (j >= N) j = 2L * (N - 1) - j;
        const long g = base + j;
        v[h] = active && g < wav_len ? wav[g] * window[2 * n + h] : 0.f;
      }
      A[n] = make_float2(v[0], v[1]);
    }
  }
  __syncthreads();
  // ---- 200-point complex FFT: radix 8, 5, 5 (A -> B -> A -> B)
  mf_pass<8, 1>(A, Bf, s_tw, lane);
  __syncthreads();
  mf_pass<5, 8>(Bf, A, s_tw, lane);
  __syncthreads();
  mf_pass<5, 40>(A, Bf, s_tw, lane);
  __syncthreads();
  // ---- real unpack -> power spectrum P[0..200] (into A, read as floats)
  float* P = reinterpret_cast<float*>(A);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    if (k < MF_NBIN) {
      const float2 zk = Bf[k % MF_HALF];
      const float2 zc0 = Bf[(MF_HALF - k) % MF_HALF];
      const float2 zc = make_float2(zc0.x, -zc0.y);
      const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
      const float2 dd = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
      const float2 o = make_float2(dd.y, -dd.x);   // -i * dd
      const float2 wo = mf_cmul(o, w400[i]);
      const float re = e.x + wo.x, im = e.y + wo.y;
      P[k] = re * re + im * im;
    }
  }
  __syncthreads();
  // ---- mel projection + dB / log
  float emax = 0.f;
  if (active) {
    for (int m = lane; m < nmel; m += 64) {
      const float* wrow = mel_w + (long)m * MF_NBIN;
      float acc = 0.f;
      const int lo = mel_lo[m], hi = mel_hi[m];   // lo > hi: an all-zero filter, energy exactly 0
      for (int k0 = lo; k0 <= hi; k0 += 8) {      // eight weights in flight per trip, the sum in ascending k
        float wk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wk[u] = k0 + u <= hi ? wrow[k0 + u] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + u <= hi) acc = fmaf(P[k0 + u], wk[u], acc);
      }
      const float e = fmaxf(acc, 1e-10f);
      emax = fmaxf(emax, e);
      mel_out[((long)b * T + t) * nmel + m] = log_mels ? logf(acc + 1e-6f) : 10.f * log10f(e);
    }
  }
  if (!log_mels) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) emax = fmaxf(emax, __shfl_xor(emax, o, 64));
    if (active && lane == 0) atomicMax(chunk_max + b, __float_as_uint(emax));
  }
}

// grid = (ceil(T / 16), Bg), block = 256: 64 output columns x 4 frame lanes, 4 frames each.  kRows: Bg = chunks
// rounded up to 16 and out = the TDNN input rows [(tile, t, b16)][64]; otherwise Bg = B and out = (B, T, n_mfcc).
template <bool kRows>
__global__ __launch_bounds__(256) void k_mfcc_dct(const float* __restrict__ mel, int B, int T, int nmel, int n_mfcc,
                                                  int log_mels, const unsigned int* __restrict__ chunk_max,
                                                  const float* __restrict__ dct, float* __restrict__ out) {
  __shared__ float v[MF_DCT_TT][MF_MAXMEL + 1];
  const int b = blockIdx.y, t0 = blockIdx.x * MF_DCT_TT;
  const int tid = threadIdx.x;
  const bool real = b < B;
  // top_db: max(x_db, max over the chunk - 80), the max taken in dB of the largest energy
  const float floor_db = !log_mels && real ? 10.f * log10f(fmaxf(__uint_as_float(chunk_max[b]), 1e-10f)) - 80.f
                                           : -__builtin_inff();
  for (int i = tid; i < MF_DCT_TT * nmel; i += 256) {
    const int tt = i / nmel, m = i - tt * nmel;
    float x = 0.f;
    if (real && t0 + tt < T) x = fmaxf(mel[((long)b * T + t0 + tt) * nmel + m], floor_db);
    v[tt][m] = x;
  }
  __syncthreads();
  const int c = tid & 63, f = tid >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int m = 0; m < nmel; ++m) {
    const float d = dct[m * MF_DCT_LD + c];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(v[f + 4 * u][m], d, acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = t0 + f + 4 * u;
    if (t >= T) continue;
    if constexpr (kRows) {
      out[(((long)(b >> 4) * T + t) * 16 + (b & 15)) * MF_DCT_LD + c] = real && c < n_mfcc ? acc[u] : 0.f;
    } else {
      if (c < n_mfcc) out[((long)b * T + t) * n_mfcc + c] = acc[u];
    }
  }
}

}  // namespace pa

// the front end for pa_xvec_mfcc_forward / pa_mfcc_features (csrc/xvec_forward.cpp).  mel_buf (B, T, nmel) and
// chunk_max (B) are scratch; rows = 1: out = the TDNN input rows of ceil(B / 16) tiles, else (B, T, n_mfcc).
// fft_tw: 200 complex exp(-2 pi i m / 200), then 201 complex exp(-2 pi i k / 400).
PA_INTERNAL int pa_mfcc_frontend(const float* wav, long wav_len, long chunk_stride, int B, int N, int T, int hop,
                                 int center, int log_mels, const float* window, const float* fft_tw,
                                 const float* mel_w, const int* mel_lo, const int* mel_hi, int nmel,
                                 const float* dct, int n_mfcc, float* mel_buf, unsigned int* chunk_max, float* out,
                                 int rows, void* stream) {
  PA_REQUIRE(nmel >= 1 && nmel <= pa::MF_MAXMEL && n_mfcc >= 1 && n_mfcc <= pa::MF_DCT_LD && hop >= 1 &&
                 hop <= pa::MF_NFFT,
             "pa_mfcc: 1 <= n_mels <= %d, 1 <= n_mfcc <= %d and 1 <= hop_length <= %d required (got %d, %d, %d)",
             pa::MF_MAXMEL, pa::MF_DCT_LD, pa::MF_NFFT, nmel, n_mfcc, hop);
  PA_REQUIRE(center ? N > pa::MF_NFFT / 2 : N >= pa::MF_NFFT,
             "pa_mfcc: %d samples is too short for one %s400-sample frame", N, center ? "reflect-padded " : "");
  const int expect = center ? 1 + N / hop : 1 + (N - pa::MF_NFFT) / hop;
  PA_REQUIRE(T == expect, "pa_mfcc: %d frames given, %d expected", T, expect);
  if (B <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  {
    pa::ProfScope prof("k_mfcc_mel", stream, (double)B * T * (5.0 * 400 * 8 + 8.0 * 201 + 2.0 * 201 * 2),
                       4.0 * B * N + 4.0 * B * T * nmel);
    if (!log_mels && pa::fill_async(chunk_max, 0, sizeof(unsigned int) * B, st) != hipSuccess) {
      pa::set_error("pa_mfcc: the fill launch failed");
      return 1;
    }
    hipLaunchKernelGGL(pa::k_mfcc_mel, dim3(pa::cdiv(T, pa::MF_FPB), B), dim3(256), 0, st, wav, wav_len,
                       chunk_stride, N, T, hop, center, log_mels, window, (const float2*)fft_tw,
                       (const float2*)(fft_tw + 2 * pa::MF_HALF), mel_w, mel_lo, mel_hi, nmel, mel_buf, chunk_max);
    PA_CHECK_LAUNCH("pa_mfcc_mel");
  }
  const int Bg = rows ? pa::cdiv(B, 16) * 16 : B;
  pa::ProfScope prof("k_mfcc_dct", stream, 2.0 * B * T * nmel * n_mfcc, 4.0 * B * T * nmel + 4.0 * Bg * T * 64);
  if (rows)
    hipLaunchKernelGGL(pa::k_mfcc_dct<true>, dim3(pa::cdiv(T, pa::MF_DCT_TT), Bg), dim3(256), 0, st, mel_buf, B, T,
                       nmel, n_mfcc, log_mels, chunk_max, dct, out);
  else
    hipLaunchKernelGGL(pa::k_mfcc_dct<false>, dim3(pa::cdiv(T, pa::MF_DCT_TT), Bg), dim3(256), 0, st, mel_buf, B, T,
                       nmel, n_mfcc, log_mels, chunk_max, dct, out);
  PA_CHECK_LAUNCH("pa_mfcc_dct");
  return 0;
}
