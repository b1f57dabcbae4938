// pa_gather_chunks: chunks of several device-resident waveforms -> one dense (num_chunks, num_samples) buffer.
//
//   out[c][i] = wav[file[c]][start[c] + i]   where start[c] + i < len[file[c]],   0 elsewhere
//   (start[c] >= 0; a chunk with a negative start is written as zeros, nothing is read for it)
//
// What a launch group of the embedding network reads when its chunks come from several files (or are a selection of
// one file's): it replaces pad + unfold + index + contiguous per file by one pass that reads every selected sample
// once and writes it once.  Purely bandwidth-bound, no arithmetic.
//
//   grid = (num_chunks, ceil(num_samples / GATHER_SLICE)), block = 256; a workgroup copies one slice of one chunk.
//   A thread moves 16 bytes at a time where the chunk's source address (file base + start) and its output row are
//   both 16-byte aligned -- the chunk grid of the pipeline (starts and window that are multiples of 4 samples, bases
//   from the allocator) always is -- and the group of four lies inside the file and the window; the groups on the
//   file's end or the window's end, and every chunk that is not aligned, go sample by sample (still coalesced).
//   Plain stores: the fbank kernel reads the buffer next.
#include "common.h"

namespace pa {

typedef float __attribute__((address_space(1))) global_f32;
typedef f32x4 __attribute__((address_space(1))) global_f32x4;

constexpr int GATHER_VEC = 4;                          // floats per 16-byte access
constexpr int GATHER_PER_THREAD = 4;                   // 16-byte accesses per thread
constexpr int GATHER_SLICE = 256 * GATHER_VEC * GATHER_PER_THREAD;   // samples per workgroup

__global__ __launch_bounds__(256) void k_gather_chunks(const float* const* __restrict__ file_ptr,
                                                        const int64_t* __restrict__ file_len,
                                                        const int32_t* __restrict__ chunk_file,
                                                        const int64_t* __restrict__ chunk_start, int num_samples,
                                                        float* __restrict__ out) {
  const int c = blockIdx.x;
  const int f = chunk_file[c];
  const float* base = file_ptr[f];
  const int64_t start = chunk_start[c];
  // samples of this chunk that exist in the file: [0, have)
  const int64_t left = file_len[f] - start;
  const int have = (start < 0 || left <= 0) ? 0 : (left >= num_samples ? num_samples : (int)left);
  // (a pointer read from a table is generic to the compiler: say that it is global memory, or every load is a flat one)
  const global_f32* src = (const global_f32*)(base + start);   // (only dereferenced below `have`)
  float* dst = out + (size_t)c * num_samples;
  const int i0 = blockIdx.y * GATHER_SLICE;
  const bool aligned = have > 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;   // (uniform)
  if (aligned) {
    f32x4 v[GATHER_PER_THREAD];
#pragma unroll
    for (int k = 0; k < GATHER_PER_THREAD; ++k) {      // all loads first
      const int i = i0 + GATHER_VEC * (threadIdx.x + 256 * k);
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i + GATHER_VEC <= have) {
        v[k] = *(const global_f32x4*)(src + i);
      } else {
#pragma unroll
        for (int j = 0; j < GATHER_VEC; ++j)
          if (i + j < have) v[k][j] = src[i + j];
      }
    }
#pragma unroll
    for (int k = 0; k < GATHER_PER_THREAD; ++k) {
      const int i = i0 + GATHER_VEC * (threadIdx.x + 256 * k);
      if (i + GATHER_VEC <= num_samples) {
        *reinterpret_cast<f32x4*>(dst + i) = v[k];
      } else {
#pragma unroll
        for (int j = 0; j < GATHER_VEC; ++j)
          if (i + j < num_samples) dst[i + j] = v[k][j];
      }
    }
    return;
  }
  const int i1 = min(i0 + GATHER_SLICE, num_samples);
  for (int i = i0 + threadIdx.x; i < i1; i += 256) dst[i] = i < have ? src[i] : 0.f;
}

}  // namespace pa

extern "C" {

int pa_gather_chunks(const float* const* file_ptr, const int64_t* file_len, const int32_t* chunk_file,
                     const int64_t* chunk_start, int num_chunks, int num_samples, float* out, void* stream) {
  if (num_chunks <= 0 || num_samples <= 0) return 0;
  const int slices = pa::cdiv(num_samples, pa::GATHER_SLICE);
  PA_REQUIRE(slices <= 65535, "pa_gather_chunks: chunks of %d samples are too long", num_samples);
  pa::ProfScope prof("k_gather_chunks", stream, 0.0, 8.0 * num_chunks * num_samples);
  hipLaunchKernelGGL(pa::k_gather_chunks, dim3(num_chunks, slices), dim3(256), 0, (hipStream_t)stream, file_ptr,
                     file_len, chunk_file, chunk_start, num_samples, out);
  PA_CHECK_LAUNCH("pa_gather_chunks");
  return 0;
}

}  // extern "C"
