// pa::fill_async: every byte of [dst, dst + nbytes) <- value, as a kernel on the caller's stream.  It stands where the
// launchers used to call hipMemsetAsync.  Reason ("The stream contract"): the header promises that every
// asynchronous entry point can be captured into a graph and replayed.  A captured hipMemsetAsync became a memset node
// that wrote zeros on the first replay and a 16-byte pattern of stale words on the second one (MI355X, ROCm 7.0:
// tests/test_stream_contract_gpu.py, seven entry points whose result depends on the zeros); a kernel node replays
// with the arguments it was captured with.  The cost is that of the memset, which is a fill kernel of the runtime.
//
//   grid <= 4096 x 256 threads, grid-stride over 16-byte stores; the bytes in front of the first 16-byte boundary and
//   behind the last one are written one by one by the first threads.  Nothing outside the range is touched.
#include "common.h"

namespace pa {

__global__ __launch_bounds__(256) void k_fill_bytes(unsigned char* __restrict__ dst, unsigned int word, size_t head,
                                                     size_t body, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const u32x4 v = {word, word, word, word};
  u32x4* b = reinterpret_cast<u32x4*>(dst + head);
  for (size_t k = i; k < body; k += stride) b[k] = v;
  const size_t tail0 = head + 16 * body;      // head < 16 and n - tail0 < 16: the first threads of the grid
  if (i < head) dst[i] = (unsigned char)word;
  if (i < n - tail0) dst[tail0 + i] = (unsigned char)word;
}

hipError_t fill_async(void* dst, int value, size_t nbytes, hipStream_t st) {
  if (nbytes == 0) return hipSuccess;
  if (dst == nullptr) return hipErrorInvalidValue;
  size_t head = (16 - (size_t)((uintptr_t)dst & 15)) & 15;
  if (head > nbytes) head = nbytes;
  const size_t body = (nbytes - head) / 16;
  size_t blocks = (body + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(k_fill_bytes, dim3((unsigned)blocks), dim3(256), 0, st, (unsigned char*)dst,
                     0x01010101u * (unsigned)(value & 0xff), head, body, nbytes);
  return hipGetLastError();
}

}  // namespace pa
