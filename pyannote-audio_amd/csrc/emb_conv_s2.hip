// The three block-entry convolutions of the WeSpeaker ResNet34 (3x3, pad 1, stride 2: 32->64, 64->128, 128->256;
// reference: models/embedding/wespeaker/resnet.py:84-145) as an implicit GEMM on v_mfma_f32_32x32x2_f32 with the data
// path of the Winograd kernels (emb_winograd4.hip): behind pa_conv3x3(..., stride = 2, ...), same weight image
// [9][COUT][CIN], same accumulation order as the kernel it replaces (the stride-2 form of k_conv3x3, emb_resnet.hip up to
// revision 56a8a7a; tools/build_variants.py conv_s2_parent) -- 16-channel blocks outermost, the 9 taps inside, 8 k-steps
// with channel 8 (lane >> 5) + q in step q -- so every output is the same chain of MFMAs and the results are
// bit-identical to that kernel's.
//
//   * ONE workgroup of 4 waves per CU (two stages of patch + weights fill the LDS), a tile of 128 output pixels x 64
//     output channels: wave w owns the 32-pixel M-tile w and BOTH 32-channel N-tiles, so an A fragment read from LDS
//     feeds two MFMAs and the patch of a pixel tile is staged by COUT / 64 workgroups instead of COUT / 32.
//     __launch_bounds__(256, 2) although only one workgroup fits a CU: with a budget of 256 registers the compiler
//     keeps the 32 accumulators in architectural registers (VGPR-form MFMAs); with 512 it moved them between VGPRs
//     and AccVGPRs around every stage (64 v_accvgpr instructions per stage, +0.5-2 % per launch).  180 are used.
//   * staging is LDS-DMA (buffer_load_dwordx4 ... lds), double-buffered: the 1 KB pieces of stage s + 1 -- of the next
//     tile's first stage in a tile's last run -- are issued from inside the MFMA run of stage s, one behind every
//     sixth MFMA, as inline assembly with scalar-only set-up (M0 = base + immediate).  The column-parity de-interleave
//     and the bank swizzle are made by the lanes' source offsets (emb_conv_s2_geom.h); halo, out-of-image and padding
//     lanes carry an out-of-bounds offset and the hardware writes the zeros.  No ds_write, no staging registers.
//   * one workgroup barrier per stage: "my pieces of this stage have landed" (s_waitcnt vmcnt) + "everybody's have, and
//     everybody is done reading the other buffer".  A tile's first stage was issued in FRONT of the previous tile's
//     epilogue, whose 32 output stores per lane are newer: vmcnt(32) there, the stores stay in flight.
//   * fragments are read with ds_read_b128 through volatile LDS pointers, those of tap + 1 under the MFMAs of tap;
//     conflict-free by the swizzle under the hardware's lane-group rule (tests/test_conv_s2_geometry_cpu.py).  The
//     20 read pointers of a lane point into the CURRENT buffer and move behind every run (one copy of the run).
//   * tiles are claimed at run time in the XCD-aware order of k_conv3x3 (tile_queue.h); the claim of the tile after
//     the next is issued by thread 0 between a tile's last run and its epilogue and used in the next tile's last
//     stage.  (The compiler rewrites the atomicAdd of a uniform address into one atomic per wave + v_readfirstlane and
//     waits for it at once with vmcnt(0): wave 0 therefore waits there for the staging just issued before it starts
//     its epilogue, and its vmcnt(32) at the next tile's top finds nothing left to wait for; waves 1-3 do not.)
//
// Measured against k_conv3x3<2, ...> of the parent commit, alternating in one call (profiles/conv_s2_dma_ab.txt), 512
// chunks per launch: 80x998 32->64 4.02 -> 3.43 ms (0.60 -> 0.70 of the f32 MFMA peak), 40x499 64->128 3.45 -> 3.03
// (0.70 -> 0.79), 20x250 128->256 3.24 -> 2.84 (0.74 -> 0.85); bench.py 752.4 / 753.0 -> 744.9 / 742.6 ms per file.
// Outputs bit-identical to the parent kernel's: run side by side on every stride-2 launch of the benchmark's pipeline
// (3 591 chunks per launch, its real activations) 0 of 8.0 G outputs per file differ.
//
// SC = 1 (k_conv3x3_s2<4, 1, false, 1> behind pa_conv3x3_s2_sc, emb_resnet.hip): the entry of a stride-2 BasicBlock in
// one launch.  The block's 1x1 stride-2 shortcut reads pixel (2 y, 2 x) of the same map -- the centre tap (tap 4) of this
// convolution, which is in LDS in A-fragment layout in every stage -- so it is a TENTH tap with weights and
// accumulators of its own instead of a k_gemm_tn launch that reads the map again:
//   * the weight slab has a tenth 4-KB tap (entries 9 * 64 + n, same swizzle, tap and N-tile still ds_read
//     immediates), filled by each wave's LAST weight piece from the plain [COUT][CIN] shortcut image through a
//     descriptor of its own: 20 pieces per wave and stage in the run's 27 issue slots, 2 x (38 + 40) KB + the mailbox of
//     the 160 KB of LDS.  The <2, 2> geometry (Ho < 16: the layer-4 entry) would need 162 KB and keeps its GEMM.
//   * the run has 16 more MFMAs at its end, on the A fragments of tap 4 (read again) and the B fragments of the new
//     tap, into acc_sc; no DMA slot of their own.  The nine-tap chain into acc is unchanged: Y keeps its bits.  The
//     shortcut's chain: 16-channel blocks ascending, 8 k-steps pairing channels q and 8 + q, from zero, shift_sc added
//     in the epilogue -- not k_gemm_tn's pairing, so Ysc has other last bits than pa_gemm_tn_s2's (measured against the
//     float64 truth: 0.022 / 0.042 of the contract where the GEMM has 0.021 / 0.052).
//   * the epilogue stores acc_sc + shift_sc (no ReLU, no residual) to Ysc at Y's offsets: 64 whole-line stores per lane
//     behind the next tile's staging, so the first-stage wait is vmcnt(63), the largest the encoding has.
// ISA of that instantiation: 180 VGPRs (147 without the shortcut, 175 with a residual input), 0 AccVGPRs, no scratch, no
// spilled VGPR; one copy of the run: 160 v_mfma_f32_32x32x2_f32, 60
// ds_read_b128 (54 inside the run), 20 buffer_load_dwordx4 ... lds in the run + 20 in the prologue, 64 buffer_store_dword,
// 313 instructions from the run's first MFMA to its last (284 without the shortcut).  The SC = 0 instantiations have the
// instruction counts they had.
// Measured, fused against pa_conv3x3(stride 2) + pa_gemm_tn_s2 alternating in one call, 512 chunks per launch, two
// passes each (profiles/conv_s2_shortcut_ab.txt): 80x998 32->64 4.720 / 4.699 -> 3.925 / 3.926 ms per block entry
// (convolution 3.42 -> 3.93, GEMM 1.29 -> 0), 40x499 64->128 3.567 / 3.576 -> 3.393 / 3.395 (3.01 -> 3.39, 0.56 -> 0):
// both shapes keep the fused path.  Per file: k_conv3x3_s2<4, 1> 45.8 -> 51.8 ms, k_gemm_tn<0, 0> 16.7 -> 3.4 ms, 7.3 ms
// less; bench.py 743.37 / 743.07 -> 734.93 / 737.35 ms per file.  With all 160 KB of LDS taken, a kernel of another
// stream that needs more than 4 KB of LDS waits for the end of the launch (21.6 ms) instead of running beside it: the
// pipelined back end of the previous file (rocprim's partition kernel behind torch.nonzero) takes about 270 instead of
// 190 ms, still hidden behind the 730 ms front end of the next file.
#include "common.h"
#include "emb_conv_s2_geom.h"

namespace pa {

typedef __attribute__((address_space(3))) unsigned char* cs2_lds_t;
// ds_read_b128 that stays one instruction at its place (volatile, through an explicit LDS pointer)
typedef const volatile f32x4 __attribute__((address_space(3))) * cs2_lds_f32x4_ptr;
__device__ __forceinline__ f32x4 cs2_lds_read128(cs2_lds_t p) { return *(cs2_lds_f32x4_ptr)p; }

__device__ __forceinline__ void cs2_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The first-stage wait of a tile counts vector-memory operations (they complete in order): the epilogue issues
// TILE_STORES output stores per lane behind the staging of the next tile, whatever else it loads.  The static_assert
// ties the literal to that constant, not to what the compiler emits: vmcnt(32) is right only while every wave issues
// at least 32 vector-memory instructions behind the staging (today: 32 unmerged buffer_store_dword).  Re-read the
// epilogue in the ISA whenever it changes.
#define CS2_STR2(x) #x
#define CS2_STR(x) CS2_STR2(x)
#define CS2_TAIL_WAIT_LIT 32
static_assert(ConvS2Geom<4, 1>::TILE_STORES == CS2_TAIL_WAIT_LIT && ConvS2Geom<2, 2>::TILE_STORES == CS2_TAIL_WAIT_LIT,
              "the literal of the s_waitcnt string");
// With the shortcut folded in (SC = 1) the epilogue issues 64 stores per lane behind the staging -- 32 of each output,
// unmerged buffer_store_dword again -- and vmcnt encodes 63 at most: vmcnt(63) then waits for the staging AND the
// oldest of those stores.  Right while at least 63 vector-memory instructions follow the staging.
#define CS2_TAIL_WAIT_LIT_SC 63
static_assert(CS2_TAIL_WAIT_LIT_SC <= 63 && ConvS2Geom<4, 1, 1>::TILE_STORES >= CS2_TAIL_WAIT_LIT_SC &&
                  ConvS2Geom<4, 1, 1>::TILE_STORES == 2 * CS2_TAIL_WAIT_LIT,
              "the literal of the s_waitcnt string, shortcut folded in: both outputs' stores");
static_assert(ConvS2Geom<4, 1>::NPW <= CS2_SLOTS && ConvS2Geom<2, 2>::NPW <= CS2_SLOTS &&
                  ConvS2Geom<4, 1, 1>::NPW <= CS2_SLOTS,
              "a slot of the MFMA run per piece");

// one LDS-DMA piece: M0 = dst + delta (an immediate, or a scalar for the clamped last patch piece); `voff` = the
// lane's source offset, `soff` = the stage's channel offset in bytes.  s_add_u32 writes SCC: declared, the compiler
// does keep SCC live across other statements of this kernel.  M0 cannot be named in a clobber list (it is reserved);
// it is written and read inside the one statement and the compiler keeps nothing in it between LDS instructions.
template <int IMM>
__device__ __forceinline__ void cs2_piece(unsigned dst, int voff, __amdgpu_buffer_rsrc_t srd, int soff) {
  asm volatile("s_add_u32 m0, %0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds"
               :: "s"(dst), "i"(IMM), "v"(voff), "s"(srd), "s"(soff)
               : "memory", "scc");
}
__device__ __forceinline__ void cs2_piece_s(unsigned dst, int delta, int voff, __amdgpu_buffer_rsrc_t srd, int soff) {
  asm volatile("s_add_u32 m0, %0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds"
               :: "s"(dst), "s"(delta), "v"(voff), "s"(srd), "s"(soff)
               : "memory", "scc");
}
struct Cs2Stage {          // wave-uniform
  __amdgpu_buffer_rsrc_t xsrd, wsrd, scsrd;   // scsrd: the shortcut's [COUT][CIN] image (SC = 1 only)
  int soff;
  unsigned pdst, wdst;     // LDS byte address of the buffers being filled + 1024 * wave
  int last_delta;          // of the wave's last patch piece (conv_s2_patch_piece)
};
template <class G, int N>
__device__ __forceinline__ void cs2_issue(const Cs2Stage& st, const int (&poff)[G::PPW], const int (&woff)[G::WPW]) {
  if constexpr (N < G::PPW - 1) cs2_piece<4096 * N>(st.pdst, poff[N], st.xsrd, st.soff);
  else if constexpr (N == G::PPW - 1) cs2_piece_s(st.pdst, st.last_delta, poff[N], st.xsrd, st.soff);
  else if constexpr (G::SC && N == G::NPW - 1) cs2_piece<4096 * (N - G::PPW)>(st.wdst, woff[N - G::PPW], st.scsrd, st.soff);
  else if constexpr (N < G::NPW) cs2_piece<4096 * (N - G::PPW)>(st.wdst, woff[N - G::PPW], st.wsrd, st.soff);
}
// (the piece number is a constant after unrolling: the switch folds)
template <class G>
__device__ __forceinline__ void cs2_issue_n(const int n, const Cs2Stage& st, const int (&poff)[G::PPW],
                                            const int (&woff)[G::WPW]) {
  switch (n) {
#define CS2_CASE(I) case I: cs2_issue<G, I>(st, poff, woff); break;
    CS2_CASE(0) CS2_CASE(1) CS2_CASE(2) CS2_CASE(3) CS2_CASE(4) CS2_CASE(5) CS2_CASE(6) CS2_CASE(7) CS2_CASE(8)
    CS2_CASE(9) CS2_CASE(10) CS2_CASE(11) CS2_CASE(12) CS2_CASE(13) CS2_CASE(14) CS2_CASE(15) CS2_CASE(16)
    CS2_CASE(17) CS2_CASE(18) CS2_CASE(19) CS2_CASE(20) CS2_CASE(21) CS2_CASE(22) CS2_CASE(23) CS2_CASE(24)
    CS2_CASE(25) CS2_CASE(26)
#undef CS2_CASE
    default: break;
  }
}

template <int TH, int TWT, bool HAS_R, int SC>
__global__ __launch_bounds__(256, 2) void k_conv3x3_s2(const float* __restrict__ X, int H, int W, int CIN,
                                                       const float* __restrict__ Wg,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ R, float* __restrict__ Y, int Ho,
                                                       int Wo, int COUT, int relu, int tiles_w, int tiles_hw,
                                                       int n_tiles, int total_tiles, int xranges,
                                                       int* __restrict__ counters, const float* __restrict__ Wsc,
                                                       const float* __restrict__ shift_sc,
                                                       float* __restrict__ Ysc) {
  using G = ConvS2Geom<TH, TWT, SC>;
  static_assert(!(SC && HAS_R), "a block entry has no residual input");
  constexpr int NT = G::WTAPS;   // taps of the run: tap 9 (SC) is the shortcut, on the A fragments of tap 4
  constexpr int BN = CS2_BN;
  constexpr int OOB = CS2_OOB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_s2[];
  const cs2_lds_t lds = (cs2_lds_t)smem_s2;
  const unsigned lds0 = (unsigned)(size_t)lds;
  int* mail = reinterpret_cast<int*>(smem_s2 + G::LDS_BYTES);   // two slots, by tile parity

  const int tid = threadIdx.x, lane = tid & 63;
  const int slw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;

  struct Tile {
    int b, n0, y0, x0;
  };
  // tile order and hole handling of k_conv3x3 (emb_resnet.hip): tile t runs on XCD t % 8 and the n_tiles cout slices
  // of a (pixel tile, image) pair are consecutive claims of one XCD
  const int num_pb = total_tiles / n_tiles;
  auto pair_of = [&](int t) {
    return xranges ? (t & 7) * ((num_pb + 7) >> 3) + (t >> 3) / n_tiles : ((t >> 3) / n_tiles) * 8 + (t & 7);
  };
  auto decode = [&](int t) {
    Tile q;
    const int pb = pair_of(t);
    q.n0 = (((t >> 3) % n_tiles)) * BN;
    const int pix = pb % tiles_hw;
    q.b = pb / tiles_hw;
    q.y0 = (pix / tiles_w) * TH;
    q.x0 = (pix % tiles_w) * G::TW;
    return q;
  };
  auto resolve = [&](const TileQueue& tqq, int r) {
    for (;;) {
      const int t = tq_resolve(tqq, r);
      if (t < 0 || pair_of(t) < num_pb) return t;
      r = tq_claim_own(tqq);
    }
  };

  // ---- what a lane needs for the whole launch: fragment read addresses and DMA sources
  // (LDS pointers, not offsets: the image's base is added here once, not by a vector add in front of every read)
  cs2_lds_t aptr[9][2];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      aptr[tap][h] = lds + conv_s2_a_addr<G>(slw, li, kh, h, tap);
      asm volatile("" : "+v"(aptr[tap][h]));   // (one register each: left alone, the sums are re-made inside the run)
    }
  cs2_lds_t bptr[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    bptr[h] = lds + G::W_BASE + conv_s2_b_addr(0, li, kh, h, 0);
    asm volatile("" : "+v"(bptr[h]));
  }
  ConvS2Lane pl[G::PPW];
#pragma unroll
  for (int k = 0; k < G::PPW; ++k) pl[k] = conv_s2_patch_lane<G>(conv_s2_patch_piece<G>(slw, k), lane, W, CIN);
  int woff[G::WPW];
#pragma unroll
  for (int k = 0; k < G::WPW; ++k)
    woff[k] = k < 9 ? conv_s2_w_lane(4 * k + slw, lane, COUT, CIN) : conv_s2_wsc_lane(4 * k + slw, lane, CIN);
  const int last_delta = 1024 * (conv_s2_patch_piece<G>(slw, G::PPW - 1) - slw);
  int poff[G::PPW];      // patch sources of the tile being staged
  auto tile_offsets = [&](const Tile& q) {
    const int sy = 2 * q.y0 - 1, sx = 2 * q.x0 - 1, sbase = conv_s2_tile_base(q.y0, q.x0, W, CIN);
#pragma unroll
    for (int k = 0; k < G::PPW; ++k) poff[k] = conv_s2_patch_off(pl[k], sy, sx, sbase, H, W);
  };
  // a descriptor without records drops every lane: what a workgroup's LAST run stages (nothing follows it)
  auto x_srd = [&](const Tile& q, bool live) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X + (long)q.b * H * W * CIN), 0,
                                             live ? H * W * CIN * 4 : 0, 0x00020000);
  };
  auto w_srd = [&](const Tile& q, bool live) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wg + (long)q.n0 * CIN), 0,
                                             live ? (9 * COUT - q.n0) * CIN * 4 : 0, 0x00020000);
  };
  auto sc_srd = [&](const Tile& q, bool live) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(SC ? Wsc + (long)q.n0 * CIN : Wg), 0,
                                             SC && live ? (COUT - q.n0) * CIN * 4 : 0, 0x00020000);
  };
  auto stage_to = [&](int to_buf, __amdgpu_buffer_rsrc_t xs, __amdgpu_buffer_rsrc_t ws, __amdgpu_buffer_rsrc_t scs,
                      int c0) {
    Cs2Stage st;
    st.xsrd = xs;
    st.wsrd = ws;
    st.scsrd = scs;
    st.soff = c0 * 4;
    st.pdst = lds0 + to_buf * G::PATCH_BYTES + 1024 * slw;
    st.wdst = lds0 + G::W_BASE + to_buf * G::W_BYTES + 1024 * slw;
    st.last_delta = __builtin_amdgcn_readfirstlane(last_delta);
    return st;
  };

  const TileQueue tq{counters, (int)(blockIdx.x & 7), ((num_pb + 7) >> 3) * n_tiles};
  if (tid == 0) mail[0] = resolve(tq, tq_claim_own(tq));
  __syncthreads();
  const int t0 = __builtin_amdgcn_readfirstlane(mail[0]);
  if (t0 < 0) {
    if (tid == 0) tq_done(tq, gridDim.x);
    return;
  }
  Tile cur = decode(t0), nxt = cur;
  __amdgpu_buffer_rsrc_t xcur = x_srd(cur, true), wcur = w_srd(cur, true), sccur = sc_srd(cur, true);
  tile_offsets(cur);
  {
    const Cs2Stage st = stage_to(0, xcur, wcur, sccur, 0);
#pragma unroll
    for (int n = 0; n < G::NPW; ++n) cs2_issue_n<G>(n, st, poff, woff);
  }
  // (the claim of the second tile, used in the first tile's last stage; the compiler waits for it right here, behind
  //  the staging above: only a workgroup's start pays that)
  int claim = 0;
  if (tid == 0) claim = tq_claim_own(tq);
  const int nst = CIN / CS2_CB;
  int buf = 0, tpar = 1, tn = -1;
  bool first_tile = true;

  for (;;) {
    // acc_sc (SC = 1): the shortcut's accumulators.  Its chain: 16-channel blocks ascending, in a block 8 k-steps, step
    // q = 4 h + c pairing channels q and 8 + q (the two lane halves of a 32x32x2 MFMA); from zero, shift_sc added in
    // the epilogue.  The nine-tap chain into acc is what it was.
    f32x16 acc[2], acc_sc[SC ? 2 : 1];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int j = 0; j < (SC ? 2 : 0); ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_sc[j][r] = 0.f;
    for (int s = 0; s < nst; ++s) {
      const bool last = s == nst - 1;
      if (s == 0 && !first_tile) {
        if constexpr (SC) asm volatile("s_waitcnt vmcnt(" CS2_STR(CS2_TAIL_WAIT_LIT_SC) ")" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(" CS2_STR(CS2_TAIL_WAIT_LIT) ")" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (last && tid == 0) mail[tpar] = resolve(tq, claim);
      cs2_barrier();
      // what this run stages -- the next 16 channels of this tile, or the first 16 of the next one -- is worked out
      // BEHIND the run's first fragment reads: their LDS latency hides the decoding of the next tile
      Cs2Stage st;
      auto setup = [&]() {
        __amdgpu_buffer_rsrc_t xs = xcur, ws = wcur, scs = sccur;
        if (last) {
          tn = __builtin_amdgcn_readfirstlane(mail[tpar]);
          if (tn >= 0) {
            nxt = decode(tn);
            tile_offsets(nxt);
          }
          xs = x_srd(nxt, tn >= 0);
          ws = w_srd(nxt, tn >= 0);
          scs = sc_srd(nxt, tn >= 0);
        }
        st = stage_to(buf ^ 1, xs, ws, scs, last ? 0 : (s + 1) * CS2_CB);
      };

      {
        // read r of a tap, in the order the MFMAs want them: A h0, B j0 h0, B j1 h0, A h1, B j0 h1, B j1 h1
        f32x4 fa[2][2], fb[2][2][2];   // [tap parity][h], [tap parity][j][h]
        auto rd = [&](const int tap, const int r, const int par) {
          const int h = r / 3, w = r % 3;
          if (w == 0) fa[par][h] = cs2_lds_read128(aptr[tap < 9 ? tap : 4][h]);
          else fb[par][w - 1][h] = cs2_lds_read128(bptr[h] + tap * 4096 + (w - 1) * 2048);
        };
#pragma unroll
        for (int r = 0; r < 6; ++r) rd(0, r, 0);
        __builtin_amdgcn_sched_barrier(0);
        setup();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tap = 0; tap < NT; ++tap) {
          const int par = tap & 1;
#pragma unroll
          for (int m = 0; m < 16; ++m) {
            const int h = m >> 3, c = (m >> 1) & 3, j = m & 1;
            const float av = fa[par][h][c], bv = fb[par][j][h][c];
            if (tap < 9) acc[j] = MFMA32(av, bv, acc[j]);
            else acc_sc[SC ? j : 0] = MFMA32(av, bv, acc_sc[SC ? j : 0]);
            __builtin_amdgcn_sched_barrier(0);
            if (tap + 1 < NT && (m & 1) == 0 && m < 12) {
              rd(tap + 1, m >> 1, par ^ 1);
              __builtin_amdgcn_sched_barrier(0);
            }
            const int slot = conv_s2_slot_of(tap, m);
            if (slot >= 0 && slot < G::NPW) {
              cs2_issue_n<G>(slot, st, poff, woff);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
      }
      // the other buffer is the next stage's: 20 pointers move (behind the run's last MFMA, nothing waits for them)
      {
        const int dp = buf ? -G::PATCH_BYTES : G::PATCH_BYTES, dw = buf ? -G::W_BYTES : G::W_BYTES;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            aptr[tap][h] += dp;
            asm volatile("" : "+v"(aptr[tap][h]));
          }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          bptr[h] += dw;
          asm volatile("" : "+v"(bptr[h]));
        }
      }
      buf ^= 1;
    }
    // the claim of the tile after the next: in front of the epilogue's stores (wave 0 waits for it at once, with
    // vmcnt(0) -- the staging issued in the run above included; see the header)
    if (tid == 0 && tn >= 0) claim = tq_claim_own(tq);
    first_tile = false;
    // ---- epilogue as k_conv3x3: lane holds channel n0 + 32 j + li of the pixels x = x0 + 32 xt + (r & 3) + 8 (r >> 2)
    // + 4 kh -- 32 lanes = one whole 128-byte line per store; branch-free buffer accesses, the residual loads of
    // N-tile 1 in front of the stores of N-tile 0
    {
      const __amdgpu_buffer_rsrc_t ysrd = __builtin_amdgcn_make_buffer_rsrc(
          Y + (long)cur.b * Ho * Wo * COUT, 0, Ho * Wo * COUT * 4, 0x00020000);
      const __amdgpu_buffer_rsrc_t rsrd = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(HAS_R ? R + (long)cur.b * Ho * Wo * COUT : Y), 0, Ho * Wo * COUT * 4, 0x00020000);
      const int y = cur.y0 + slw / TWT, xbase = cur.x0 + 32 * (slw % TWT) + 4 * kh;
      int off[2][16];
      float rv[2][16];
      auto goffs = [&](int j, int* o) {
        const int n = cur.n0 + 32 * j + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int x = xbase + (r & 3) + 8 * (r >> 2);
          o[r] = (y < Ho && x < Wo) ? ((y * Wo + x) * COUT + n) * 4 : OOB;
        }
      };
      auto gres = [&](const int* o, float* v) {
        if (HAS_R) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrd, o[r], 0, 0));
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = 0.f;
        }
      };
      // (both shift values in front of the first store: a load behind the stores of N-tile 0 is waited for with
      //  vmcnt(0), i.e. behind those stores)
      const float shv[2] = {shift[cur.n0 + li], shift[cur.n0 + 32 + li]};
      // the shortcut's output (SC = 1): Ysc = acc_sc + shift_sc at the offsets of Y, no ReLU, no residual -- 32 more
      // whole-line stores per lane, those of an N-tile behind Y's
      const __amdgpu_buffer_rsrc_t yscsrd = __builtin_amdgcn_make_buffer_rsrc(
          SC ? Ysc + (long)cur.b * Ho * Wo * COUT : Y, 0, SC ? Ho * Wo * COUT * 4 : 0, 0x00020000);
      float shsc[2] = {0.f, 0.f};
      if constexpr (SC) {
        shsc[0] = shift_sc[cur.n0 + li];
        shsc[1] = shift_sc[cur.n0 + 32 + li];
      }
      goffs(0, off[0]);
      gres(off[0], rv[0]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j + 1 < 2) {
          goffs(j + 1, off[(j + 1) & 1]);
          gres(off[(j + 1) & 1], rv[(j + 1) & 1]);
        }
        const float sh = shv[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[j][r] + sh + rv[j & 1][r];
          if (relu) v = fmaxf(v, 0.f);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), ysrd, off[j & 1][r], 0, 0);
        }
        if constexpr (SC) {
          const float ss = shsc[j];
#pragma unroll
          for (int r = 0; r < 16; ++r)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, acc_sc[j][r] + ss), yscsrd,
                                                  off[j & 1][r], 0, 0);
        }
      }
    }
    if (tn < 0) break;
    cur = nxt;
    xcur = x_srd(cur, true);
    wcur = w_srd(cur, true);
    sccur = sc_srd(cur, true);
    tpar ^= 1;
  }
  if (tid == 0) tq_done(tq, gridDim.x);
}

template <int TH, int TWT, bool HAS_R, int SC = 0>
static int launch_conv_s2_r(const float* X, int B, int H, int W, int CIN, const float* Wg, const float* shift,
                            const float* R, float* Y, int COUT, int relu, hipStream_t st, const float* Wsc = nullptr,
                            const float* shift_sc = nullptr, float* Ysc = nullptr) {
  using G = ConvS2Geom<TH, TWT, SC>;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int tiles_w = cdiv(Wo, G::TW), tiles_h = cdiv(Ho, TH);
  const size_t lds = (size_t)G::LDS_BYTES + 16;   // + the mailbox
  PA_PERSISTENT("pa_conv3x3", (k_conv3x3_s2<TH, TWT, HAS_R, SC>), 256, lds, 1);   // one workgroup per CU: LDS-bound
  const int tiles_hw = tiles_w * tiles_h, n_tiles = COUT / CS2_BN;
  const long total = (long)tiles_hw * n_tiles * B;
  const int grid = persistent_grid(total, resident);
  hipLaunchKernelGGL((k_conv3x3_s2<TH, TWT, HAS_R, SC>), dim3(grid), dim3(256), lds, st, X, H, W, CIN, Wg, shift, R, Y,
                     Ho, Wo, COUT, relu, tiles_w, tiles_hw, n_tiles, (int)total, xcd_ranges_wanted(true), counters, Wsc,
                     shift_sc, Ysc);
  return 0;
}

// stride-2 launcher of pa_conv3x3 (emb_resnet.hip): cin % 16 == 0, cout % 64 == 0
int launch_conv_s2(const float* X, int B, int H, int W, int CIN, const float* Wg, const float* shift, const float* R,
                   float* Y, int COUT, int relu, hipStream_t st) {
  const int Ho = (H - 1) / 2 + 1;
  if (Ho >= 16)
    return R != nullptr ? launch_conv_s2_r<4, 1, true>(X, B, H, W, CIN, Wg, shift, R, Y, COUT, relu, st)
                        : launch_conv_s2_r<4, 1, false>(X, B, H, W, CIN, Wg, shift, R, Y, COUT, relu, st);
  return R != nullptr ? launch_conv_s2_r<2, 2, true>(X, B, H, W, CIN, Wg, shift, R, Y, COUT, relu, st)
                      : launch_conv_s2_r<2, 2, false>(X, B, H, W, CIN, Wg, shift, R, Y, COUT, relu, st);
}

// launcher of pa_conv3x3_s2_sc (emb_resnet.hip): the <4, 1> geometry with the 1x1 stride-2 shortcut as a tenth tap;
// cin % 16 == 0, cout % 64 == 0, Ho >= 16 (the <2, 2> geometry has no LDS left for the tenth tap)
int launch_conv_s2_sc(const float* X, int B, int H, int W, int CIN, const float* Wg, const float* shift,
                      const float* Wsc, const float* shift_sc, float* Y, float* Ysc, int COUT, int relu,
                      hipStream_t st) {
  return launch_conv_s2_r<4, 1, false, 1>(X, B, H, W, CIN, Wg, shift, nullptr, Y, COUT, relu, st, Wsc, shift_sc, Ysc);
}

}  // namespace pa
