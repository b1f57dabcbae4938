// Host harness for the shortcut form of csrc/emb_conv_s2_geom.h, ConvS2Geom<4, 1, 1> (compiled unchanged): the weight
// slab of k_conv3x3_s2<4, 1, false, 1> has a tenth 4-KB tap, the block entry's 1x1 stride-2 shortcut, whose DMA lanes
// read the plain [COUT][CIN] image through a descriptor of their own and whose A fragments are those of tap 4.  As
// tests/native/conv_s2_geom_harness.cpp does for the nine-tap slab, it replays
//   (1) the LDS-DMA of all 40 weight pieces of a stage, every lane: which element of which image lands in which
//       16-byte slot (the buffer bounds check as the hardware does it: offset + 16 > num_records, per descriptor);
//   (2) the ds_read_b128 B-fragment reads of all ten taps, both N-tiles and both halves, and the A-fragment reads the
//       tenth tap uses (tap 4's) on a replayed patch,
// and checks that every weight of both images is written exactly once, that every B read is base + (tap, N-tile)
// immediate with the immediate inside 16 bits, returns the element its (tap, channel) names -- for tap 9 the
// shortcut's Wsc[n0 + 32 j + li][c0 + 8 kh + 4 h ..] -- and is conflict-free under the hardware's lane-group rule, that
// tap 4's A read is input pixel (2 y, 2 x) of the output pixel, the one the 1x1 stride-2 convolution reads, that the
// piece counts are 38 / 10 / 20 / 159744, and that ConvS2Geom<4, 1, 0> is ConvS2Geom<4, 1>.  Exit code 0 = all good.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "emb_conv_s2_geom.h"
using namespace pa;

struct Cell {
  int kind;   // 0 = never written, 1 = zero fill, 2 = data of the 3x3 image, 3 = data of the shortcut image
  long a;     // patch: linear pixel iy * W + ix; 3x3 image: tap * COUT + n; shortcut image: n
  int ch;     // first channel of the quad
};

static const int GROUPS[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// one ds_read_b128 of a wave: 64 byte addresses -> conflict-free?
static bool conflict_free(const int (&addr)[64]) {
  for (int g = 0; g < 4; ++g) {
    std::set<int> banks;
    for (int i = 0; i < 16; ++i)
      for (int d = 0; d < 4; ++d) banks.insert((addr[GROUPS[g][i]] / 4 + d) % 64);
    if (banks.size() != 64) return false;
  }
  return true;
}

#define FAIL(...) return printf(__VA_ARGS__), printf("\n"), 1

using G = ConvS2Geom<4, 1, 1>;
using G0 = ConvS2Geom<4, 1>;

static int check_weights(int COUT, int CIN, int n0, int c0) {
  std::vector<Cell> lds((size_t)G::WPIECES * 64, Cell{0, 0, 0});
  std::set<long> named, named_sc;
  // the kernel's two descriptors: the slice of [9][COUT][CIN] from output channel n0 on, and of [COUT][CIN]
  const unsigned rec_w = (unsigned)((9L * COUT - n0) * CIN * 4), rec_sc = (unsigned)((long)(COUT - n0) * CIN * 4);
  for (int w = 0; w < 4; ++w)
    for (int k = 0; k < G::WPW; ++k) {
      const int piece = 4 * k + w;   // wave w's k-th weight piece; its last one (k = 9) is the shortcut's
      for (int lane = 0; lane < 64; ++lane) {
        const bool sc = k >= 9;
        const int off = sc ? conv_s2_wsc_lane(piece, lane, CIN) : conv_s2_w_lane(piece, lane, COUT, CIN);
        if (off < 0 || (unsigned long)off + 16 > (sc ? rec_sc : rec_w)) FAIL("weight lane out of its slice");
        const long fl = (long)off / 4 + (long)n0 * CIN + c0;   // in the lane's image
        Cell& c = lds[(size_t)64 * piece + lane];
        if (c.kind != 0) FAIL("LDS slot written twice");
        c = Cell{sc ? 3 : 2, fl / CIN, (int)(fl % CIN)};
        if (!(sc ? named_sc : named).insert(fl).second) FAIL("weight staged twice");
      }
    }
  if ((int)named.size() != 9 * CS2_BN * 4 || (int)named_sc.size() != CS2_BN * 4) FAIL("weights missing");
  for (const Cell& c : lds)
    if (c.kind == 0) FAIL("a slot of the slab is never written");
  for (int j = 0; j < 2; ++j)
    for (int tap = 0; tap < G::WTAPS; ++tap)
      for (int h = 0; h < 2; ++h) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int li = lane & 31, kh = lane >> 5;
          const int ad = conv_s2_b_addr(j, li, kh, h, tap);
          addr[lane] = ad;
          // the kernel reads base(li, kh, h) + tap * 4096 + j * 2048, the second term a ds_read immediate
          if (ad != conv_s2_b_addr(0, li, kh, h, 0) + tap * 4096 + j * 2048) FAIL("B read is not base + immediate");
          if (tap * 4096 + j * 2048 >= 65536) FAIL("B read immediate does not fit 16 bits");
          if (ad % 16 != 0 || ad / 16 >= (int)lds.size()) FAIL("B read outside the weight image");
          const Cell& c = lds[ad / 16];
          const int n = n0 + 32 * j + li, ch = c0 + 8 * kh + 4 * h;
          if (tap < 9 ? (c.kind != 2 || c.a != (long)tap * COUT + n || c.ch != ch) : (c.kind != 3 || c.a != n || c.ch != ch))
            FAIL("B read (tap %d j %d h %d lane %d): wrong element", tap, j, h, lane);
        }
        if (!conflict_free(addr)) FAIL("B read with a bank conflict (tap %d j %d h %d)", tap, j, h);
      }
  return 0;
}

// the patch DMA of a stage and the A reads of the tenth tap: tap 4's, which must be pixel (2 oy, 2 ox)
static int check_centre_tap(int H, int W, int CIN, int y0, int x0, int c0) {
  const unsigned num_records = (unsigned)((long)H * W * CIN * 4);
  std::vector<Cell> lds((size_t)G::PPIECES * 64, Cell{0, 0, 0});
  const int sy = 2 * y0 - 1, sx = 2 * x0 - 1, sbase = conv_s2_tile_base(y0, x0, W, CIN);
  for (int piece = 0; piece < G::PPIECES; ++piece)
    for (int lane = 0; lane < 64; ++lane) {
      const ConvS2Lane L = conv_s2_patch_lane<G>(piece, lane, W, CIN);
      const int off = conv_s2_patch_off(L, sy, sx, sbase, H, W);
      const ConvS2Lane L0 = conv_s2_patch_lane<G0>(piece, lane, W, CIN);
      if (L.rel != L0.rel || L.py != L0.py || L.px != L0.px) FAIL("the patch of <4, 1, 1> is not that of <4, 1>");
      Cell& c = lds[(size_t)64 * piece + lane];
      if ((unsigned long)(unsigned)off + 16 > num_records) {
        c = Cell{1, 0, 0};
      } else {
        const long fl = (long)((unsigned)off / 4) + c0;
        c = Cell{2, fl / CIN, (int)(fl % CIN)};
      }
    }
  for (int mt = 0; mt < 4; ++mt)
    for (int h = 0; h < 2; ++h) {
      int addr[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int li = lane & 31, kh = lane >> 5;
        const int ad = conv_s2_a_addr<G>(mt, li, kh, h, 4);
        addr[lane] = ad;
        if (ad != conv_s2_a_addr<G0>(mt, li, kh, h, 4)) FAIL("A read of <4, 1, 1> is not that of <4, 1>");
        if (ad < 0 || ad % 16 != 0 || ad / 16 >= (int)lds.size()) FAIL("A read outside the patch image");
        const Cell& c = lds[ad / 16];
        const int oy = y0 + mt / G::TWT, ox = x0 + 32 * (mt % G::TWT) + li;
        const int iy = 2 * oy, ix = 2 * ox;   // what conv1x1_s2 reads for output pixel (oy, ox)
        const bool inside = iy < H && ix < W;
        if (inside ? (c.kind != 2 || c.a != (long)iy * W + ix || c.ch != c0 + 8 * kh + 4 * h) : c.kind != 1)
          FAIL("tap 4 is not pixel (2y, 2x) (tile %d,%d mt %d h %d lane %d)", y0, x0, mt, h, lane);
      }
      if (!conflict_free(addr)) FAIL("A read with a bank conflict (mt %d h %d)", mt, h);
    }
  return 0;
}

static int check_counts() {
  static_assert(std::is_same<ConvS2Geom<4, 1, 0>, ConvS2Geom<4, 1>>::value, "SC = 0 is the default");
  using Z = ConvS2Geom<4, 1, 0>;
  if (Z::PPIECES != 38 || Z::PPW != 10 || Z::WPIECES != 36 || Z::WPW != 9 || Z::NPW != 19 || Z::LDS_BYTES != 151552 ||
      Z::TILE_STORES != 32 || Z::W_BASE != G0::W_BASE || Z::W_BYTES != 36 * 1024 || Z::WTAPS != 9)
    FAIL("<4, 1, 0> is not <4, 1>");
  if (G::PPIECES != 38 || G::PPW != 10 || G::NPW != 20 || G::LDS_BYTES != 159744)
    FAIL("piece counts: %d %d %d %d", G::PPIECES, G::PPW, G::NPW, G::LDS_BYTES);
  if (G::WPIECES != 40 || G::WPW != 10 || G::WTAPS != 10 || G::W_BYTES != 40 * 1024) FAIL("weight pieces");
  if (G::TILE_STORES != 64) FAIL("stores per lane and tile: both outputs");
  if (G::LDS_BYTES + 64 > 160 * 1024) FAIL("two stages and the mailbox do not fit LDS");
  if (G::PATCH_BYTES != G0::PATCH_BYTES || G::W_BASE != G0::W_BASE) FAIL("the patch images moved");
  if (G::NPW > CS2_SLOTS) FAIL("more pieces than issue slots");
  // every weight piece once, the same number per wave; the four shortcut pieces are the waves' last ones
  std::multiset<int> wp;
  for (int w = 0; w < 4; ++w)
    for (int k = 0; k < G::WPW; ++k) wp.insert(4 * k + w);
  for (int i = 0; i < G::WPIECES; ++i)
    if (wp.count(i) != 1) FAIL("weight piece %d", i);
  for (int w = 0; w < 4; ++w)
    if ((4 * (G::WPW - 1) + w) * 16 / CS2_BN != 9) FAIL("a wave's last weight piece is not in tap 9");
  // the tenth tap has MFMAs but no issue slot of its own: all pieces go behind the first nine taps
  for (int m = 0; m < 16; ++m) {
    const int s = conv_s2_slot_of(9, m);
    if (s >= 0 && s < G::NPW) FAIL("a piece would be issued from the tenth tap");
  }
  return 0;
}

int main() {
  if (check_counts()) return 1;
  const int wshapes[][2] = {{64, 16}, {128, 48}, {64, 32}, {128, 64}, {256, 128}};
  for (const auto& s : wshapes)
    for (int n0 = 0; n0 < s[0]; n0 += 64)
      for (int c0 = 0; c0 < s[1]; c0 += 16)
        if (check_weights(s[0], s[1], n0, c0)) return printf("  (COUT %d CIN %d n0 %d c0 %d)\n", s[0], s[1], n0, c0), 1;
  // Ho >= 16 only: odd and even sizes, the ResNet34 maps of layers 2 and 3; corner and edge tiles of the large ones
  const int shapes[][3] = {{31, 63, 16}, {32, 64, 16}, {33, 66, 48}, {37, 61, 16}, {80, 998, 32}, {40, 499, 64}};
  for (const auto& s : shapes) {
    const int H = s[0], W = s[1], CIN = s[2];
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int th = (Ho + G::TH - 1) / G::TH, tw = (Wo + G::TW - 1) / G::TW;
    for (int ty = 0; ty < th; ++ty) {
      if (th > 4 && ty > 1 && ty < th - 2) continue;
      for (int tx = 0; tx < tw; ++tx) {
        if (tw > 4 && tx > 1 && tx < tw - 2) continue;
        for (int c0 = 0; c0 < CIN; c0 += (CIN > 32 ? CIN - 16 : 16))
          if (check_centre_tap(H, W, CIN, ty * G::TH, tx * G::TW, c0))
            return printf("  (H %d W %d CIN %d tile %d,%d c0 %d)\n", H, W, CIN, ty, tx, c0), 1;
      }
    }
  }
  printf("conv_s2 shortcut geometry: ok\n");
  return 0;
}
