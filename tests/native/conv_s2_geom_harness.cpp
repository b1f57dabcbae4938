// Host harness for csrc/emb_conv_s2_geom.h (the integer geometry of k_conv3x3_s2, compiled unchanged).  For both
// instantiations and a set of images, tiles and stages it replays
//   (1) the LDS-DMA of a stage -- every piece, every lane: which global element, or a hardware zero, lands in which
//       16-byte LDS slot (the buffer bounds check is replayed as the hardware does it: offset + 16 > num_records);
//   (2) the ds_read_b128 fragment reads of every wave, lane, tap and half,
// and checks that every patch element and every weight of the stage is written by exactly one lane of exactly one
// piece, that every read returns the element its (tap, pixel, channel) names -- a zero where the pixel lies outside
// the image -- and never an unwritten slot, that halo / out-of-image / padding lanes carry exactly the out-of-bounds
// offset, that every read is conflict-free under the hardware's lane-group rule (ds_read_b128: four groups of 16
// lanes, {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32, bank = (byte / 4) mod 64), and that the piece
// counts are the constants the kernel's issue slots and waits are built from.  Exit code 0 = all good.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "emb_conv_s2_geom.h"
using namespace pa;

struct Cell {
  int kind;   // 0 = never written, 1 = zero fill, 2 = data
  long a;     // patch: linear pixel iy * W + ix; weights: tap * COUT + n
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

template <class G>
static int check_patch(int H, int W, int CIN, int y0, int x0, int c0) {
  const unsigned num_records = (unsigned)((long)H * W * CIN * 4);
  std::vector<Cell> lds((size_t)G::PPIECES * 64, Cell{0, 0, 0});
  std::set<long> named;   // (py, px, q) elements of the patch
  const int sy = 2 * y0 - 1, sx = 2 * x0 - 1, sbase = conv_s2_tile_base(y0, x0, W, CIN);
  for (int piece = 0; piece < G::PPIECES; ++piece)
    for (int lane = 0; lane < 64; ++lane) {
      const ConvS2Lane L = conv_s2_patch_lane<G>(piece, lane, W, CIN);
      const int off = conv_s2_patch_off(L, sy, sx, sbase, H, W);
      // what the lane is FOR: slot 64 piece + lane holds quad q of entry e
      const int sl = 64 * piece + lane, e = sl >> 2, q = (sl & 3) ^ conv_s2_swz(e);
      const int plane = e / G::PWH, col = e % G::PWH, py = plane >> 1, px = 2 * col + (plane & 1);
      const bool real = e < G::PENT && px < G::PW;
      const int iy = sy + py, ix = sx + px;
      const bool inside = real && iy >= 0 && iy < H && ix >= 0 && ix < W;
      if (real && !named.insert(((long)py * G::PW + px) * 4 + q).second) FAIL("patch element staged twice");
      Cell& c = lds[(size_t)sl];
      if (c.kind != 0) FAIL("LDS slot written twice");
      if (!inside) {
        if (off != CS2_OOB) FAIL("halo / out-of-image / padding lane without the out-of-bounds offset");
      }
      // the hardware's range check (the stage's channel offset is the scalar offset: not part of it)
      if ((unsigned long)(unsigned)off + 16 > num_records) {
        c = Cell{1, 0, 0};
      } else {
        const long fl = (long)((unsigned)off / 4) + c0;
        c = Cell{2, fl / CIN, (int)(fl % CIN)};
      }
      if (inside && (c.kind != 2 || c.a != (long)iy * W + ix || c.ch != c0 + 4 * q))
        FAIL("piece %d lane %d: wrong source", piece, lane);
      if (!inside && c.kind != 1) FAIL("piece %d lane %d: no zero", piece, lane);
    }
  if ((int)named.size() != G::PH * G::PW * 4) FAIL("patch elements missing: %zu of %d", named.size(), G::PH * G::PW * 4);
  // fragment reads of the four waves
  for (int mt = 0; mt < 4; ++mt)
    for (int tap = 0; tap < 9; ++tap)
      for (int h = 0; h < 2; ++h) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int li = lane & 31, kh = lane >> 5;
          const int ad = conv_s2_a_addr<G>(mt, li, kh, h, tap);
          addr[lane] = ad;
          if (ad < 0 || ad % 16 != 0 || ad / 16 >= (int)lds.size()) FAIL("A read outside the patch image");
          const Cell& c = lds[ad / 16];
          if (c.kind == 0) FAIL("A read of a slot the DMA never wrote (mt %d tap %d lane %d)", mt, tap, lane);
          const int oy = y0 + mt / G::TWT, ox = x0 + 32 * (mt % G::TWT) + li;
          const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
          const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
          if (inside ? (c.kind != 2 || c.a != (long)iy * W + ix || c.ch != c0 + 8 * kh + 4 * h) : c.kind != 1)
            FAIL("A read (tile %d,%d mt %d tap %d h %d lane %d): wrong element", y0, x0, mt, tap, h, lane);
        }
        if (!conflict_free(addr)) FAIL("A read with a bank conflict (mt %d tap %d h %d)", mt, tap, h);
      }
  return 0;
}

template <class G>
static int check_weights(int COUT, int CIN, int n0, int c0) {
  std::vector<Cell> lds((size_t)G::WPIECES * 64, Cell{0, 0, 0});
  std::set<long> named;
  const unsigned num_records = (unsigned)((9L * COUT - n0) * CIN * 4);
  for (int piece = 0; piece < G::WPIECES; ++piece)
    for (int lane = 0; lane < 64; ++lane) {
      const int off = conv_s2_w_lane(piece, lane, COUT, CIN);
      if (off < 0 || (unsigned long)off + 16 > num_records) FAIL("weight lane out of the slice");
      const long fl = (long)off / 4 + (long)n0 * CIN + c0;   // in the image [9][COUT][CIN]
      Cell& c = lds[(size_t)64 * piece + lane];
      if (c.kind != 0) FAIL("LDS slot written twice");
      c = Cell{2, fl / CIN, (int)(fl % CIN)};
      if (!named.insert(fl).second) FAIL("weight staged twice");
    }
  if ((int)named.size() != 9 * CS2_BN * 4) FAIL("weights missing");
  for (int j = 0; j < 2; ++j)
    for (int tap = 0; tap < 9; ++tap)
      for (int h = 0; h < 2; ++h) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int li = lane & 31, kh = lane >> 5;
          const int ad = conv_s2_b_addr(j, li, kh, h, tap);
          addr[lane] = ad;
          // the kernel reads base(li, kh, h) + tap * 4096 + j * 2048: the address must be exactly that
          if (ad != conv_s2_b_addr(0, li, kh, h, 0) + tap * 4096 + j * 2048) FAIL("B read is not base + immediate");
          if (ad % 16 != 0 || ad / 16 >= (int)lds.size()) FAIL("B read outside the weight image");
          const Cell& c = lds[ad / 16];
          if (c.kind != 2 || c.a != (long)tap * COUT + n0 + 32 * j + li || c.ch != c0 + 8 * kh + 4 * h)
            FAIL("B read (tap %d j %d h %d lane %d): wrong element", tap, j, h, lane);
        }
        if (!conflict_free(addr)) FAIL("B read with a bank conflict (tap %d j %d h %d)", tap, j, h);
      }
  return 0;
}

template <class G>
static int check_counts(int pieces, int ppw, int npw, int lds_bytes) {
  if (G::PPIECES != pieces || G::PPW != ppw || G::WPW != 9 || G::NPW != npw || G::LDS_BYTES != lds_bytes)
    FAIL("piece counts: %d %d %d %d %d", G::PPIECES, G::PPW, G::WPW, G::NPW, G::LDS_BYTES);
  if (G::TILE_STORES != 32) FAIL("the first-stage wait is vmcnt(32)");
  if (G::NPW > CS2_SLOTS) FAIL("more pieces than issue slots");
  // the waves' pieces: every piece of the stage, the same number per wave, repeats only of the last patch piece
  std::multiset<int> pp, wp;
  for (int w = 0; w < 4; ++w) {
    for (int k = 0; k < G::PPW; ++k) pp.insert(conv_s2_patch_piece<G>(w, k));
    for (int k = 0; k < G::WPW; ++k) wp.insert(4 * k + w);
  }
  for (int i = 0; i < G::PPIECES; ++i)
    if (pp.count(i) != (i == G::PPIECES - 1 ? (size_t)(4 * G::PPW - G::PPIECES + 1) : 1u)) FAIL("patch piece %d", i);
  for (int i = 0; i < G::WPIECES; ++i)
    if (wp.count(i) != 1) FAIL("weight piece %d", i);
  // issue slots: 0 .. 26 once each, in order, never behind two neighbouring MFMAs
  int next = 0, last_at = -10;
  for (int tap = 0; tap < 9; ++tap)
    for (int m = 0; m < 16; ++m) {
      const int s = conv_s2_slot_of(tap, m);
      if (s < 0) continue;
      if (s != next++ || 16 * tap + m - last_at < 2) FAIL("issue slots");
      last_at = 16 * tap + m;
    }
  if (next != CS2_SLOTS) FAIL("issue slots: %d", next);
  return 0;
}

template <class G>
static int check_geom() {
  // images: odd and even sizes, maps smaller than a tile, the ResNet34 maps; all tiles of the small ones, the
  // corner and edge tiles of the large ones
  const int shapes[][3] = {{7, 63, 16}, {8, 64, 16}, {9, 66, 48}, {3, 5, 16}, {1, 1, 32}, {80, 998, 32}, {40, 499, 64},
                           {20, 250, 128}, {19, 129, 32}};
  for (const auto& s : shapes) {
    const int H = s[0], W = s[1], CIN = s[2];
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int th = (Ho + G::TH - 1) / G::TH, tw = (Wo + G::TW - 1) / G::TW;
    for (int ty = 0; ty < th; ++ty) {
      if (th > 4 && ty > 1 && ty < th - 2) continue;
      for (int tx = 0; tx < tw; ++tx) {
        if (tw > 4 && tx > 1 && tx < tw - 2) continue;
        for (int c0 = 0; c0 < CIN; c0 += (CIN > 32 ? CIN - 16 : 16))
          if (check_patch<G>(H, W, CIN, ty * G::TH, tx * G::TW, c0))
            return printf("  (H %d W %d CIN %d tile %d,%d c0 %d)\n", H, W, CIN, ty, tx, c0), 1;
      }
    }
  }
  const int wshapes[][2] = {{64, 16}, {128, 48}, {64, 32}, {256, 128}};
  for (const auto& s : wshapes)
    for (int n0 = 0; n0 < s[0]; n0 += 64)
      for (int c0 = 0; c0 < s[1]; c0 += 16)
        if (check_weights<G>(s[0], s[1], n0, c0)) return printf("  (COUT %d CIN %d n0 %d c0 %d)\n", s[0], s[1], n0, c0), 1;
  return 0;
}

int main() {
  if (check_counts<ConvS2Geom<4, 1>>(38, 10, 19, 151552)) return 1;
  if (check_counts<ConvS2Geom<2, 2>>(41, 11, 20, 157696)) return 1;
  if (check_geom<ConvS2Geom<4, 1>>()) return 1;
  if (check_geom<ConvS2Geom<2, 2>>()) return 1;
  printf("conv_s2 geometry: ok\n");
  return 0;
}
