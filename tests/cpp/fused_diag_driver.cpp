// Walks the DIAG4 index maps of csrc/mo_fused_diag.h lane by lane on the CPU (tests/test_fused_diag_cpu.py):
//   the LDS-DMA lays a random 4 x n group of J into a ring slot, the block instructions' operand reads and 4x4x4 products are carried
//   out with the lane layout tools/microbench.hip measured (A(i,k) at lane i + 4 blk + 16 k, B(k,j) at j + 4 blk + 16 k, D(i,j) at
//   j + 4 blk + 16 i), the accumulators go through the staging area into the 16x16x4 C/D layout, and the four diagonal tiles are compared
//   with J^T J (same fma order over the rows, both triangles, exact).  Bank checks: 64 banks of 4 bytes; ds_read_b128 is served in the
//   four 16-lane groups below, ds_read_b64 in two groups of 32.
// usage: fused_diag_driver n [n ...]   -> one line of key=value pairs per n, then the coverage line
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "mo_fused_diag.h"

using namespace mo::diag4;

static const int kB128Groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                       {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// no two lanes of a group touch the same bank (width bytes per lane at addr[lane])
static bool conflict_free(const int* addr, const int* lanes, int nlanes, int width) {
  std::set<int> banks;
  for (int x = 0; x < nlanes; ++x)
    for (int b = 0; b < width; b += 4)
      if (!banks.insert(((addr[lanes[x]] + b) / 4) % 64).second) return false;
  return true;
}

static double rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5 + ((s >> 24) & 0xff) / 16777216.0; }

int main(int argc, char** argv) {
  constexpr int N = 64, NH = 2, NT = 4;
  int all_lanes[64];
  for (int l = 0; l < 64; ++l) all_lanes[l] = l;
  for (int arg = 1; arg < argc; ++arg) {
    const int nn = atoi(argv[arg]);
    unsigned seed = 1234u + nn;
    std::vector<double> J(4 * N, 0.0);   // row g, variable v (zero beyond nn: the padded system)
    for (int g = 0; g < 4; ++g) for (int v = 0; v < nn; ++v) J[g * N + v] = rnd(seed);
    // the DMA: lane (g, j) fetches piece swz(g, j) of band h (variables 32h + 2 piece, +1) into byte h * 1024 + lane * 16; pieces beyond the row are never written
    std::vector<unsigned char> slot(NH * 1024, 0);
    for (int h = 0; h < NH; ++h)
      for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, piece = swz(g, lane & 15), v = 32 * h + 2 * piece;
        if (v < nn) memcpy(&slot[h * 1024 + lane * 16], &J[g * N + v], 16);
      }
    // the lane's own 16 bytes: piece j of its row
    bool natural_ok = true, natural_free = true, operand_free = true;
    int addr[64];
    for (int h = 0; h < NH; ++h) {
      for (int lane = 0; lane < 64; ++lane) {
        addr[lane] = h * 1024 + natural_off(lane);
        double v[2];
        memcpy(v, &slot[addr[lane]], 16);
        const int g = lane >> 4, j = lane & 15;
        natural_ok = natural_ok && v[0] == J[g * N + 32 * h + 2 * j] && v[1] == J[g * N + 32 * h + 2 * j + 1];
      }
      for (int q = 0; q < 4; ++q) natural_free = natural_free && conflict_free(addr, kB128Groups[q], 16, 16);
    }
    // operand reads and block products
    double acc[NH][kNumIns][64];
    for (int h = 0; h < NH; ++h) {
      double vec[kNumVec][64];
      for (int v = 0; v < kNumVec; ++v) {
        for (int lane = 0; lane < 64; ++lane) {
          addr[lane] = h * 1024 + operand_off(v, lane);
          memcpy(&vec[v][lane], &slot[addr[lane]], 8);
        }
        operand_free = operand_free && conflict_free(addr, all_lanes, 32, 8) && conflict_free(addr, all_lanes + 32, 32, 8);
      }
      for (int ins = 0; ins < kNumIns; ++ins)
        for (int lane = 0; lane < 64; ++lane) {   // D(i, j) of block blk at lane j + 4 blk + 16 i
          const int i = lane >> 4, blk = (lane >> 2) & 3, j = lane & 3;
          double s = 0.0;
          for (int k = 0; k < 4; ++k) s = fma(vec[kInsA[ins]][i + 4 * blk + 16 * k], vec[kInsB[ins]][j + 4 * blk + 16 * k], s);
          acc[h][ins][lane] = s;
        }
    }
    // accumulators -> staged tiles (lower sub-block and its mirror image) -> C/D layout
    std::vector<double> stage(kStageBytes / 8, NAN);
    for (int h = 0; h < NH; ++h)
      for (int ins = 0; ins < kNumIns; ++ins)
        for (int lane = 0; lane < 64; ++lane) {
          const int c = 2 * h + acc_tile(lane), r = acc_row(ins, lane), cc = acc_col(ins, lane);
          stage[stage_off(c, r, cc) / 8] = acc[h][ins][lane];
          if (!ins_diagonal(ins)) stage[stage_off(c, cc, r) / 8] = acc[h][ins][lane];
        }
    bool tiles_exact = true;
    for (int c = 0; c < NT; ++c)
      for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 4; ++t) {
          const int g = lane >> 4, j = lane & 15, r = g + 4 * t;
          const double got = stage[stage_off(c, r, j) / 8];   // register t of lane (g, j): as the kernel reads it back
          const int vr = 32 * (c >> 1) + 2 * r + (c & 1), vc = 32 * (c >> 1) + 2 * j + (c & 1);   // tile c, position p = variable 32 (c >> 1) + 2 p + (c & 1)
          double want = 0.0;
          for (int k = 0; k < 4; ++k) want = fma(J[k * N + vr], J[k * N + vc], want);
          tiles_exact = tiles_exact && got == want;   // NaN (an element nobody staged) fails too
        }
    printf("n=%d natural_ok=%d natural_conflict_free=%d operand_conflict_free=%d tiles_exact=%d\n", nn, natural_ok, natural_free, operand_free, tiles_exact);
  }
  // the ten lower sub-block pairs of a tile, each exactly once over the five instructions and two slots
  std::multiset<std::pair<int, int>> seen;
  for (int ins = 0; ins < kNumIns; ++ins) for (int u = 0; u < 2; ++u) seen.insert({ins_p(ins, u), ins_q(ins, u)});
  bool once = seen.size() == 10;
  for (int p = 0; p < 4; ++p) for (int q = 0; q <= p; ++q) once = once && seen.count({p, q}) == 1;
  printf("pairs_once=%d\n", once);
  return 0;
}
