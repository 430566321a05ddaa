// mo_fused_diag.h -- index maps of the DIAG4 J stream: the diagonal J^T J tiles of the 64 grid on v_mfma_f64_4x4x4_4b_f64 (four
// independent 4x4x4 products per instruction), lower sub-blocks only.  constexpr and host-compilable: the kernel (JStream<..., DIAG4> in
// kkt_fused.hip) takes every address from the functions below -- swz, natural_off, operand_off, acc_tile / acc_row / acc_col, stage_off --
// and tests/cpp/fused_diag_driver.cpp walks the same functions lane by lane on the CPU.  Tables are read through selects on compile-time
// indices (vec_sub), so that device code never indexes them with a lane value.
//
// Hardware layout of the instruction (tools/microbench.hip, measured on gfx950; one double of A, B and D per lane):
//   A(i, k) of block blk at lane i + 4 blk + 16 k,  B(k, j) at lane j + 4 blk + 16 k,  D(i, j) at lane j + 4 blk + 16 i.
// A 16-lane row of the wave is therefore one row k of the 4-row group -- the row g the lane fetches for the 16x16x4 stream anyway --
// and the blocks are the four quads of a row.
//
// Ring slot (per tile pair h = 0, 1: 1 KiB): row g of the group at g * 256, sixteen 16-byte pieces; piece p holds position p of tile 2h
// (low 8 bytes) and of tile 2h + 1 (high 8 bytes).  The LDS-DMA's destination is lane-linear, its source is per lane: lane (g, j) fetches
// piece j ^ 4 X[g], so piece p of row g sits at POSITION p ^ 4 X[g] of the row.  Sub-block s of a tile = positions 4s .. 4s + 3 = quad s.
// A block instruction reads, per half wave (rows 2a, 2a + 1), quads {s0, s1} of one row and {s0, s1} ^ X[2a] ^ X[2a + 1] of the other:
// X[0] ^ X[1] = X[2] ^ X[3] = 3 maps every pair the table uses onto its complement, so the 32 lanes hit 32 different 8-byte words.
#pragma once

namespace mo {
namespace diag4 {

constexpr int kX[4] = {0, 3, 1, 2};                                   // quad swizzle of row g
constexpr int kXPacked = 0x9C;                                        // kX as four 2-bit fields: a lane looks its row's entry up by a shift
constexpr int x_of(int g) { return (kXPacked >> (2 * g)) & 3; }
static_assert(x_of(0) == kX[0] && x_of(1) == kX[1] && x_of(2) == kX[2] && x_of(3) == kX[3], "kXPacked encodes kX");
static_assert((kX[0] ^ kX[1]) == 3 && (kX[2] ^ kX[3]) == 3, "the two rows of a half wave read complementary quad pairs");
constexpr int swz(int g, int piece) { return piece ^ (4 * x_of(g)); }   // position of piece `piece` in row g (and the piece a lane (g, j) fetches)

// lane -> coordinates inside the block instruction
constexpr int lane_k(int lane) { return lane >> 4; }        // row of the 4-row group (A, B); row i of the result block (D)
constexpr int lane_blk(int lane) { return (lane >> 2) & 3; }
constexpr int lane_i(int lane) { return lane & 3; }         // i of A, j of B and D
constexpr int blk_u(int blk) { return blk >> 1; }           // which of the two sub-block slots of an operand vector
constexpr int blk_e(int blk) { return blk & 1; }            // tile 2h + e of the pair

// operand vectors: sub-block in slot u = 0 | u = 1
constexpr int kNumVec = 5, kNumIns = 5;
constexpr int kVec[kNumVec][2] = {{0, 1}, {2, 3}, {3, 2}, {1, 3}, {0, 2}};   // Va .. Ve
// instructions: D += A B with A = vector kInsA, B = vector kInsB; slot u yields sub-block (p, q) = (kVec[A][u], kVec[B][u]), p >= q
constexpr int kInsA[kNumIns] = {0, 1, 1, 2, 3};
constexpr int kInsB[kNumIns] = {0, 1, 0, 0, 4};
constexpr int vec_sub(int vec, int u) { return u ? kVec[vec][1] : kVec[vec][0]; }
constexpr int ins_p(int ins, int u) { return vec_sub(kInsA[ins], u); }
constexpr int ins_q(int ins, int u) { return vec_sub(kInsB[ins], u); }

// byte offsets inside the 1 KiB of a tile pair
constexpr int natural_off(int lane) { return lane_k(lane) * 256 + swz(lane_k(lane), lane & 15) * 16; }   // the lane's own 16-byte piece (lane & 15)
constexpr int operand_off(int vec, int lane) {
  return lane_k(lane) * 256 + swz(lane_k(lane), 4 * vec_sub(vec, blk_u(lane_blk(lane))) + lane_i(lane)) * 16 + 8 * blk_e(lane_blk(lane));
}

// accumulator (ins, lane) -> element (row, col) of tile 2h + acc_tile: the lower sub-block (p, q); its mirror is (col, row)
constexpr int acc_tile(int lane) { return blk_e(lane_blk(lane)); }
constexpr int acc_row(int ins, int lane) { return 4 * ins_p(ins, blk_u(lane_blk(lane))) + lane_k(lane); }
constexpr int acc_col(int ins, int lane) { return 4 * ins_q(ins, blk_u(lane_blk(lane))) + lane_i(lane); }
constexpr bool ins_diagonal(int ins) { return kInsA[ins] == kInsB[ins]; }   // sub-blocks (p, p): both triangles come out of the product

// staging of the finished tiles (8 KiB of the drained ring): tile c row-major, read back in the 16x16x4 C/D layout
// (lane (g, j), register t = element (g + 4t, j): 512 consecutive bytes per register)
constexpr int stage_off(int tile, int row, int col) { return tile * 2048 + (row * 16 + col) * 8; }
constexpr int kStageBytes = 4 * 2048;

}  // namespace diag4
}  // namespace mo
