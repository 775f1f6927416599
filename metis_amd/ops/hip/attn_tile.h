// Tile toolkit shared by the MFMA attention kernels (attention.hip forward,
// attention_bwd.hip dQ and dKV): per-D geometry, the dynamic-LDS layout,
// fragment reads, the block-coordinate decode and the register-staged
// (T14) tile copy. A new attention kernel starts from these pieces
// (docs/KERNELS.md). All __forceinline__ / constexpr: no scratch.
#pragma once

#include "common.h"

namespace attn_tile {

typedef short short4v __attribute__((ext_vector_type(4)));

constexpr int VPAD = 8;                 // per-wave P / dS tile row padding (bf16)
constexpr int LDS_PER_CU = 160 * 1024;

// Per-D geometry. LDS tiles are NATURAL [row][D] images of raw bf16 bits
// (shorts), each row padded by one 16-B slot so the power-of-2 row stride
// does not land every row on the same banks.
template <int D>
struct Geom {
    static constexpr int dchunks = (D + 31) / 32;   // 32-wide MFMA K chunks of D
    static constexpr int djtiles = D / 16;          // 16-wide output column tiles
    static constexpr int KSLOT = D / 8 + 1;         // 16-B slots per LDS row
    static constexpr int tile(int rows) { return rows * KSLOT * 8; }   // shorts
};

// Dynamic-LDS layout all three kernels instantiate, offsets in shorts: two
// natural [ROWS][D] images (A, B) and WTILES per-wave [16][ROWS + VPAD]
// tiles (P, dS, P^T). The kernel carves its pointers from the offsets and
// its launcher requests `bytes`, so the two cannot disagree.
template <int D, int ROWS, int WTILES, int RESIDENT>
struct TileLayout {
    static constexpr int WROW = ROWS + VPAD;
    static constexpr int a_off = 0;
    static constexpr int b_off = Geom<D>::tile(ROWS);
    static constexpr int w_off = 2 * Geom<D>::tile(ROWS);
    static constexpr int w_tile = 16 * WROW;
    static constexpr int bytes = (w_off + WTILES * w_tile) * 2;
    // b128 accesses need 16-B alignment; a tr16 read off it returns wrong data
    static_assert(b_off % 8 == 0 && w_off % 8 == 0 && w_tile % 8 == 0);
    static_assert(bytes * RESIDENT <= LDS_PER_CU, "resident blocks must fit one CU");
};

// A/B fragment (8 bf16 of row `row` at column d0) straight from global,
// rows `pitch` elements apart; zero where a 32-wide chunk runs past D
// (D = 80).
template <int D>
__device__ __forceinline__ bf16x8 frag8(const bf16* base, long row, int d0,
                                        int pitch) {
    if (d0 < D)
        return *reinterpret_cast<const bf16x8*>(base + row * pitch + d0);
    return bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// The same fragment from a natural [row][KSLOT*8] LDS image.
template <int D, int KSLOT>
__device__ __forceinline__ bf16x8 lds_frag(const short* img, int row, int d0) {
    if (d0 < D)
        return *reinterpret_cast<const bf16x8*>(img + row * KSLOT * 8 + d0);
    return bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// Two images read at the same (row, d0) under ONE tail guard: two separate
// lds_frag calls compile to two exec-masked regions at D = 80.
template <int D, int KSLOT>
__device__ __forceinline__ void lds_frag2(const short* img_a, const short* img_b,
                                          int row, int d0, bf16x8& a, bf16x8& b) {
    a = b = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (d0 < D) {
        a = *reinterpret_cast<const bf16x8*>(img_a + row * KSLOT * 8 + d0);
        b = *reinterpret_cast<const bf16x8*>(img_b + row * KSLOT * 8 + d0);
    }
}

// Fragment via ds_read_b64_tr_b16 from a NATURAL [row][KSLOT*8] LDS image:
// per 16-lane group, two reads cover two blocks of 4 opposing-index rows,
// starting at row_lo (elements 0..3) and row_hi (elements 4..7); lane l&15
// receives its d-column (semantics pinned by ext.tr16_probe). The caller
// passes each block's first row FOR ITS LANE GROUP; two row rules are in use.
template <int KSLOT>
__device__ __forceinline__ bf16x8 tr16_rows(
    const short* img, int row_lo, int row_hi, int col0, int p4) {
    bf16x8 out;
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = (r ? row_hi : row_lo) + (p4 >> 2);
        const int col = col0 + (p4 & 3) * 4;
        short4v t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) short4v*)(
                img + row * KSLOT * 8 + col));
        out[r * 4 + 0] = t[0];
        out[r * 4 + 1] = t[1];
        out[r * 4 + 2] = t[2];
        out[r * 4 + 3] = t[3];
    }
    return out;
}

// Natural k order: element i of lane group g is row row0 + i of the image,
// row0 = chunk + 8g. The B operand [k][n = d] against an A operand read
// in natural order (lds_frag / frag8).
template <int KSLOT>
__device__ __forceinline__ bf16x8 tr16_frag(
    const short* img, int row0, int col0, int p4) {
    return tr16_rows<KSLOT>(img, row0, row0 + 4, col0, p4);
}

// Accumulator k order: the other operand of the product is acc_frag() of
// the two 16-row accumulator tiles that start at rows `chunk` and
// `chunk + 16`, so element i of lane group g is row chunk + 16 (i >> 2) +
// 4g + (i & 3). B operand [k][n = d] or, the read being symmetric, the A
// operand [m = d][k] of the transposed product.
template <int KSLOT>
__device__ __forceinline__ bf16x8 tr16_frag_acc(
    const short* img, int chunk, int g, int col0, int p4) {
    return tr16_rows<KSLOT>(img, chunk + 4 * g, chunk + 16 + 4 * g, col0, p4);
}

// Two fp32 values to packed bf16 bits, round-to-nearest-even
// (v_cvt_pk_bf16_f32), `lo` in the low half.
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    typedef float floatx2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(
        unsigned, __builtin_convertvector(floatx2{lo, hi}, bf16x2v));
}

// An MFMA accumulator tile as the next MFMA's operand, no LDS and no lane
// movement. Lane (c = l & 15, g = l >> 4) holds X[4g + r][c] of a 16x16
// accumulator tile X. Two tiles (the rows `chunk ..` and `chunk + 16 ..` of
// one 32-row strip) give the 8-element fragment of a product that sums over
// X's ROW index: elements 0..3 from x_lo, 4..7 from x_hi. As the B operand
// that is X, as the A operand X^T. The k order inside the 32-row strip is
// the permuted one of tr16_frag_acc, which the other operand must follow.
// A half is one tile's four values; a kernel that finishes its tiles one at
// a time fills the halves as they come.
struct AccFrag {
    unsigned w[4];
    __device__ __forceinline__ void set_half(int hi, floatx4 x) {
        w[2 * hi + 0] = pack_bf16x2(x[0], x[1]);
        w[2 * hi + 1] = pack_bf16x2(x[2], x[3]);
    }
    __device__ __forceinline__ bf16x8 frag() const {
        typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
        return __builtin_bit_cast(bf16x8, uintx4{w[0], w[1], w[2], w[3]});
    }
};

// blockIdx.x = (batch * H + head) * tiles + tile: the tile index, the
// offsets of row 0 of that q head and of its GQA kv head, and the distance
// between consecutive rows of one head (wave-uniform: SGPRs).
//
// Two addressing modes. Unpacked: q/o/dO/dQ are [B, H, S, D] and k/v
// [B, Hkv, S, D], every pitch is the constant D. PACKED (H == Hkv only):
// q, k, v (and dq, dk, dv) are the three column blocks of ONE
// [B, S, (H + 2 Hkv) * D] buffer, the k and v pointers already advanced to
// their block's first column by the launcher, so one base serves all three;
// o and dO are [B, S, H * D]. LSE / delta rows are [B, H, S] in both.
struct BlockCoord {
    int tile;
    long q_base, kv_base;   // row 0 of the head in q|dq and in k|v|dk|dv
    long o_base;            // row 0 of the head in o|dO
    long row_base;          // row offset into [B, H, S]
    int qkv_pitch;          // elements between rows of q, k, v, dq, dk, dv
    int o_pitch;            // elements between rows of o, dO
};

template <int D, bool PACKED>
__device__ __forceinline__ BlockCoord block_coord(int tiles, int H, int Hkv, int S) {
    const int head = (blockIdx.x / tiles) % H;
    const int batch = blockIdx.x / tiles / H;
    BlockCoord c;
    c.tile = blockIdx.x % tiles;
    c.row_base = ((long)batch * H + head) * S;
    if constexpr (PACKED) {
        const int HT = H + 2 * Hkv;
        c.qkv_pitch = HT * D;
        c.o_pitch = H * D;
        c.q_base = c.kv_base = ((long)batch * S * HT + head) * D;
        c.o_base = ((long)batch * S * H + head) * D;
    } else {
        const int kv_head = head / (H / Hkv);
        c.qkv_pitch = c.o_pitch = D;
        c.q_base = c.o_base = c.row_base * D;
        c.kv_base = (((long)batch * Hkv + kv_head) * S) * D;
    }
    return c;
}

// How the NT threads of a block walk the 16-B chunks of a [ROWS][D] tile.
// The first two number the chunks c = thread + u * NT and lay consecutive c
// along a row first, or down the rows of one d-chunk. WholeRows gives each
// pass u the next NT / (D/8) whole rows, thread t taking chunk t % (D/8) of
// row t / (D/8) (threads past the last whole row idle): the same lanes-along-
// a-row order as DChunksInRow, but a thread's chunks are a constant number of
// rows apart whatever D/8 is, so one lane offset serves every pass.
enum class Walk { DChunksInRow, RowsInDChunk, WholeRows };

template <int ROWS, int D, Walk W>
__device__ __forceinline__ void chunk_pos(int c, int& row, int& d0) {
    if constexpr (W == Walk::DChunksInRow) {
        row = c / (D / 8);
        d0 = c % (D / 8) * 8;
    } else {
        row = c % ROWS;
        d0 = c / ROWS * 8;
    }
}

// T14 register-staged copy of two [ROWS][D] global tiles (A, B) into
// natural LDS images by NT threads: issue_loads() one tile AHEAD (HBM
// latency hides under the current tile's compute), write_stage() at loop
// top. With STAGE_B false B has no registers and is loaded at write time.
// LANE_OFFS splits each address into a wave-uniform 64-bit base (the first
// row of the tile, or of the pass) and a loop-invariant unsigned 32-bit lane
// offset in bytes, the form the load takes an SGPR base for; (row * pitch +
// d0) * 2 < 2^32 because the packed launchers pin the pitch below 2^24.
template <int ROWS, int D, int NT, Walk WA, Walk WB, bool STAGE_B = true,
          bool LANE_OFFS = false>
struct TileStage {
    static_assert((WA == Walk::WholeRows) == (WB == Walk::WholeRows));
    static constexpr bool whole_rows = WA == Walk::WholeRows;
    static constexpr int chunks = ROWS * D / 8;     // 16-B chunks per tile
    static constexpr int pass_rows = NT / (D / 8);  // WholeRows: rows per pass
    static constexpr int per_thread =
        whole_rows ? (ROWS + pass_rows - 1) / pass_rows : (chunks + NT - 1) / NT;

    bf16x8 a[per_thread];
    bf16x8 b[STAGE_B ? per_thread : 1];

    // Position of this thread's chunk of pass u: row = urow (wave-uniform) +
    // lrow, column d0; false once the thread has no chunk left.
    template <Walk W>
    static __device__ __forceinline__ bool pos(int u, int& urow, int& lrow, int& d0) {
        if constexpr (W == Walk::WholeRows) {
            urow = u * pass_rows;
            lrow = threadIdx.x / (D / 8);
            d0 = threadIdx.x % (D / 8) * 8;
            return lrow < pass_rows && urow + lrow < ROWS;
        } else {
            const int c = threadIdx.x + u * NT;
            urow = 0;
            chunk_pos<ROWS, D, W>(c, lrow, d0);
            return c < chunks;
        }
    }

    template <Walk W>
    static __device__ __forceinline__ bf16x8 load(const bf16* src, int row0, int u,
                                                  int pitch) {
        int urow, lrow, d0;
        pos<W>(u, urow, lrow, d0);
        if constexpr (LANE_OFFS) {
            const unsigned lane_off = (unsigned)(lrow * pitch + d0) * 2u;
            return *reinterpret_cast<const bf16x8*>(
                reinterpret_cast<const char*>(src + (long)(row0 + urow) * pitch)
                + lane_off);
        }
        return *reinterpret_cast<const bf16x8*>(
            src + (long)(row0 + urow + lrow) * pitch + d0);
    }
    template <Walk W>
    static __device__ __forceinline__ void store(short* img, int u, bf16x8 val) {
        int urow, lrow, d0;
        pos<W>(u, urow, lrow, d0);
        *reinterpret_cast<bf16x8*>(img + Geom<D>::tile(urow + lrow) + d0) = val;
    }

    // A and B point at row 0 of this head, their rows pitch_a and pitch_b
    // elements apart; row0 is the tile's first row
    __device__ __forceinline__ void issue_loads(
        const bf16* A, const bf16* B, int row0, int pitch_a, int pitch_b) {
        #pragma unroll
        for (int u = 0; u < per_thread; ++u) {
            int urow, lrow, d0;
            if (!pos<WA>(u, urow, lrow, d0)) break;
            a[u] = load<WA>(A, row0, u, pitch_a);
            if constexpr (STAGE_B) b[u] = load<WB>(B, row0, u, pitch_b);
        }
    }
    __device__ __forceinline__ void write_stage(
        short* As, short* Bs, const bf16* B, int row0, int pitch_b) {
        #pragma unroll
        for (int u = 0; u < per_thread; ++u) {
            int urow, lrow, d0;
            if (!pos<WA>(u, urow, lrow, d0)) break;
            store<WA>(As, u, a[u]);
            bf16x8 bv;
            if constexpr (STAGE_B) bv = b[u];
            else bv = load<WB>(B, row0, u, pitch_b);
            store<WB>(Bs, u, bv);
        }
    }
};

}  // namespace attn_tile
