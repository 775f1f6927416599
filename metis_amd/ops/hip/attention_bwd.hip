// Flash attention backward for gfx950 (causal, GQA) — bf16 I/O, fp32
// accumulation, MFMA 16x16x32, LSE-based recompute.
//
// Structure (mirrors attention.hip's forward; pieces from attn_tile.h):
//   * split dQ / dKV kernels (deterministic, no atomics); GQA dK/dV come
//     back per q-head and the wrapper reduces the group;
//   * dQ: block = 4 waves over 128 q rows, each wave owning TWO 16-row
//     blocks paired (w, 7-w) so causal work balances across waves; dKV:
//     one 16-row kv block per wave, 4 waves (8 at D = 64);
//   * own-side fragments (Q, dO for dQ; K, V for dKV) are read once from
//     global into registers; opposing-side tiles are 64 rows, staged into
//     LDS as NATURAL padded images (K, V for dQ; Q, dO for dKV) with the
//     T14 split: the next tile's chunks load to registers under the
//     current tile's compute. The same image feeds the plain A-fragment
//     reads of the first products and the ds_read_b64_tr_b16 B-fragments
//     of the second (dS K; dS^T Q, P^T dO) — no transposed copy exists;
//   * P and dS never leave the registers: the first products are oriented
//     with the OPPOSING-side row in the accumulator registers and the
//     own-side row on the lane, so their accumulators are the A operand of
//     the second products as they stand (attn_tile.h AccFrag), the tr16
//     reads following the accumulator's k order;
//   * D in {64, 80, 96, 128} template instantiations (register arrays
//     compile-time indexed).
//
//   dQ kernel:  P^T = exp(scale*K Q^T - lse[col]); dP^T = V dO^T;
//               dS^T = scale * P^T o (dP^T - delta[col]); dQ += dS @ K
//   dKV kernel: P = exp(scale*Q K^T - lse[row]); dP = dO V^T;
//               dV += P^T @ dO; dK += dS^T @ Q

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"
#include "attn_tile.h"

namespace {

using namespace attn_tile;

constexpr int THREADS = 256;
constexpr int RBLK = 128;    // dQ: q rows per block (2 x 16 per wave)
constexpr int CTILE = 64;    // opposing-side tile rows
// Waves/SIMD asked of __launch_bounds__ = blocks/CU the LDS is sized for (the
// eight-wave D=64 dKV block reaches 4 waves/SIMD, so two of it fit as well).
constexpr int RESIDENT = 2;
static_assert(RBLK == ATTN_SEQ_TILE, "check_attn_qkv pins S to this tile");

// dKV: kv rows per block, one 16-row block per wave
template <int D>
constexpr int dkv_rows() { return D == 64 ? 128 : 64; }

// Waves/SIMD each kernel is compiled for (the register budget it may not
// exceed); the LDS leaves room for more blocks than that at every D.
template <int D>
constexpr int dq_waves() { return D == 64 ? 3 : 2; }
template <int D>
constexpr int dkv_waves() { return D == 64 ? 4 : D == 80 ? 3 : 2; }

// dQ: whether the two row blocks of a wave run through a tile together,
// each K and V fragment read from LDS once for both, or one after the other
// (the same arithmetic per row block either way, so the choice is invisible
// in the results). Together takes about 45 more VGPRs: scratch at D = 64
// and 128, and at D = 80 the packed kernel's third wave per SIMD, without
// which it measured 2 % slower; it wins only at D = 96 (BENCHMARKS.md).
template <int D>
constexpr bool dq_pair_rows() { return D == 96; }

// LDS. dQ: K and V images; dKV: Q and dO images. Nothing else.
template <int D>
using DqLayout = TileLayout<D, CTILE, 0, RESIDENT>;
template <int D>
using DkvLayout = TileLayout<D, CTILE, 0, RESIDENT>;
static_assert(DqLayout<64>::bytes == 18432 && DqLayout<80>::bytes == 22528
              && DqLayout<96>::bytes == 26624 && DqLayout<128>::bytes == 34816);

// ---------------------------------------------------------------- dQ ----
// PACKED (attn_tile.h BlockCoord) in both kernels: Q, K, V and dQ / dK, dV
// point at the q, k, v column blocks of qkv and dqkv [B, S, (H + 2 Hkv) * D];
// dO is [B, S, H * D]; LSE and Delta stay [B, H, S].
template <int D, bool PACKED>
__global__ __launch_bounds__(THREADS, dq_waves<D>()) void attn_bwd_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Delta,
    bf16* __restrict__ dQ,
    int B, int H, int Hkv, int S, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col16 = lane & 15;
    const int k8 = lane >> 4;

    using L = DqLayout<D>;
    constexpr int dchunks = Geom<D>::dchunks;
    constexpr int djtiles = Geom<D>::djtiles;
    constexpr int KSLOT = Geom<D>::KSLOT;

    const BlockCoord bc = block_coord<D, PACKED>(S / RBLK, H, Hkv, S);
    const long q_base = bc.q_base, row_base = bc.row_base;
    const int pitch = bc.qkv_pitch;

    const int rbid[2] = {wave, 7 - wave};
    const int qb = bc.tile * RBLK;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    short* Ks = reinterpret_cast<short*>(smem) + L::a_off;
    short* Vs = reinterpret_cast<short*>(smem) + L::b_off;

    // Q/dO fragments for both row blocks: the B operands of S^T = K Q^T and
    // dP^T = V dO^T, [k = d][n = q row on the lane]. The lane's q row is
    // q0 + col16 in every first-product accumulator, so it needs one
    // lse/delta pair per row block.
    float lse_c[2], delta_c[2];
    bf16x8 q_frag[2][dchunks], do_frag[2][dchunks];
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int q0 = qb + rbid[rb] * 16;
        lse_c[rb] = LSE[row_base + q0 + col16];
        delta_c[rb] = Delta[row_base + q0 + col16];
        #pragma unroll
        for (int c = 0; c < dchunks; ++c) {
            q_frag[rb][c] = frag8<D>(Q + q_base, q0 + col16, c * 32 + k8 * 8,
                                     pitch);
            do_frag[rb][c] = frag8<D>(dO + bc.o_base, q0 + col16,
                                      c * 32 + k8 * 8, bc.o_pitch);
        }
    }

    floatx4 dq_acc[2][djtiles] = {};

    // T14 staged K (one natural image serves the S^T reads and the tr16
    // reads of dS K); V has no stage registers and is loaded when its
    // natural image is written. Lanes walk kv rows for both; in PACKED
    // mode, where a row is its own 2*D-byte run, whole rows (dKV likewise).
    constexpr Walk WALK = PACKED ? Walk::WholeRows : Walk::RowsInDChunk;
    TileStage<CTILE, D, THREADS, WALK, WALK, /*STAGE_B=*/false,
              /*LANE_OFFS=*/PACKED> stage;
    const bf16* Kh = K + bc.kv_base;
    const bf16* Vh = V + bc.kv_base;

    // One KV tile for the row blocks rb >= RB0 (the later block is live in
    // every tile of the loop, the earlier one is not). Each K and V
    // fragment is read once and feeds both row blocks.
    auto tile_body = [&](auto rb_lo, auto rb_hi, int kv0) {
        constexpr int RB0 = decltype(rb_lo)::value, RB1 = decltype(rb_hi)::value;

        AccFrag ds_frag[2][CTILE / 32];   // dS^T tiles, [kv rows][q on the lane]
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int j = 0; j < CTILE / 16; ++j) {
            floatx4 st_acc[2] = {}, dpt_acc[2] = {};
            #pragma unroll
            for (int c = 0; c < dchunks; ++c) {
                bf16x8 kf, vf;
                lds_frag2<D, KSLOT>(Ks, Vs, j * 16 + col16, c * 32 + k8 * 8,
                                    kf, vf);
                #pragma unroll
                for (int rb = RB0; rb < RB1; ++rb) {
                    st_acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        kf, q_frag[rb][c], st_acc[rb], 0, 0, 0);
                    dpt_acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        vf, do_frag[rb][c], dpt_acc[rb], 0, 0, 0);
                }
            }
            #pragma unroll
            for (int rb = RB0; rb < RB1; ++rb) {
                const int qrow = qb + rbid[rb] * 16 + col16;
                floatx4 ds;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kvrow = kv0 + j * 16 + k8 * 4 + r;
                    const float p =
                        (kvrow > qrow)
                            ? 0.f
                            : __expf(st_acc[rb][r] * scale - lse_c[rb]);
                    ds[r] = scale * p * (dpt_acc[rb][r] - delta_c[rb]);
                }
                ds_frag[rb][j >> 1].set_half(j & 1, ds);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);

        // dQ += dS K: dS is the A operand from the registers, K the tr16
        // B-fragment in the accumulator's k order
        #pragma unroll
        for (int ks = 0; ks < CTILE / 32; ++ks) {
            #pragma unroll
            for (int jd = 0; jd < djtiles; ++jd) {
                const bf16x8 kt_frag = tr16_frag_acc<KSLOT>(
                    Ks, ks * 32, k8, jd * 16, col16);
                #pragma unroll
                for (int rb = RB0; rb < RB1; ++rb)
                    dq_acc[rb][jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        ds_frag[rb][ks].frag(), kt_frag, dq_acc[rb][jd], 0, 0, 0);
            }
        }
    };

    const int kv_end = qb + RBLK;
    stage.issue_loads(Kh, Vh, 0, pitch, pitch);
    for (int kv0 = 0; kv0 < kv_end; kv0 += CTILE) {
        stage.write_stage(Ks, Vs, Vh, kv0, pitch);
        if (kv0 + CTILE < kv_end)
            stage.issue_loads(Kh, Vh, kv0 + CTILE, pitch, pitch);
        __syncthreads();

        // a row block is live while the tile starts at or below its diagonal
        const bool early_live = kv0 <= qb + rbid[0] * 16 + 15;
        constexpr std::integral_constant<int, 0> i0;
        constexpr std::integral_constant<int, 1> i1;
        constexpr std::integral_constant<int, 2> i2;
        if constexpr (dq_pair_rows<D>()) {
            if (early_live) tile_body(i0, i2, kv0);
            else tile_body(i1, i2, kv0);
        } else {
            if (early_live) tile_body(i0, i1, kv0);
            tile_body(i1, i2, kv0);
        }
        __syncthreads();
    }

    #pragma unroll
    for (int rb = 0; rb < 2; ++rb)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long qrow = qb + rbid[rb] * 16 + k8 * 4 + r;
            #pragma unroll
            for (int jd = 0; jd < djtiles; ++jd)
                dQ[q_base + qrow * pitch + jd * 16 + col16] =
                    __float2bfloat16(dq_acc[rb][jd][r]);
        }
}

// --------------------------------------------------------------- dKV ----
// One 16-row kv block per wave. At D=64 the block is EIGHT waves (128
// kv rows): all waves share one staged Q/dO stream, halving the number
// of Q/dO sweeps over the sequence (the kernel is wait-bound - 57-64%
// SQ_WAIT_ANY in the r2 PMC run). Measured: +15% at D=64; at D=80 the
// same change was -8.5% and at D=128/S=4096 -9.5% (deeper per-wave
// VGPR footprints lose the second independent block's latency
// cover), so those stay 4-wave x 64 rows.
template <int D, bool PACKED>
__global__ __launch_bounds__(dkv_rows<D>() / 16 * 64, dkv_waves<D>())
void attn_bwd_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Delta,
    bf16* __restrict__ dK,   // [B, H, S, D] per q-head (wrapper reduces GQA)
    bf16* __restrict__ dV,
    int B, int H, int Hkv, int S, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col16 = lane & 15;
    const int k8 = lane >> 4;

    using L = DkvLayout<D>;
    constexpr int dchunks = Geom<D>::dchunks;
    constexpr int djtiles = Geom<D>::djtiles;
    constexpr int KSLOT = Geom<D>::KSLOT;
    constexpr int KVB = dkv_rows<D>();
    constexpr int NW = KVB / 16;             // waves per block

    const BlockCoord bc = block_coord<D, PACKED>(S / KVB, H, Hkv, S);
    const long kv_base = bc.kv_base, row_base = bc.row_base;
    const long out_base = bc.q_base;      // dK/dV come back per q-head
    const int pitch = bc.qkv_pitch;

    const int kv0 = bc.tile * KVB + wave * 16;   // this wave's kv rows

    // natural Q/dO images only: dK/dV B-fragments are tr16 reads off these
    extern __shared__ __attribute__((aligned(16))) char smem[];
    short* Qs = reinterpret_cast<short*>(smem) + L::a_off;
    short* dOs = reinterpret_cast<short*>(smem) + L::b_off;

    // K and V fragments for this wave's rows: the B operands of S = Q K^T
    // and dP = dO V^T, [k = d][n = kv row on the lane]
    bf16x8 k_frag[dchunks], v_frag[dchunks];
    #pragma unroll
    for (int c = 0; c < dchunks; ++c) {
        k_frag[c] = frag8<D>(K + kv_base, kv0 + col16, c * 32 + k8 * 8, pitch);
        v_frag[c] = frag8<D>(V + kv_base, kv0 + col16, c * 32 + k8 * 8, pitch);
    }

    floatx4 dk_acc[djtiles] = {}, dv_acc[djtiles] = {};

    // T14 staged Q and dO, all NW waves staging, lanes walking q rows. At
    // D=128 the dO set would spill past 256 VGPRs on top of the dK+dV
    // accumulators, so dO is loaded at write time there.
    constexpr bool STAGE_DO = (D <= 96);
    constexpr Walk WALK = PACKED ? Walk::WholeRows : Walk::RowsInDChunk;
    TileStage<CTILE, D, NW * 64, WALK, WALK, STAGE_DO,
              /*LANE_OFFS=*/PACKED> stage;
    const bf16* Qh = Q + bc.q_base;
    const bf16* dOh = dO + bc.o_base;

    const int q_start = bc.tile * KVB;   // causal: from the block's kv start
    stage.issue_loads(Qh, dOh, q_start, pitch, bc.o_pitch);
    for (int q0 = q_start; q0 < S; q0 += CTILE) {
        // The first-product accumulators hold q rows 16 j + 4 k8 + r in their
        // registers: one aligned float4 of LSE and of Delta per subtile j.
        // A tile runs as two 32-row halves, each the k range of one second
        // product. The first half's rows are loaded here, ahead of the LDS
        // write, the barrier and the MFMAs and behind the staged tile in the
        // load queue; the second half's under the first half's second products.
        const bool active = q0 + CTILE - 1 >= kv0;
        float4 lse4[2], delta4[2];
        auto load_rows = [&](int ks) {
            #pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const long q = row_base + q0 + ks * 32 + jj * 16 + k8 * 4;
                lse4[jj] = *reinterpret_cast<const float4*>(LSE + q);
                delta4[jj] = *reinterpret_cast<const float4*>(Delta + q);
            }
        };
        if (active) load_rows(0);

        stage.write_stage(Qs, dOs, dOh, q0, bc.o_pitch);
        if (q0 + CTILE < S)
            stage.issue_loads(Qh, dOh, q0 + CTILE, pitch, bc.o_pitch);
        __syncthreads();

        if (active) {
            #pragma unroll
            for (int ks = 0; ks < CTILE / 32; ++ks) {
                AccFrag p_frag, ds_frag;   // [32 q rows][kv on the lane]
                __builtin_amdgcn_s_setprio(1);
                #pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int j = ks * 2 + jj;
                    floatx4 s_acc = {}, dp_acc = {};
                    #pragma unroll
                    for (int c = 0; c < dchunks; ++c) {
                        bf16x8 qf, dof;
                        lds_frag2<D, KSLOT>(Qs, dOs, j * 16 + col16,
                                            c * 32 + k8 * 8, qf, dof);
                        s_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            qf, k_frag[c], s_acc, 0, 0, 0);
                        dp_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            dof, v_frag[c], dp_acc, 0, 0, 0);
                    }
                    const float lse_r[4] = {lse4[jj].x, lse4[jj].y, lse4[jj].z,
                                            lse4[jj].w};
                    const float delta_r[4] = {delta4[jj].x, delta4[jj].y,
                                              delta4[jj].z, delta4[jj].w};
                    floatx4 p, ds;
                    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int qrow = q0 + j * 16 + k8 * 4 + r;
                        const int kvrow = kv0 + col16;
                        p[r] = (qrow < kvrow)
                                   ? 0.f
                                   : __expf(s_acc[r] * scale - lse_r[r]);
                        ds[r] = scale * p[r] * (dp_acc[r] - delta_r[r]);
                    }
                    p_frag.set_half(jj, p);
                    ds_frag.set_half(jj, ds);
                }
                __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
                if (ks + 1 < CTILE / 32) load_rows(ks + 1);

                // dK += dS^T Q, dV += P^T dO: the tiles are the A operand
                // from the registers, Q and dO tr16 B-fragments in the
                // accumulator's k order
                const bf16x8 dst_frag = ds_frag.frag();
                const bf16x8 pt_frag = p_frag.frag();
                #pragma unroll
                for (int jd = 0; jd < djtiles; ++jd) {
                    bf16x8 qt_frag = tr16_frag_acc<KSLOT>(
                        Qs, ks * 32, k8, jd * 16, col16);
                    dk_acc[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        dst_frag, qt_frag, dk_acc[jd], 0, 0, 0);
                    bf16x8 dot_frag = tr16_frag_acc<KSLOT>(
                        dOs, ks * 32, k8, jd * 16, col16);
                    dv_acc[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        pt_frag, dot_frag, dv_acc[jd], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }

    #pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long kvrow = kv0 + k8 * 4 + r;
        #pragma unroll
        for (int jd = 0; jd < djtiles; ++jd) {
            dK[out_base + kvrow * pitch + jd * 16 + col16] =
                __float2bfloat16(dk_acc[jd][r]);
            dV[out_base + kvrow * pitch + jd * 16 + col16] =
                __float2bfloat16(dv_acc[jd][r]);
        }
    }
}

// delta[row] = sum_d dO[row, d] * O[row, d] in fp32: the softmax-backward
// row term both kernels above consume. 16 lanes per row, one bf16x8 chunk
// each (D/8 = 8/10/12/16 of them live), 4 rows per wave step, DELTA_U steps
// in flight per thread; o and dO are read once, 4 B per row written.
// PACKED: o and dO are [B, S, H * D], so the rows walked are in (b, s, h)
// order and row (b, s, h) is stored to the [B, H, S] index (b * H + h) * S + s.
constexpr int DELTA_THREADS = 256;
constexpr int DELTA_U = 4;

template <bool PACKED>
__global__ void __launch_bounds__(DELTA_THREADS) attn_bwd_delta_kernel(
    const bf16x8* __restrict__ o,
    const bf16x8* __restrict__ d_o,
    float* __restrict__ delta,
    long rows,
    int dv,                         // D / 8 chunks per row, <= 16
    int H, int S) {                 // read in packed mode only
    const int sub = threadIdx.x & 15;
    const bool live = sub < dv;
    const int ci = live ? sub : dv - 1;     // idle lanes re-read a valid chunk
    const long rows_per_block = DELTA_THREADS / 16 * DELTA_U;
    const long row0 = (long)blockIdx.x * rows_per_block + threadIdx.x / 16;

    bf16x8 a[DELTA_U], b[DELTA_U];
    #pragma unroll
    for (int u = 0; u < DELTA_U; ++u) {
        long row = row0 + u * (DELTA_THREADS / 16);
        if (row >= rows) row = rows - 1;    // clamped, not stored below
        a[u] = o[row * dv + ci];
        b[u] = d_o[row * dv + ci];
    }
    #pragma unroll
    for (int u = 0; u < DELTA_U; ++u) {
        float s = 0.f;
        #pragma unroll
        for (int k = 0; k < 8; ++k)
            s += bf16_bits_to_float(a[u][k]) * bf16_bits_to_float(b[u][k]);
        if (!live) s = 0.f;
        #pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE_SIZE);
        const long row = row0 + u * (DELTA_THREADS / 16);
        if (sub == 0 && row < rows) {
            if constexpr (PACKED) {
                // the launcher pins rows = B * S * H below 2^31
                const int bs = (int)row / H, h = (int)row % H;
                delta[((long)(bs / S) * H + h) * S + bs % S] = s;
            } else {
                delta[row] = s;
            }
        }
    }
}

}  // namespace

torch::Tensor attn_bwd_delta(torch::Tensor o, torch::Tensor d_o) {
    TORCH_CHECK(o.is_cuda() && o.dtype() == torch::kBFloat16
                && d_o.is_cuda() && d_o.dtype() == torch::kBFloat16,
                "o and d_o must be CUDA bf16");
    TORCH_CHECK(o.dim() == 4 && o.sizes() == d_o.sizes(),
                "o and d_o must both be [B, H, S, D]");
    TORCH_CHECK(o.is_contiguous() && d_o.is_contiguous(),
                "o and d_o must be contiguous");
    const long D = o.size(3);
    check_head_dim(D);
    const long rows = o.numel() / D;
    auto delta = torch::empty({o.size(0), o.size(1), o.size(2)},
                              o.options().dtype(torch::kFloat32));
    if (rows == 0) return delta;
    const long rows_per_block = DELTA_THREADS / 16 * DELTA_U;
    const long grid = (rows + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(attn_bwd_delta_kernel<false>, dim3((unsigned)grid),
        dim3(DELTA_THREADS), 0, c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(o.data_ptr()),
        reinterpret_cast<const bf16x8*>(d_o.data_ptr()),
        delta.data_ptr<float>(), rows, (int)(D / 8), 0, 0);
    HIP_CHECK_LAST();
    return delta;
}

torch::Tensor attn_bwd_delta_packed(torch::Tensor o, torch::Tensor d_o, long H) {
    check_attn_packed_operand(o, "o");
    TORCH_CHECK(H > 0 && o.size(2) % H == 0, "o width must be H * D");
    const long B = o.size(0), S = o.size(1), D = o.size(2) / H;
    check_head_dim(D);
    check_attn_packed_out(d_o, "d_o", o, B, S, H, D);
    TORCH_CHECK(B > 0 && S > 0 && B * H * S < (1L << 31),
                "o must be non-empty and B * H * S must fit an int");
    const long rows = B * S * H;
    auto delta = torch::empty({B, H, S}, o.options().dtype(torch::kFloat32));
    const long rows_per_block = DELTA_THREADS / 16 * DELTA_U;
    const long grid = (rows + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(attn_bwd_delta_kernel<true>, dim3((unsigned)grid),
        dim3(DELTA_THREADS), 0, c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(o.data_ptr()),
        reinterpret_cast<const bf16x8*>(d_o.data_ptr()),
        delta.data_ptr<float>(), rows, (int)(D / 8), (int)H, (int)S);
    HIP_CHECK_LAST();
    return delta;
}

std::vector<torch::Tensor> attn_bwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor d_o, torch::Tensor lse, torch::Tensor delta,
    double scale) {
    const AttnDims a = check_attn_qkv(q, k, v);
    TORCH_CHECK(d_o.is_cuda() && d_o.dtype() == torch::kBFloat16,
                "d_o must be CUDA bf16");
    TORCH_CHECK(lse.is_cuda() && lse.dtype() == torch::kFloat32
                && delta.is_cuda() && delta.dtype() == torch::kFloat32,
                "lse and delta must be CUDA fp32");
    for (const torch::Tensor* t : {&d_o, &lse, &delta})
        TORCH_CHECK(t->get_device() == q.get_device(),
                    "all attn_bwd arguments must be on the same device");
    TORCH_CHECK(d_o.sizes() == q.sizes(), "d_o must be [B, H, S, D] like q");
    TORCH_CHECK(lse.dim() == 3 && lse.size(0) == a.B && lse.size(1) == a.H
                && lse.size(2) == a.S, "lse must be [B, H, S]");
    TORCH_CHECK(delta.sizes() == lse.sizes(), "delta must be [B, H, S]");
    auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
    auto doc = d_o.contiguous();
    auto lsec = lse.contiguous(), dc = delta.contiguous();
    check_attn_rows_aligned(lsec, "lse");
    check_attn_rows_aligned(dc, "delta");

    auto dq = torch::empty_like(qc);
    auto dk = torch::empty({a.B, a.H, a.S, a.D}, q.options());
    auto dv = torch::empty({a.B, a.H, a.S, a.D}, q.options());

    auto stream = c10::hip::getCurrentHIPStream().stream();
    dispatch_head_dim(a.D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        const int grid_dq = (int)(a.B * a.H * (a.S / RBLK));
        hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, false>), dim3(grid_dq),
            dim3(THREADS), DqLayout<DD>::bytes, stream,
            bf16_ptr(qc), bf16_ptr(kc), bf16_ptr(vc), bf16_ptr(doc),
            lsec.data_ptr<float>(), dc.data_ptr<float>(), bf16_ptr(dq),
            (int)a.B, (int)a.H, (int)a.Hkv, (int)a.S, (float)scale);
        // one block per dkv_rows kv rows, one wave per 16 of them
        constexpr int KVB = dkv_rows<DD>();
        const int grid_dkv = (int)(a.B * a.H * (a.S / KVB));
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<DD, false>), dim3(grid_dkv),
            dim3(KVB / 16 * 64), DkvLayout<DD>::bytes, stream,
            bf16_ptr(qc), bf16_ptr(kc), bf16_ptr(vc), bf16_ptr(doc),
            lsec.data_ptr<float>(), dc.data_ptr<float>(),
            bf16_ptr(dk), bf16_ptr(dv),
            (int)a.B, (int)a.H, (int)a.Hkv, (int)a.S, (float)scale);
    });
    HIP_CHECK_LAST();
    return {dq, dk, dv};
}

// Packed mode: dQ, dK, dV go straight into the q, k, v column blocks of one
// dqkv [B, S, (H + 2 Hkv) * D], which is what the qkv GEMM's backward reads.
torch::Tensor attn_bwd_packed(
    torch::Tensor qkv, torch::Tensor d_o, torch::Tensor lse, torch::Tensor delta,
    long H, long Hkv, long D, double scale) {
    const AttnDims a = check_attn_packed_qkv(qkv, H, Hkv, D);
    check_attn_packed_out(d_o, "d_o", qkv, a.B, a.S, a.H, a.D);
    check_attn_rows(lse, "lse", qkv, a.B, a.H, a.S);
    check_attn_rows(delta, "delta", qkv, a.B, a.H, a.S);

    // every element is written: the dQ grid covers every (batch, head, 128
    // q rows) of the q block, the dKV grid every (batch, head, KVB kv rows)
    // of the k and v blocks (H == Hkv), each over all D columns
    auto dqkv = torch::empty_like(qkv);

    auto stream = c10::hip::getCurrentHIPStream().stream();
    const bf16* in = bf16_ptr(qkv);
    bf16* out = bf16_ptr(dqkv);
    const long k_off = a.H * a.D, v_off = (a.H + a.Hkv) * a.D;
    dispatch_head_dim(a.D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        const int grid_dq = (int)(a.B * a.H * (a.S / RBLK));
        hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, true>), dim3(grid_dq),
            dim3(THREADS), DqLayout<DD>::bytes, stream,
            in, in + k_off, in + v_off, bf16_ptr(d_o),
            lse.data_ptr<float>(), delta.data_ptr<float>(), out,
            (int)a.B, (int)a.H, (int)a.Hkv, (int)a.S, (float)scale);
        constexpr int KVB = dkv_rows<DD>();
        const int grid_dkv = (int)(a.B * a.H * (a.S / KVB));
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<DD, true>), dim3(grid_dkv),
            dim3(KVB / 16 * 64), DkvLayout<DD>::bytes, stream,
            in, in + k_off, in + v_off, bf16_ptr(d_o),
            lse.data_ptr<float>(), delta.data_ptr<float>(),
            out + k_off, out + v_off,
            (int)a.B, (int)a.H, (int)a.Hkv, (int)a.S, (float)scale);
    });
    HIP_CHECK_LAST();
    return dqkv;
}
