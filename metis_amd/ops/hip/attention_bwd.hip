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
//     current tile's compute. The same image feeds the plain B-fragment
//     reads (QK^T, dO V^T) and the ds_read_b64_tr_b16 B-fragments (dS K;
//     dS^T Q, P^T dO) — no transposed copy exists;
//   * dS / P^T redistribute through per-wave LDS (raw bf16 bits as
//     shorts), published by a wave-local compiler fence — DS ops of one
//     wave complete in order;
//   * D in {64, 80, 96, 128} template instantiations (register arrays
//     compile-time indexed).
//
//   dQ kernel:  P = exp(scale*QK^T - lse); dP = dO V^T;
//               dS = scale * P o (dP - delta); dQ += dS @ K
//   dKV kernel: P^T = exp(scale*K Q^T - lse[col]); dP^T = V dO^T;
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
constexpr int VROW = CTILE + VPAD;   // per-wave dS / P^T tile row length
// Waves/SIMD asked of __launch_bounds__ = blocks/CU the LDS is sized for (the
// eight-wave D=64 dKV block reaches 4 waves/SIMD, so two of it fit as well).
constexpr int RESIDENT = 2;
static_assert(RBLK == ATTN_SEQ_TILE, "check_attn_qkv pins S to this tile");

// dKV: kv rows per block, one 16-row block per wave
template <int D>
constexpr int dkv_rows() { return D == 64 ? 128 : 64; }

// LDS. dQ: K and V images, dS tiles [4 waves][2 row blocks][16][VROW];
// dKV: Q and dO images, dS^T tiles [NW][16][VROW] then P^T tiles likewise.
template <int D>
using DqLayout = TileLayout<D, CTILE, THREADS / 64 * 2, RESIDENT>;
template <int D>
using DkvLayout = TileLayout<D, CTILE, 2 * (dkv_rows<D>() / 16), RESIDENT>;
static_assert(DqLayout<64>::bytes == 36864 && DqLayout<80>::bytes == 40960
              && DqLayout<96>::bytes == 45056 && DqLayout<128>::bytes == 53248);
static_assert(DkvLayout<64>::bytes == 55296 && DkvLayout<80>::bytes == 40960
              && DkvLayout<96>::bytes == 45056 && DkvLayout<128>::bytes == 53248);

// ---------------------------------------------------------------- dQ ----
// PACKED (attn_tile.h BlockCoord) in both kernels: Q, K, V and dQ / dK, dV
// point at the q, k, v column blocks of qkv and dqkv [B, S, (H + 2 Hkv) * D];
// dO is [B, S, H * D]; LSE and Delta stay [B, H, S].
template <int D, bool PACKED>
__global__ __launch_bounds__(THREADS, RESIDENT) void attn_bwd_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Delta,
    bf16* __restrict__ dQ,
    int B, int H, int Hkv, int S, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
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
    short* Sw = reinterpret_cast<short*>(smem) + L::w_off + wave * 2 * L::w_tile;

    // per-row state and Q/dO fragments for both row blocks
    float lse_r[2][4], delta_r[2][4];
    bf16x8 q_frag[2][dchunks], do_frag[2][dchunks];
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int q0 = qb + rbid[rb] * 16;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            lse_r[rb][r] = LSE[row_base + q0 + k8 * 4 + r];
            delta_r[rb][r] = Delta[row_base + q0 + k8 * 4 + r];
        }
        #pragma unroll
        for (int c = 0; c < dchunks; ++c) {
            q_frag[rb][c] = frag8<D>(Q + q_base, q0 + col16, c * 32 + k8 * 8,
                                     pitch);
            do_frag[rb][c] = frag8<D>(dO + bc.o_base, q0 + col16,
                                      c * 32 + k8 * 8, bc.o_pitch);
        }
    }

    floatx4 dq_acc[2][djtiles] = {};

    // T14 staged K (one natural image serves the QK^T reads and the tr16
    // reads of dS K); V has no stage registers and is loaded when its
    // natural image is written. Lanes walk kv rows for both; in PACKED
    // mode, where a row is its own 2*D-byte run, whole rows (dKV likewise).
    constexpr Walk WALK = PACKED ? Walk::WholeRows : Walk::RowsInDChunk;
    TileStage<CTILE, D, THREADS, WALK, WALK, /*STAGE_B=*/false,
              /*LANE_OFFS=*/PACKED> stage;
    const bf16* Kh = K + bc.kv_base;
    const bf16* Vh = V + bc.kv_base;

    const int kv_end = qb + RBLK;
    stage.issue_loads(Kh, Vh, 0, pitch, pitch);
    for (int kv0 = 0; kv0 < kv_end; kv0 += CTILE) {
        stage.write_stage(Ks, Vs, Vh, kv0, pitch);
        if (kv0 + CTILE < kv_end)
            stage.issue_loads(Kh, Vh, kv0 + CTILE, pitch, pitch);
        __syncthreads();

        bool rb_active[2];
        #pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int q0 = qb + rbid[rb] * 16;
            rb_active[rb] = kv0 <= q0 + 15;
            if (!rb_active[rb]) continue;

            __builtin_amdgcn_s_setprio(1);
            floatx4 s_acc[4], dp_acc[4];
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                s_acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
                dp_acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
                const int kvrow = j * 16 + col16;
                #pragma unroll
                for (int c = 0; c < dchunks; ++c) {
                    const int d0 = c * 32 + k8 * 8;
                    bf16x8 kf, vf;
                    lds_frag2<D, KSLOT>(Ks, Vs, kvrow, d0, kf, vf);
                    s_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        q_frag[rb][c], kf, s_acc[j], 0, 0, 0);
                    dp_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        do_frag[rb][c], vf, dp_acc[j], 0, 0, 0);
                }
            }
            __builtin_amdgcn_s_setprio(0);

            short* Srb = Sw + rb * 16 * VROW;
            #pragma unroll
            for (int j = 0; j < 4; ++j)
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qrow = q0 + k8 * 4 + r;
                    const int kvcol = kv0 + j * 16 + col16;
                    float p = (kvcol > qrow)
                                  ? 0.f
                                  : __expf(s_acc[j][r] * scale - lse_r[rb][r]);
                    float ds = scale * p * (dp_acc[j][r] - delta_r[rb][r]);
                    Srb[(k8 * 4 + r) * VROW + j * 16 + col16] =
                        float_to_bf16_bits(ds);
                }
        }

        // wave-local publish of dS (DS ops of one wave are in order)
        asm volatile("" ::: "memory");

        #pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            if (!rb_active[rb]) continue;
            const short* Srb = Sw + rb * 16 * VROW;
            #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 ds_frag = *reinterpret_cast<const bf16x8*>(
                    Srb + col16 * VROW + ks * 32 + k8 * 8);
                #pragma unroll
                for (int jd = 0; jd < djtiles; ++jd) {
                    bf16x8 kt_frag = tr16_frag<KSLOT>(
                        Ks, ks * 32 + k8 * 8, jd * 16, col16);
                    dq_acc[rb][jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        ds_frag, kt_frag, dq_acc[rb][jd], 0, 0, 0);
                }
            }
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
__global__ __launch_bounds__(dkv_rows<D>() / 16 * 64, RESIDENT)
void attn_bwd_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Delta,
    bf16* __restrict__ dK,   // [B, H, S, D] per q-head (wrapper reduces GQA)
    bf16* __restrict__ dV,
    int B, int H, int Hkv, int S, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
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
    short* Sw = reinterpret_cast<short*>(smem) + L::w_off + wave * L::w_tile;
    short* Pw = reinterpret_cast<short*>(smem) + L::w_off + (NW + wave) * L::w_tile;

    // K and V fragments for this wave's rows (A layout, m = col16)
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
        stage.write_stage(Qs, dOs, dOh, q0, bc.o_pitch);
        if (q0 + CTILE < S)
            stage.issue_loads(Qh, dOh, q0 + CTILE, pitch, bc.o_pitch);
        __syncthreads();

        const bool active = q0 + CTILE - 1 >= kv0;
        if (active) {
            __builtin_amdgcn_s_setprio(1);
            floatx4 st_acc[4], dpt_acc[4];
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                st_acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
                dpt_acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
                const int qrow = j * 16 + col16;
                #pragma unroll
                for (int c = 0; c < dchunks; ++c) {
                    const int d0 = c * 32 + k8 * 8;
                    bf16x8 qf, dof;
                    lds_frag2<D, KSLOT>(Qs, dOs, qrow, d0, qf, dof);
                    st_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        k_frag[c], qf, st_acc[j], 0, 0, 0);
                    dpt_acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        v_frag[c], dof, dpt_acc[j], 0, 0, 0);
                }
            }
            __builtin_amdgcn_s_setprio(0);

            #pragma unroll
            for (int j = 0; j < 4; ++j)
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kvrow = kv0 + k8 * 4 + r;
                    const int qcol = q0 + j * 16 + col16;
                    float p = (qcol < kvrow)
                                  ? 0.f
                                  : __expf(st_acc[j][r] * scale
                                           - LSE[row_base + qcol]);
                    float ds = scale * p
                               * (dpt_acc[j][r] - Delta[row_base + qcol]);
                    Sw[(k8 * 4 + r) * VROW + j * 16 + col16] =
                        float_to_bf16_bits(ds);
                    Pw[(k8 * 4 + r) * VROW + j * 16 + col16] =
                        float_to_bf16_bits(p);
                }

            asm volatile("" ::: "memory");   // wave-local publish

            #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 dst_frag = *reinterpret_cast<const bf16x8*>(
                    Sw + col16 * VROW + ks * 32 + k8 * 8);
                bf16x8 pt_frag = *reinterpret_cast<const bf16x8*>(
                    Pw + col16 * VROW + ks * 32 + k8 * 8);
                #pragma unroll
                for (int jd = 0; jd < djtiles; ++jd) {
                    bf16x8 qt_frag = tr16_frag<KSLOT>(
                        Qs, ks * 32 + k8 * 8, jd * 16, col16);
                    dk_acc[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        dst_frag, qt_frag, dk_acc[jd], 0, 0, 0);
                    bf16x8 dot_frag = tr16_frag<KSLOT>(
                        dOs, ks * 32 + k8 * 8, jd * 16, col16);
                    dv_acc[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        pt_frag, dot_frag, dv_acc[jd], 0, 0, 0);
                }
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
