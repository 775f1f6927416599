// Flash attention forward (causal, GQA) for gfx950 — bf16 I/O, fp32
// online softmax, MFMA (v_mfma_f32_16x16x32_bf16) for QK^T and PV.
//
// Structure (pieces from attn_tile.h):
//   * block = 256 threads = 4 waves covering 128 q rows; each wave owns
//     TWO 16-row blocks paired as (w, 7-w) so causal work is balanced
//     across waves (early rows pair with late rows);
//   * KV tiles 128 rows wide for D <= 80, 64 above; K and V are both
//     staged into LDS as NATURAL [kv][D] images with one 16-B slot of row
//     padding, register-staged one tile ahead (T14);
//   * the products are transposed so that P never leaves the registers:
//     S^T = K Q^T puts the kv row in the accumulator registers and the q
//     row on the lane, and that accumulator is the B operand of
//     O^T += V^T P^T as it stands (attn_tile.h AccFrag). K A-fragments are
//     plain reads of the K image, V^T A-fragments come from
//     ds_read_b64_tr_b16 (hardware transpose) off the V image in the
//     accumulator's k order; each K and V fragment is read once and feeds
//     both row blocks of the wave;
//   * online softmax with ONE (m, l) pair per lane and row block: the row
//     max and sum run over the lane's own registers plus two cross-group
//     steps (lanes +-16, +-32);
//   * D in {64, 80, 96, 128} as template instantiations so every
//     accumulator array is compile-time indexed (registers, not scratch).
//
// Saves the row LSE (m + log l) for the backward pass.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"
#include "attn_tile.h"

namespace {

using namespace attn_tile;

constexpr int THREADS = 256;
constexpr int QBLK = 128;     // q rows per block (2 x 16 per wave)
constexpr int RESIDENT = 2;   // waves/SIMD asked of __launch_bounds__ = blocks/CU
static_assert(QBLK == ATTN_SEQ_TILE, "check_attn_qkv pins S to this tile");

// KV tile width: 128 for D <= 80, 64 above. Wider tiles amortize the two
// barriers per tile over twice the MFMA work.
template <int D>
constexpr int kvblk_for() { return D <= 80 ? 128 : 64; }

// Whether the two row blocks of a wave run through a tile together, each K
// and V fragment read from LDS once for both, or one after the other (the
// same arithmetic per row block either way, so the choice is invisible in
// the results). Together takes about 30 more VGPRs and measured 9-14 %
// faster (BENCHMARKS.md): chosen wherever it leaves no scratch, which it
// does not at D = 128 nor, with its extra address registers, in the
// unpacked D = 80 kernel (docs/KERNELS.md).
template <int D, bool PACKED>
constexpr bool pair_rows() { return D == 64 || D == 96 || (D == 80 && PACKED); }

// LDS: K and V images of KVBLK rows, nothing else
template <int D>
using FwdLayout = TileLayout<D, kvblk_for<D>(), 0, RESIDENT>;
static_assert(FwdLayout<64>::bytes == 36864 && FwdLayout<80>::bytes == 45056
              && FwdLayout<96>::bytes == 26624 && FwdLayout<128>::bytes == 34816);

// PACKED (attn_tile.h BlockCoord): Q, K, V point at the q, k, v column
// blocks of one qkv [B, S, (H + 2 Hkv) * D] and O is [B, S, H * D].
template <int D, bool PACKED>
__global__ __launch_bounds__(THREADS, RESIDENT) void attn_fwd_kernel(
    const bf16* __restrict__ Q,   // [B, H, S, D]
    const bf16* __restrict__ K,   // [B, Hkv, S, D]
    const bf16* __restrict__ V,   // [B, Hkv, S, D]
    bf16* __restrict__ O,         // [B, H, S, D]
    float* __restrict__ LSE,      // [B, H, S] in both modes
    int B, int H, int Hkv, int S,
    float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col16 = lane & 15;
    const int k8 = lane >> 4;

    using L = FwdLayout<D>;
    constexpr int KVBLK = kvblk_for<D>();    // kv rows per tile
    constexpr int JSUB = KVBLK / 16;         // 16-row S^T subtiles per tile
    constexpr int dchunks = Geom<D>::dchunks;
    constexpr int djtiles = Geom<D>::djtiles;
    constexpr int KSLOT = Geom<D>::KSLOT;

    const BlockCoord bc = block_coord<D, PACKED>(S / QBLK, H, Hkv, S);
    const long q_base = bc.q_base;
    const int pitch = bc.qkv_pitch;

    // this wave's two 16-row blocks: rb index within the 128-row block
    const int rbid[2] = {wave, 7 - wave};
    const int qb = bc.tile * QBLK;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // raw bf16 BITS as shorts (a short into __hip_bfloat16 converts
    // numerically — never store element-wise through the struct type).
    short* Ks = reinterpret_cast<short*>(smem) + L::a_off;
    short* Vs = reinterpret_cast<short*>(smem) + L::b_off;

    // ---- preload Q fragments for both row blocks: the B operand of
    // S^T = K Q^T, [k = d][n = q row on the lane] ---------------------------
    bf16x8 q_frag[2][dchunks];
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb)
        #pragma unroll
        for (int c = 0; c < dchunks; ++c)
            q_frag[rb][c] = frag8<D>(Q + q_base, qb + rbid[rb] * 16 + col16,
                                     c * 32 + k8 * 8, pitch);

    // the lane's q row is q0 + col16 in every accumulator below, so the
    // softmax state is one value per lane and row block (the four lane
    // groups hold copies)
    float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
    floatx4 o_acc[2][djtiles] = {};   // O^T: [d = 16 jd + 4 k8 + r][q]

    // T14 staging, 256 threads. K: lanes walk d-chunks within a row
    // (coalesced reads, conflict-free vector LDS writes at row stride
    // KSLOT*16 B). V: lanes walk kv rows; that walk served a transposed V
    // image that no longer exists; it stays, as changing it would change speed.
    // PACKED: a tile is KVBLK runs of 2*D bytes at the qkv pitch, not one
    // run, so both operands walk whole rows (Walk::WholeRows) off an SGPR
    // tile base; measured against the walks above in BENCHMARKS.md.
    constexpr Walk WK = PACKED ? Walk::WholeRows : Walk::DChunksInRow;
    constexpr Walk WV = PACKED ? Walk::WholeRows : Walk::RowsInDChunk;
    TileStage<KVBLK, D, THREADS, WK, WV, /*STAGE_B=*/true,
              /*LANE_OFFS=*/PACKED> stage;
    const bf16* Kh = K + bc.kv_base;
    const bf16* Vh = V + bc.kv_base;

    // One KV tile for the row blocks rb >= RB0. The later block (7 - wave)
    // is live in every tile of the loop; the earlier one drops out of the
    // last 64-row tile, which lies wholly above its diagonal.
    auto tile_body = [&](auto rb_lo, auto rb_hi, int kv0) {
        constexpr int RB0 = decltype(rb_lo)::value, RB1 = decltype(rb_hi)::value;

        // ---- S^T = scale * K Q^T, masked ----------------------------------
        float p[2][JSUB][4];   // [rb][j][r]: kv = kv0 + 16 j + 4 k8 + r
        __builtin_amdgcn_s_setprio(1);   // T5: favor the MFMA cluster
        #pragma unroll
        for (int j = 0; j < JSUB; ++j) {    // 16-row kv subtiles
            floatx4 s_acc[2] = {};
            #pragma unroll
            for (int c = 0; c < dchunks; ++c) {
                const bf16x8 k_frag =
                    lds_frag<D, KSLOT>(Ks, j * 16 + col16, c * 32 + k8 * 8);
                #pragma unroll
                for (int rb = RB0; rb < RB1; ++rb)
                    s_acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        k_frag, q_frag[rb][c], s_acc[rb], 0, 0, 0);
            }
            #pragma unroll
            for (int rb = RB0; rb < RB1; ++rb) {
                const int qrow = qb + rbid[rb] * 16 + col16;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kvrow = kv0 + j * 16 + k8 * 4 + r;
                    p[rb][j][r] = (kvrow > qrow) ? -1e30f : s_acc[rb][r] * scale;
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);

        // ---- online softmax, P^T to operand fragments ---------------------
        AccFrag p_frag[2][KVBLK / 32];
        #pragma unroll
        for (int rb = RB0; rb < RB1; ++rb) {
            float tile_max = -1e30f;
            #pragma unroll
            for (int j = 0; j < JSUB; ++j)
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    tile_max = fmaxf(tile_max, p[rb][j][r]);
            tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, WAVE_SIZE));
            tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, WAVE_SIZE));

            const float m_new = fmaxf(m_run[rb], tile_max);
            const float alpha = __expf(m_run[rb] - m_new);
            float row_sum = 0.f;
            #pragma unroll
            for (int j = 0; j < JSUB; ++j) {
                floatx4 e;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    e[r] = __expf(p[rb][j][r] - m_new);
                    row_sum += e[r];
                }
                p_frag[rb][j >> 1].set_half(j & 1, e);
            }
            row_sum += __shfl_xor(row_sum, 16, WAVE_SIZE);
            row_sum += __shfl_xor(row_sum, 32, WAVE_SIZE);

            l_run[rb] = l_run[rb] * alpha + row_sum;
            m_run[rb] = m_new;
            #pragma unroll
            for (int jd = 0; jd < djtiles; ++jd)
                o_acc[rb][jd] *= alpha;
        }

        __builtin_amdgcn_sched_barrier(0);
        // ---- O^T += V^T P^T: V^T A-fragments via hardware transpose read,
        // rows in the accumulator's k order ----------------------------------
        #pragma unroll
        for (int ks = 0; ks < KVBLK / 32; ++ks) {   // 32-row kv chunks
            #pragma unroll
            for (int jd = 0; jd < djtiles; ++jd) {
                const bf16x8 vt_frag = tr16_frag_acc<KSLOT>(
                    Vs, ks * 32, k8, jd * 16, col16);
                #pragma unroll
                for (int rb = RB0; rb < RB1; ++rb)
                    o_acc[rb][jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        vt_frag, p_frag[rb][ks].frag(), o_acc[rb][jd], 0, 0, 0);
            }
        }
    };

    const int kv_end = qb + QBLK;
    stage.issue_loads(Kh, Vh, 0, pitch, pitch);
    for (int kv0 = 0; kv0 < kv_end; kv0 += KVBLK) {
        stage.write_stage(Ks, Vs, Vh, kv0, pitch);
        if (kv0 + KVBLK < kv_end) stage.issue_loads(Kh, Vh, kv0 + KVBLK, pitch,
                                                      pitch);
        __syncthreads();

        // a row block is live while the tile starts at or below its diagonal
        const bool early_live = KVBLK == QBLK || kv0 <= qb + rbid[0] * 16 + 15;
        constexpr std::integral_constant<int, 0> i0;
        constexpr std::integral_constant<int, 1> i1;
        constexpr std::integral_constant<int, 2> i2;
        if constexpr (pair_rows<D, PACKED>()) {
            if (early_live) tile_body(i0, i2, kv0);
            else tile_body(i1, i2, kv0);
        } else {
            if (early_live) tile_body(i0, i1, kv0);
            tile_body(i1, i2, kv0);
        }
        __syncthreads();   // K/V reused next tile
    }

    // ---- normalize + store: 4 consecutive d of one q row per register
    // quad, 8 bytes ----------------------------------------------------------
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int qrow = qb + rbid[rb] * 16 + col16;
        const float inv_l = 1.f / l_run[rb];
        #pragma unroll
        for (int jd = 0; jd < djtiles; ++jd) {
            const floatx4 o = o_acc[rb][jd] * inv_l;
            uint2 packed;
            packed.x = pack_bf16x2(o[0], o[1]);
            packed.y = pack_bf16x2(o[2], o[3]);
            *reinterpret_cast<uint2*>(
                O + bc.o_base + (long)qrow * bc.o_pitch + jd * 16 + k8 * 4) = packed;
        }
        if (k8 == 0)
            LSE[bc.row_base + qrow] = m_run[rb] + __logf(l_run[rb]);
    }
}

}  // namespace

std::vector<torch::Tensor> attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale) {
    const AttnDims a = check_attn_qkv(q, k, v);
    auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();

    auto o = torch::empty_like(qc);
    auto lse = torch::empty({a.B, a.H, a.S}, q.options().dtype(torch::kFloat32));

    const int grid = (int)(a.B * a.H * (a.S / QBLK));
    auto stream = c10::hip::getCurrentHIPStream().stream();
    dispatch_head_dim(a.D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((attn_fwd_kernel<DD, false>), dim3(grid), dim3(THREADS),
            FwdLayout<DD>::bytes, stream,
            bf16_ptr(qc), bf16_ptr(kc), bf16_ptr(vc), bf16_ptr(o),
            lse.data_ptr<float>(),
            (int)a.B, (int)a.H, (int)a.Hkv, (int)a.S, (float)scale);
    });
    HIP_CHECK_LAST();
    return {o, lse};
}

// Packed mode: q, k, v are read where the qkv GEMM left them and o is written
// where the proj GEMM reads it; no relayout copy on either side.
std::vector<torch::Tensor> attn_fwd_packed(
    torch::Tensor qkv, long H, long Hkv, long D, double scale) {
    const AttnDims a = check_attn_packed_qkv(qkv, H, Hkv, D);

    // every element is written by the kernel: 128-row tiles cover S, the
    // djtiles column tiles cover D, the grid covers every (batch, head)
    auto o = torch::empty({a.B, a.S, a.H * a.D}, qkv.options());
    auto lse = torch::empty({a.B, a.H, a.S}, qkv.options().dtype(torch::kFloat32));

    const int grid = (int)(a.B * a.H * (a.S / QBLK));
    auto stream = c10::hip::getCurrentHIPStream().stream();
    const bf16* base = bf16_ptr(qkv);
    dispatch_head_dim(a.D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((attn_fwd_kernel<DD, true>), dim3(grid), dim3(THREADS),
            FwdLayout<DD>::bytes, stream,
            base, base + a.H * a.D, base + (a.H + a.Hkv) * a.D, bf16_ptr(o),
            lse.data_ptr<float>(),
            (int)a.B, (int)a.H, (int)a.Hkv, (int)a.S, (float)scale);
    });
    HIP_CHECK_LAST();
    return {o, lse};
}
