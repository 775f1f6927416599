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
//   * Q fragments preloaded to registers; K B-fragments are plain reads of
//     the K image, V B-fragments come from ds_read_b64_tr_b16 (hardware
//     transpose) off the V image — no transposed copy exists;
//   * per-row (m, l) online softmax; P goes through a per-wave LDS tile
//     (C layout -> A layout), published by a wave-local compiler fence;
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

// KV tile width: 128 for D <= 80 (the K/V/P images still fit two blocks
// per CU), 64 above. Wider tiles amortize the two barriers per tile over
// twice the MFMA work.
template <int D>
constexpr int kvblk_for() { return D <= 80 ? 128 : 64; }

// LDS: K and V images of KVBLK rows, P tiles [4 waves][2 row blocks][16][VROW]
template <int D>
using FwdLayout = TileLayout<D, kvblk_for<D>(), THREADS / 64 * 2, RESIDENT>;
static_assert(FwdLayout<64>::bytes == 71680 && FwdLayout<80>::bytes == 79872
              && FwdLayout<96>::bytes == 45056 && FwdLayout<128>::bytes == 53248);

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
    const int wave = threadIdx.x >> 6;
    const int col16 = lane & 15;
    const int k8 = lane >> 4;

    using L = FwdLayout<D>;
    constexpr int KVBLK = kvblk_for<D>();    // kv columns per tile
    constexpr int JSUB = KVBLK / 16;         // 16-col S subtiles per tile
    constexpr int dchunks = Geom<D>::dchunks;
    constexpr int djtiles = Geom<D>::djtiles;
    constexpr int KSLOT = Geom<D>::KSLOT;
    constexpr int VROW = L::WROW;            // P tile row length

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
    short* Pw = reinterpret_cast<short*>(smem) + L::w_off + wave * 2 * L::w_tile;

    // ---- preload Q fragments for both row blocks ------------------------
    bf16x8 q_frag[2][dchunks];
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb)
        #pragma unroll
        for (int c = 0; c < dchunks; ++c)
            q_frag[rb][c] = frag8<D>(Q + q_base, qb + rbid[rb] * 16 + col16,
                                     c * 32 + k8 * 8, pitch);

    float m_run[2][4], l_run[2][4];
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            m_run[rb][r] = -1e30f;
            l_run[rb][r] = 0.f;
        }
    floatx4 o_acc[2][djtiles] = {};

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

    const int kv_end = qb + QBLK;
    stage.issue_loads(Kh, Vh, 0, pitch, pitch);
    for (int kv0 = 0; kv0 < kv_end; kv0 += KVBLK) {
        stage.write_stage(Ks, Vs, Vh, kv0, pitch);
        if (kv0 + KVBLK < kv_end) stage.issue_loads(Kh, Vh, kv0 + KVBLK, pitch,
                                                      pitch);
        __syncthreads();

        // ---- per row block: S = scale * Q K^T, online softmax, P -> LDS -
        bool rb_active[2];
        float p[2][JSUB][4];   // [rb][j][r]
        #pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int q0 = qb + rbid[rb] * 16;
            rb_active[rb] = kv0 <= q0 + 15;
            if (!rb_active[rb]) continue;

            __builtin_amdgcn_s_setprio(1);   // T5: favor the MFMA cluster
            #pragma unroll
            for (int j = 0; j < JSUB; ++j) {    // 16-col subtiles
                floatx4 s_acc = floatx4{0.f, 0.f, 0.f, 0.f};
                const int kvrow = j * 16 + col16;
                #pragma unroll
                for (int c = 0; c < dchunks; ++c) {
                    const bf16x8 k_frag =
                        lds_frag<D, KSLOT>(Ks, kvrow, c * 32 + k8 * 8);
                    s_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        q_frag[rb][c], k_frag, s_acc, 0, 0, 0);
                }
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qrow = q0 + k8 * 4 + r;
                    const int kvcol = kv0 + j * 16 + col16;
                    float sv = s_acc[r] * scale;
                    p[rb][j][r] = (kvcol > qrow) ? -1e30f : sv;
                }
            }
            __builtin_amdgcn_s_setprio(0);

            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                float tile_max = -1e30f;
                #pragma unroll
                for (int j = 0; j < JSUB; ++j)
                    tile_max = fmaxf(tile_max, p[rb][j][r]);
                #pragma unroll
                for (int off = 8; off > 0; off >>= 1)
                    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, off, 16));

                const float m_new = fmaxf(m_run[rb][r], tile_max);
                const float alpha = __expf(m_run[rb][r] - m_new);
                float row_sum = 0.f;
                #pragma unroll
                for (int j = 0; j < JSUB; ++j) {
                    p[rb][j][r] = __expf(p[rb][j][r] - m_new);
                    row_sum += p[rb][j][r];
                }
                #pragma unroll
                for (int off = 8; off > 0; off >>= 1)
                    row_sum += __shfl_xor(row_sum, off, 16);

                l_run[rb][r] = l_run[rb][r] * alpha + row_sum;
                m_run[rb][r] = m_new;
                #pragma unroll
                for (int jd = 0; jd < djtiles; ++jd)
                    o_acc[rb][jd][r] *= alpha;
            }

            short* Prb = Pw + rb * 16 * VROW;
            #pragma unroll
            for (int j = 0; j < JSUB; ++j)
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    Prb[(k8 * 4 + r) * VROW + j * 16 + col16] =
                        float_to_bf16_bits(p[rb][j][r]);
        }

        // P is per-wave private: DS ops of one wave complete in order, so
        // a compiler-level fence (no barrier) suffices to keep the vector
        // re-read below the scalar writes above.
        asm volatile("" ::: "memory");

        // ---- O += P @ V -------------------------------------------------
        #pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            if (!rb_active[rb]) continue;
            const short* Prb = Pw + rb * 16 * VROW;
            // V B-fragments via hardware transpose read (tr16_frag)
            #pragma unroll
            for (int ks = 0; ks < KVBLK / 32; ++ks) {   // 32-wide kv chunks
                bf16x8 p_frag = *reinterpret_cast<const bf16x8*>(
                    Prb + col16 * VROW + ks * 32 + k8 * 8);
                #pragma unroll
                for (int jd = 0; jd < djtiles; ++jd) {
                    const bf16x8 v_frag = tr16_frag<KSLOT>(
                        Vs, ks * 32 + k8 * 8, jd * 16, col16);
                    o_acc[rb][jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        p_frag, v_frag, o_acc[rb][jd], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // K/V/P reused next tile
    }

    // ---- normalize + store ----------------------------------------------
    #pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qrow = qb + rbid[rb] * 16 + k8 * 4 + r;
            const float inv_l = 1.f / l_run[rb][r];
            #pragma unroll
            for (int jd = 0; jd < djtiles; ++jd)
                O[bc.o_base + (long)qrow * bc.o_pitch + jd * 16 + col16] =
                    __float2bfloat16(o_acc[rb][jd][r] * inv_l);
            if (col16 == 0)
                LSE[bc.row_base + qrow] =
                    m_run[rb][r] + __logf(l_run[rb][r]);
        }
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
