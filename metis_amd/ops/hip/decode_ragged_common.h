// Pieces shared by the ragged split-S decode kernels (decode_ragged.hip on
// a bf16 cache, decode_ragged_fp8.hip on an e4m3 cache) and the cache
// writer kv_quant.hip: the lane-group geometry (8 elements per lane, LPR
// lanes per K/V row), the DPP group reductions, the merge of the
// per-lane-group online-softmax states into one workgroup result, the
// combine kernel of pass 2 and the host-side split rule.
//
// decode_ragged.hip keeps its own inline copy of the merge that
// merge_and_write() holds: calling the function there changed the bf16
// instantiations' register allocation (docs/KERNELS.md records their
// figures), so only the fp8 kernel uses it.
//
// Everything is in an anonymous namespace: each translation unit that
// includes this header gets its own copy of the combine kernel.
#pragma once

#include <torch/extension.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int NWAVE = THREADS / WAVE_SIZE;
constexpr int COMBINE_THREADS = 128;
constexpr float NEG_BIG = -1e30f;

typedef unsigned int uintx4 __attribute__((ext_vector_type(4)));

// Lanes that share one K/V row of D elements, 8 elements each.
template <int D>
struct RowLanes { static constexpr int value = D == 64 ? 8 : 16; };

__device__ __forceinline__ void unpack8(bf16x8 raw, float* f) {
    const uintx4 w = __builtin_bit_cast(uintx4, raw);
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

// Cross-lane read inside a 16-lane DPP row (no LDS traffic, unlike the
// ds_bpermute behind __shfl_xor). Controls: quad_perm [1,0,3,2] and
// [2,3,0,1] (xor 1, xor 2), row_half_mirror (lane i <- 7-i of its 8),
// row_mirror (lane i <- 15-i of its 16).
template <int CTRL>
__device__ __forceinline__ float dpp_read(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(
        0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// Sum over the LPR (8 or 16) aligned lanes that share a K/V row; every
// lane of the group ends with the total.
template <int LPR>
__device__ __forceinline__ float group_sum(float x) {
    x += dpp_read<0xB1>(x);
    x += dpp_read<0x4E>(x);
    x += dpp_read<0x141>(x);      // quad sums are lane-uniform: mirror = other quad
    if (LPR == 16) x += dpp_read<0x140>(x);
    return x;
}

// The same butterfly with max (x >= 0 everywhere, so the 0 a DPP read
// returns for a lane outside the exec mask cannot win wrongly).
template <int LPR>
__device__ __forceinline__ float group_max(float x) {
    x = fmaxf(x, dpp_read<0xB1>(x));
    x = fmaxf(x, dpp_read<0x4E>(x));
    x = fmaxf(x, dpp_read<0x141>(x));
    if (LPR == 16) x = fmaxf(x, dpp_read<0x140>(x));
    return x;
}

// End of pass 1: every lane group holds an online-softmax state
// (m, l, acc[8]) per query head of its kv head. Groups merge by shuffle,
// the four waves merge through LDS, and the workgroup writes one fp32
// partial per (b, h, split) — or bf16 output directly when
// num_splits == 1.
template <int D, int G>
__device__ __forceinline__ void merge_and_write(
    float (&m)[G], float (&l)[G], float (&acc)[G][8],
    short* __restrict__ Out, float* __restrict__ ws_acc,
    float* __restrict__ ws_ml, int H, int num_splits,
    int split, int kvh, int b) {
    constexpr int LPR = RowLanes<D>::value;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int d0 = sub * 8;
    const bool act = d0 < D;

    // merge the lane groups of a wave (butterfly over the group index)
    #pragma unroll
    for (int off = LPR; off < WAVE_SIZE; off <<= 1) {
        #pragma unroll
        for (int g = 0; g < G; ++g) {
            const float m_o = __shfl_xor(m[g], off, WAVE_SIZE);
            const float l_o = __shfl_xor(l[g], off, WAVE_SIZE);
            const float m_n = fmaxf(m[g], m_o);
            const float a = __expf(m[g] - m_n), bb = __expf(m_o - m_n);
            l[g] = l[g] * a + l_o * bb;
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float acc_o = __shfl_xor(acc[g][j], off, WAVE_SIZE);
                acc[g][j] = acc[g][j] * a + acc_o * bb;
            }
            m[g] = m_n;
        }
    }

    // merge the 4 wave-partials through LDS
    __shared__ float sm[NWAVE][G], sl[NWAVE][G];
    __shared__ float sacc[NWAVE][G][D];
    if (grp == 0 && act) {
        #pragma unroll
        for (int g = 0; g < G; ++g) {
            #pragma unroll
            for (int j = 0; j < 8; ++j) sacc[wave][g][d0 + j] = acc[g][j];
        }
    }
    if (lane == 0) {
        #pragma unroll
        for (int g = 0; g < G; ++g) { sm[wave][g] = m[g]; sl[wave][g] = l[g]; }
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < G * D; idx += THREADS) {
        const int g = idx / D, d = idx % D;
        float gm = NEG_BIG;
        #pragma unroll
        for (int w = 0; w < NWAVE; ++w) gm = fmaxf(gm, sm[w][g]);
        float gl = 0.f, ga = 0.f;
        #pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            const float aw = __expf(sm[w][g] - gm);
            gl += sl[w][g] * aw;
            ga += sacc[w][g][d] * aw;
        }
        const long bh = (long)b * H + kvh * G + g;
        if (num_splits == 1) {
            Out[bh * D + d] = float_to_bf16_bits(gl > 0.f ? ga / gl : 0.f);
        } else {
            const long slot = bh * num_splits + split;
            ws_acc[slot * D + d] = ga;
            if (d == 0) { ws_ml[slot * 2] = gm; ws_ml[slot * 2 + 1] = gl; }
        }
    }
}

// One workgroup per (b, h): thread d merges element d of the partials.
__global__ __launch_bounds__(COMBINE_THREADS) void attn_decode_combine_kernel(
    const float* __restrict__ ws_acc,   // [B*H, num_splits, D]
    const float* __restrict__ ws_ml,    // [B*H, num_splits, 2]
    short* __restrict__ Out,            // [B*H, D]
    int D, int num_splits) {
    const long bh = blockIdx.x;
    const int d = threadIdx.x;
    if (d >= D) return;
    const float* ml = ws_ml + bh * num_splits * 2;
    float gm = NEG_BIG;
    for (int s = 0; s < num_splits; ++s) gm = fmaxf(gm, ml[2 * s]);
    float gl = 0.f, ga = 0.f;
    for (int s = 0; s < num_splits; ++s) {
        const float w = __expf(ml[2 * s] - gm);
        gl += ml[2 * s + 1] * w;
        ga += ws_acc[(bh * num_splits + s) * D + d] * w;
    }
    Out[bh * D + d] = float_to_bf16_bits(gl > 0.f ? ga / gl : 0.f);
}

// Host-side split count from shapes only (no device sync): about two
// workgroups per CU, each split at least MIN_ROWS rows.
inline int auto_num_splits(long B, long Hkv, long S) {
    constexpr long TARGET_WG = 2 * 256, MIN_ROWS = 256, MAX_SPLITS = 64;
    const long want = (TARGET_WG + B * Hkv - 1) / (B * Hkv);
    const long fit = std::max<long>(S / MIN_ROWS, 1);
    return (int)std::min({want, fit, MAX_SPLITS});
}

}  // namespace
