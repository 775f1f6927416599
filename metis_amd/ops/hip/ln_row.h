// LayerNorm forward of one row held in registers (gfx950).
//
// A 256-thread workgroup takes a row of up to 8192 bf16 elements; thread t
// owns the 16-byte chunks t, t + 256, ... (NC = 1..4 of them, a template
// parameter), so the row is read once and stays in registers between the
// statistics and the normalisation. The caller fills the chunks: from
// memory (layernorm_fwd) or from residual + (y + bias) computed in place
// (bias_residual_layernorm_fwd), which is why this is a header.
//
// The statistics are summed in one fixed order, and every kernel built on
// this body gives the same mean, rstd and y bits for the same row: per
// thread over its chunks in increasing index, the 8 elements of a chunk in
// order, a 64-lane butterfly, then the four wave totals as
// (w0 + w2) + (w1 + w3). Which products are fused into the following add is
// spelled out as well (contraction is off in the body, fmaf where a fused
// multiply-add is meant), so the bits do not depend on how the compiler
// happens to pair the operations of one instantiation: d * d is rounded
// before it is added, the variance and the output use one fma each.
#pragma once

#include "common.h"

namespace ln_row {

constexpr int BLOCK = 256;
constexpr int VEC = 8;          // bf16 per chunk (16 B)
constexpr int MAX_CHUNKS = 4;   // per thread: H <= 8192
static_assert(BLOCK / WAVE_SIZE == 4, "row_stats adds four wave totals");

// The shift K of the variance sums: the mean of the row's first 8 elements
// (one chunk, the same for every thread) rounded to the bf16 grid of the
// largest of them. With d = x - K, var = E[d^2] - E[d]^2 subtracts numbers
// of the size of the variance, where E[x^2] - mean^2 subtracts two of the
// size of the squared mean and loses (mean/std)^2 ulps; d has as few bits
// as x, so the sums of d*d stay as nearly exact as sums of squares of bf16
// numbers are.
__device__ __forceinline__ float row_shift(const bf16x8 v0) {
    float shift = 0.f;
    float amax = 0.f;
    #pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float f = bf16_bits_to_float(v0[k]);
        shift += f;
        amax = fmaxf(amax, fabsf(f));
    }
    shift *= 1.f / VEC;
    // 1.5 * 2^23 grid units: adding and subtracting it rounds to the grid
    // (2^-7 of amax's power of two)
    const float big = __uint_as_float(
        __float_as_uint(amax) & 0x7f800000u) * 98304.f;
    return (shift + big) - big;
}

// v[c] is chunk threadIdx.x + c * BLOCK of the row (ignored where that is
// >= hv), v0 the row's chunk 0. Writes y, mean and rstd of the row.
// `scratch` is the workgroup's LDS; the caller puts a barrier between two
// rows.
template <int NC>
__device__ __forceinline__ void normalize(
    const bf16x8 (&v)[NC], const bf16x8 v0, int hv,
    const floatx4* __restrict__ gamma, const floatx4* __restrict__ beta,
    bf16x8* __restrict__ yrow, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, float eps,
    float (&scratch)[3][BLOCK / WAVE_SIZE]) {
    #pragma clang fp contract(off)
    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x / WAVE_SIZE;

    const float shift = row_shift(v0);
    float sum = 0.f, dsum = 0.f, dsumsq = 0.f;
    #pragma unroll
    for (int c = 0; c < NC; ++c) {
        if ((int)threadIdx.x + c * BLOCK < hv) {
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float f = bf16_bits_to_float(v[c][k]);
                float d = f - shift;
                sum += f;
                dsum += d;
                dsumsq += d * d;
            }
        }
    }
    // the three block sums share one barrier: every thread adds the four
    // wave totals itself, in a fixed order
    sum = wave_reduce_sum(sum);
    dsum = wave_reduce_sum(dsum);
    dsumsq = wave_reduce_sum(dsumsq);
    if (lane == 0) {
        scratch[0][wave] = sum;
        scratch[1][wave] = dsum;
        scratch[2][wave] = dsumsq;
    }
    __syncthreads();
    sum = (scratch[0][0] + scratch[0][2]) + (scratch[0][1] + scratch[0][3]);
    dsum = (scratch[1][0] + scratch[1][2]) + (scratch[1][1] + scratch[1][3]);
    dsumsq = (scratch[2][0] + scratch[2][2]) + (scratch[2][1] + scratch[2][3]);

    const float inv_n = 1.f / (hv * VEC);
    const float mean = sum * inv_n;
    const float dmean = dsum * inv_n;
    const float var = fmaxf(fmaf(-dmean, dmean, dsumsq * inv_n), 0.f);
    const float rstd = rsqrtf(var + eps);
    if (threadIdx.x == 0) {
        *mean_out = mean;
        *rstd_out = rstd;
    }

    #pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int i = (int)threadIdx.x + c * BLOCK;
        if (i < hv) {
            floatx4 g0 = gamma[i * 2], g1 = gamma[i * 2 + 1];
            floatx4 b0 = beta[i * 2], b1 = beta[i * 2 + 1];
            bf16x8 o;
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                float xn = (bf16_bits_to_float(v[c][k]) - mean) * rstd;
                o[k] = float_to_bf16_bits(fmaf(xn, g0[k], b0[k]));
            }
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                float xn = (bf16_bits_to_float(v[c][4 + k]) - mean) * rstd;
                o[4 + k] = float_to_bf16_bits(fmaf(xn, g1[k], b1[k]));
            }
            yrow[i] = o;
        }
    }
}

// bf16(residual + bf16(y + bias)) of one chunk: the two roundings of two
// separate bf16 adds.
__device__ __forceinline__ bf16x8 bias_residual(
    const bf16x8 y, const bf16x8 bias, const bf16x8 residual) {
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const short t = float_to_bf16_bits(
            bf16_bits_to_float(y[k]) + bf16_bits_to_float(bias[k]));
        o[k] = float_to_bf16_bits(
            bf16_bits_to_float(residual[k]) + bf16_bits_to_float(t));
    }
    return o;
}

}  // namespace ln_row
