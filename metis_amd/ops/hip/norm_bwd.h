// Streaming backward shared by layernorm.hip and rmsnorm.hip (gfx950).
//
// The backward of a row norm needs dy + x in and dx out, once each: at
// 32768 x 2560 bf16 that is 503 MB, ~80 us at the ~6.3 TB/s achievable.
// To get near that the kernel keeps many independent rows in flight and
// never re-reads a row:
//  * thread i owns the 16-byte column chunk i of EVERY row its workgroup
//    visits (workgroup = ceil(H/8 / 64) waves), so gamma (8 floats) and the
//    dgamma/dbeta accumulators (8 + 8 floats) live in registers for the
//    whole kernel and no column index is ever recomputed;
//  * R rows are loaded per iteration (2 R independent 16-B loads per lane)
//    and stay in registers between the row statistics and dx;
//  * the R x {s1, s2} row sums cross the waves through one double-buffered
//    LDS slot: one barrier per R rows;
//  * the grid is one resident wave of workgroups (CUs x blocks per CU,
//    <= 1024) that grid-stride over row groups, each leaving one
//    dgamma/dbeta slab; norm_bwd_reduce_kernel sums the slabs in a fixed
//    order, so the result is deterministic (no atomics).
//
// ADD (LayerNorm only) folds the gradient of a residual branch in: with one
// more input dres [rows, H] the kernel writes g = bf16(dres + bf16(dx)), the
// sum autograd would form from the two rounded tensors, and keeps a third
// set of 8 accumulators for the column sums of the rounded g, which is the
// bias gradient of the linear layer in front of the residual add. Neither
// costs a pass of its own. ADD = false is the kernel without any of it.
#pragma once

#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <algorithm>

#include "common.h"

namespace norm_bwd {

constexpr int VEC = 8;          // bf16 per lane per row (16 B)
constexpr int MAX_WAVES = 16;   // 1024 threads = H 8192
constexpr int MAX_SLABS = 1024;

// Arguments of layernorm_bwd / rmsnorm_bwd (mean == nullptr). The kernels
// read x and dy as [rows, H] bf16, H floats of gamma and `rows` floats of
// mean and rstd, all through raw pointers: every one of those sizes,
// dtypes and devices is pinned here, before anything is launched.
inline void check_args(const torch::Tensor& dy, const torch::Tensor& x,
                       const torch::Tensor& gamma, const torch::Tensor* mean,
                       const torch::Tensor& rstd, long max_h, const char* op) {
    TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16,
                op, ": x must be CUDA bf16");
    TORCH_CHECK(dy.is_cuda() && dy.dtype() == torch::kBFloat16,
                op, ": dy must be CUDA bf16");
    TORCH_CHECK(x.dim() >= 1 && x.is_contiguous(), op, ": x must be contiguous");
    const long H = x.size(-1);
    TORCH_CHECK(H > 0 && H % VEC == 0 && H <= max_h,
                op, " supports hidden size % 8 == 0, <= ", max_h);
    const long rows = x.numel() / H;
    TORCH_CHECK(rows >= 1 && rows < (1L << 31), op, ": row count out of range");
    TORCH_CHECK(dy.dim() >= 1 && dy.size(-1) == H && dy.numel() == x.numel(),
                op, ": dy must have x's row length and row count");
    TORCH_CHECK(gamma.is_cuda() && gamma.numel() == H,
                op, ": gamma must be a CUDA tensor of H elements");
    TORCH_CHECK(rstd.is_cuda() && rstd.dtype() == torch::kFloat32
                && rstd.is_contiguous() && rstd.numel() == rows,
                op, ": rstd must be a contiguous CUDA fp32 tensor, one per row");
    if (mean)
        TORCH_CHECK(mean->is_cuda() && mean->dtype() == torch::kFloat32
                    && mean->is_contiguous() && mean->numel() == rows,
                    op, ": mean must be a contiguous CUDA fp32 tensor, one per row");
    for (const torch::Tensor* t : {&dy, &gamma, &rstd, mean})
        TORCH_CHECK(!t || t->get_device() == x.get_device(),
                    op, ": all arguments must be on x's device");
}

// RMS = false: LayerNorm, xhat = (x - mean) * rstd,
//   dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)), dgamma, dbeta.
// RMS = true:  RMSNorm, xhat = x * rstd,
//   dx = rstd * dy*g - rstd * xhat * mean(dy*g*xhat), dgamma only.
template <bool RMS, int R, int MAXT, bool ADD = false>
__global__ void __launch_bounds__(MAXT) norm_bwd_kernel(
    const bf16x8* __restrict__ dy,
    const bf16x8* __restrict__ x,
    const floatx4* __restrict__ gamma,
    const float* __restrict__ mean_in,    // unused when RMS
    const float* __restrict__ rstd_in,
    bf16x8* __restrict__ dx,
    float* __restrict__ dgamma_part,      // [gridDim.x, H]
    float* __restrict__ dbeta_part,       // [gridDim.x, H], unused when RMS
    int rows,
    int hv,                               // H / VEC
    const bf16x8* __restrict__ dres,      // ADD only
    float* __restrict__ colsum_part) {    // [gridDim.x, H], ADD only
    static_assert(!(RMS && ADD), "ADD is instantiated for LayerNorm only");
    constexpr int NS = RMS ? 1 : 2;       // row sums per row
    __shared__ float red[2][MAX_WAVES][R * NS];

    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x / WAVE_SIZE;
    const int nw = blockDim.x / WAVE_SIZE;
    // lanes past the row in the last wave load chunk hv-1 again (always a
    // valid address, no branch around the loads) and contribute zeros
    const bool live = (int)threadIdx.x < hv;
    const int ci = live ? (int)threadIdx.x : hv - 1;

    float g[VEC], dg[VEC], db[VEC], cs[ADD ? VEC : 1];
    {
        const floatx4 g0 = gamma[ci * 2], g1 = gamma[ci * 2 + 1];
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[k] = g0[k];
            g[4 + k] = g1[k];
        }
        #pragma unroll
        for (int k = 0; k < VEC; ++k) dg[k] = db[k] = 0.f;
        #pragma unroll
        for (int k = 0; k < (ADD ? VEC : 1); ++k) cs[k] = 0.f;
    }
    const float inv_n = 1.f / (hv * VEC);
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    int buf = 0;
    for (long r0 = (long)blockIdx.x * R; r0 < rows; r0 += (long)gridDim.x * R) {
        bf16x8 dv[R], xv[R], av[ADD ? R : 1];
        float mu[R], rs[R];
        bool ok[R];
        #pragma unroll
        for (int r = 0; r < R; ++r) {
            // rows past the end re-read the last row and are zeroed below
            const long row = (r0 + r < rows) ? r0 + r : (long)rows - 1;
            ok[r] = live && (r0 + r < rows);
            dv[r] = dy[row * hv + ci];
            xv[r] = x[row * hv + ci];
            if (ADD) av[r] = dres[row * hv + ci];
            rs[r] = rstd_in[row];
            mu[r] = RMS ? 0.f : mean_in[row];
        }

        float s[R][NS];
        #pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!ok[r]) dv[r] = zero8;    // dy = 0: adds nothing anywhere
            float s1 = 0.f, s2 = 0.f;
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float dyf = bf16_bits_to_float(dv[r][k]);
                const float xhat = (bf16_bits_to_float(xv[r][k]) - mu[r]) * rs[r];
                const float dyg = dyf * g[k];
                s1 += dyg;
                s2 += dyg * xhat;
                dg[k] += dyf * xhat;
                db[k] += dyf;
            }
            s[r][NS - 1] = wave_reduce_sum(s2);
            if (!RMS) s[r][0] = wave_reduce_sum(s1);
        }
        if (lane == 0) {
            #pragma unroll
            for (int r = 0; r < R; ++r)
                #pragma unroll
                for (int j = 0; j < NS; ++j) red[buf][wave][r * NS + j] = s[r][j];
        }
        __syncthreads();
        // every thread sums the waves in the same order: one value per row
        #pragma unroll
        for (int r = 0; r < R; ++r)
            #pragma unroll
            for (int j = 0; j < NS; ++j) s[r][j] = 0.f;
        for (int w = 0; w < nw; ++w) {
            #pragma unroll
            for (int r = 0; r < R; ++r)
                #pragma unroll
                for (int j = 0; j < NS; ++j) s[r][j] += red[buf][w][r * NS + j];
        }
        buf ^= 1;   // next iteration writes the other slot: one barrier each

        #pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s2 = s[r][NS - 1] * inv_n;
            const float s1 = RMS ? 0.f : s[r][0] * inv_n;
            bf16x8 o;
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float dyf = bf16_bits_to_float(dv[r][k]);
                const float xhat = (bf16_bits_to_float(xv[r][k]) - mu[r]) * rs[r];
                const float v = RMS ? rs[r] * (dyf * g[k]) - rs[r] * xhat * s2
                                    : rs[r] * (dyf * g[k] - s1 - xhat * s2);
                o[k] = float_to_bf16_bits(v);
                if (ADD) {
                    // the sum of the two rounded tensors, rounded; its
                    // column sum takes the rounded value (dead rows and
                    // lanes add nothing)
                    o[k] = float_to_bf16_bits(bf16_bits_to_float(av[r][k])
                                              + bf16_bits_to_float(o[k]));
                    cs[k] += ok[r] ? bf16_bits_to_float(o[k]) : 0.f;
                }
            }
            if (ok[r]) dx[(r0 + r) * hv + ci] = o;
        }
    }

    if (live) {
        const long base = ((long)blockIdx.x * hv + ci) * 2;
        floatx4* gp = reinterpret_cast<floatx4*>(dgamma_part);
        gp[base] = floatx4{dg[0], dg[1], dg[2], dg[3]};
        gp[base + 1] = floatx4{dg[4], dg[5], dg[6], dg[7]};
        if (!RMS) {
            floatx4* bp = reinterpret_cast<floatx4*>(dbeta_part);
            bp[base] = floatx4{db[0], db[1], db[2], db[3]};
            bp[base + 1] = floatx4{db[4], db[5], db[6], db[7]};
        }
        if (ADD) {
            floatx4* cp = reinterpret_cast<floatx4*>(colsum_part);
            cp[base] = floatx4{cs[0], cs[1], cs[2], cs[3]};
            cp[base + 1] = floatx4{cs[4], cs[5], cs[6], cs[7]};
        }
    }
}

// Sum the slabs into dgamma (and dbeta, and with THIRD a third array, each
// in the same order). A workgroup owns 16 columns and
// spreads the slabs over 64 lanes of them, so every load of a thread is
// independent; the 64 partials of a column are then added in a fixed order
// (shuffle over the 4 in a wave, then 16 waves through LDS).
constexpr int RED_COLS = 16;
constexpr int RED_THREADS = 1024;

template <bool RMS, bool THIRD = false>
__global__ void __launch_bounds__(RED_THREADS) norm_bwd_reduce_kernel(
    const float* __restrict__ dgamma_part,
    const float* __restrict__ dbeta_part,
    float* __restrict__ dgamma,
    float* __restrict__ dbeta,
    int nslabs,
    int H,
    const float* __restrict__ third_part,   // THIRD only
    float* __restrict__ third) {
    constexpr int SL = RED_THREADS / RED_COLS;          // 64 slab lanes
    constexpr int NWAVE = RED_THREADS / WAVE_SIZE;      // 16
    __shared__ float red[THIRD ? 3 : 2][NWAVE][RED_COLS];

    const int cx = threadIdx.x % RED_COLS;
    const int sy = threadIdx.x / RED_COLS;
    const int col = blockIdx.x * RED_COLS + cx;
    float g = 0.f, b = 0.f, c = 0.f;
    if (col < H) {
        #pragma unroll 4
        for (int s = sy; s < nslabs; s += SL) {
            g += dgamma_part[(long)s * H + col];
            if (!RMS) b += dbeta_part[(long)s * H + col];
            if (THIRD) c += third_part[(long)s * H + col];
        }
    }
    g += __shfl_xor(g, 16, WAVE_SIZE);
    g += __shfl_xor(g, 32, WAVE_SIZE);
    if (!RMS) {
        b += __shfl_xor(b, 16, WAVE_SIZE);
        b += __shfl_xor(b, 32, WAVE_SIZE);
    }
    if (THIRD) {
        c += __shfl_xor(c, 16, WAVE_SIZE);
        c += __shfl_xor(c, 32, WAVE_SIZE);
    }
    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x / WAVE_SIZE;
    if (lane < RED_COLS) {
        red[0][wave][cx] = g;
        if (!RMS) red[1][wave][cx] = b;
        if (THIRD) red[2][wave][cx] = c;
    }
    __syncthreads();
    if (threadIdx.x < RED_COLS && col < H) {
        g = 0.f;
        b = 0.f;
        c = 0.f;
        #pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            g += red[0][w][cx];
            if (!RMS) b += red[1][w][cx];
            if (THIRD) c += red[2][w][cx];
        }
        dgamma[col] = g;
        if (!RMS) dbeta[col] = b;
        if (THIRD) third[col] = c;
    }
}

template <bool RMS, bool THIRD = false>
void launch_reduce(const float* dgamma_part, const float* dbeta_part,
                   float* dgamma, float* dbeta, int nslabs, int H,
                   hipStream_t stream, const float* third_part = nullptr,
                   float* third = nullptr) {
    hipLaunchKernelGGL((norm_bwd_reduce_kernel<RMS, THIRD>),
        dim3((H + RED_COLS - 1) / RED_COLS), dim3(RED_THREADS), 0, stream,
        dgamma_part, dbeta_part, dgamma, dbeta, nslabs, H, third_part, third);
}

// Rows per iteration. 4 rows cost ~136 VGPRs = 3 waves/SIMD = 12 waves/CU;
// 2 rows fit 4 waves/SIMD = 16 waves/CU. Workgroups of up to 6 waves fill
// 10-12 of the 12 either way and take 4 rows (most bytes in flight: at
// H = 2560, 2 x 5 waves x 8 KB per CU). 7 and 8 waves fit 12 only once, so
// 2 rows put the same bytes in flight from two workgroups whose barriers
// do not line up; from 9 waves on only the 2-row kernel fits at all.
constexpr int R4_MAX_THREADS = 384;

inline int block_threads(long H) {
    return (int)((H / VEC + WAVE_SIZE - 1) / WAVE_SIZE * WAVE_SIZE);
}

template <typename Fn>
int resident_blocks(Fn fn, int threads) {
    int per_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, fn, threads, 0);
    TORCH_CHECK(e == hipSuccess && per_cu > 0, "norm bwd: occupancy query failed");
    const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    return std::min(per_cu * cus, MAX_SLABS);
}

// Workgroups (= slabs) for a [rows, H] problem, H <= 8192: one resident
// wave of the chip (asked of the runtime once per workgroup size), capped
// by MAX_SLABS and by the row groups there are.
template <bool RMS>
int grid_for(long rows, long H) {
    const int threads = block_threads(H);
    TORCH_CHECK(threads <= MAX_WAVES * WAVE_SIZE, "norm bwd: hidden size > 8192");
    static int cache[MAX_WAVES + 1] = {};
    int& resident = cache[threads / WAVE_SIZE];
    if (threads <= R4_MAX_THREADS) {
        if (resident == 0)
            resident = resident_blocks(
                norm_bwd_kernel<RMS, 4, R4_MAX_THREADS>, threads);
        return (int)std::min<long>(resident, (rows + 3) / 4);
    }
    if (resident == 0)
        resident = resident_blocks(norm_bwd_kernel<RMS, 2, 1024>, threads);
    return (int)std::min<long>(resident, (rows + 1) / 2);
}

// dx plus `grid` slabs ([grid, H] floats each in dgamma_part/dbeta_part).
// ADD: g = dres + dx in dx's place and a third slab array colsum_part.
template <bool RMS, bool ADD = false>
void launch_main(const void* dy, const void* x, const float* gamma,
                 const float* mean, const float* rstd, void* dx,
                 float* dgamma_part, float* dbeta_part,
                 long rows, long H, int grid, hipStream_t stream,
                 const void* dres = nullptr, float* colsum_part = nullptr) {
    const int threads = block_threads(H);
    #define NORM_BWD_LAUNCH(RR, MT)                                            \
        hipLaunchKernelGGL((norm_bwd_kernel<RMS, RR, MT, ADD>), dim3(grid),    \
            dim3(threads), 0, stream,                                          \
            reinterpret_cast<const bf16x8*>(dy),                               \
            reinterpret_cast<const bf16x8*>(x),                                \
            reinterpret_cast<const floatx4*>(gamma), mean, rstd,               \
            reinterpret_cast<bf16x8*>(dx), dgamma_part, dbeta_part,            \
            (int)rows, (int)(H / VEC),                                         \
            reinterpret_cast<const bf16x8*>(dres), colsum_part)
    if (threads <= R4_MAX_THREADS) NORM_BWD_LAUNCH(4, R4_MAX_THREADS);
    else NORM_BWD_LAUNCH(2, 1024);
    #undef NORM_BWD_LAUNCH
}

}  // namespace norm_bwd
