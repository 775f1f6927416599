// Fused LayerNorm forward/backward for gfx950 (bf16 I/O, fp32 statistics).
//
// The transformer hot-op the Metis profiler times per layer (reference
// README.md:142-186 prescribes the per-layer profiler; the kernel itself is
// new MI355X work). Memory-bound: the design target is the HBM roofline
// (~6.3 TB/s achievable), reached by 16 B/lane vectorized bf16 access and
// one-pass row statistics (guide G13; scalar bf16 is ~2x slower).
//
// Layout: x [rows, H] row-major bf16; gamma/beta fp32[H]; y bf16;
// mean/rstd fp32[rows] saved for backward. Forward: one 256-thread block
// per row (grid-stride over rows), H a multiple of 8. Backward: norm_bwd.h.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "norm_bwd.h"

namespace {

constexpr int BLOCK = 256;
constexpr int VEC = 8;   // bf16 per lane per step (16 B)
static_assert(BLOCK / WAVE_SIZE == 4, "ln_fwd_kernel adds four wave totals");

__global__ void ln_fwd_kernel(
    const bf16x8* __restrict__ x,
    const floatx4* __restrict__ gamma,   // read as float4 pairs
    const floatx4* __restrict__ beta,
    bf16x8* __restrict__ y,
    float* __restrict__ mean_out,
    float* __restrict__ rstd_out,
    int rows,
    int hv,            // H / VEC
    float eps) {
    __shared__ float scratch[3][BLOCK / WAVE_SIZE];
    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    const int wave = threadIdx.x / WAVE_SIZE;

    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const bf16x8* xrow = x + (long)row * hv;

        // One statistics pass, three sums. The mean comes from the plain
        // sum. The variance comes from shifted sums: with d = x - K,
        // var = E[d^2] - E[d]^2 subtracts numbers of the size of the
        // variance, where E[x^2] - mean^2 subtracts two of the size of the
        // squared mean and loses (mean/std)^2 ulps. K is the mean of the
        // row's first 8 elements (one 16-byte load, the same for every
        // thread) rounded to the bf16 grid of the largest of them: d then
        // has as few bits as x, and the sums of d*d stay as nearly exact
        // as sums of squares of bf16 numbers are.
        float shift = 0.f;
        {
            const bf16x8 v0 = xrow[0];
            float amax = 0.f;
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float f = bf16_bits_to_float(v0[k]);
                shift += f;
                amax = fmaxf(amax, fabsf(f));
            }
            shift *= 1.f / VEC;
            // 1.5 * 2^23 grid units: adding and subtracting it rounds to
            // the grid (2^-7 of amax's power of two)
            const float big = __uint_as_float(
                __float_as_uint(amax) & 0x7f800000u) * 98304.f;
            shift = (shift + big) - big;
        }
        float sum = 0.f, dsum = 0.f, dsumsq = 0.f;
        for (int i = threadIdx.x; i < hv; i += BLOCK) {
            bf16x8 v = xrow[i];
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float f = bf16_bits_to_float(v[k]);
                float d = f - shift;
                sum += f;
                dsum += d;
                dsumsq += d * d;
            }
        }
        // the three block sums share one barrier: every thread adds the
        // four wave totals itself, in a fixed order
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
        const float var = fmaxf(dsumsq * inv_n - dmean * dmean, 0.f);
        const float rstd = rsqrtf(var + eps);
        if (threadIdx.x == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }

        bf16x8* yrow = y + (long)row * hv;
        for (int i = threadIdx.x; i < hv; i += BLOCK) {
            bf16x8 v = xrow[i];
            floatx4 g0 = gamma[i * 2], g1 = gamma[i * 2 + 1];
            floatx4 b0 = beta[i * 2], b1 = beta[i * 2 + 1];
            bf16x8 o;
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                float xn = (bf16_bits_to_float(v[k]) - mean) * rstd;
                o[k] = float_to_bf16_bits(xn * g0[k] + b0[k]);
            }
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                float xn = (bf16_bits_to_float(v[4 + k]) - mean) * rstd;
                o[4 + k] = float_to_bf16_bits(xn * g1[k] + b1[k]);
            }
            yrow[i] = o;
        }
        __syncthreads();
    }
}

// Backward: norm_bwd.h (streaming kernel shared with rmsnorm.hip).

}  // namespace

std::vector<torch::Tensor> layernorm_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta, double eps) {
    TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16, "x must be CUDA bf16");
    TORCH_CHECK(x.is_contiguous(), "x must be contiguous");
    const long H = x.size(-1);
    TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
    const long rows = x.numel() / H;
    TORCH_CHECK(gamma.is_cuda() && beta.is_cuda()
                && gamma.numel() == H && beta.numel() == H,
                "gamma and beta must be CUDA tensors of H elements");

    auto y = torch::empty_like(x);
    auto f32 = x.options().dtype(torch::kFloat32);
    auto mean = torch::empty({rows}, f32);
    auto rstd = torch::empty({rows}, f32);
    auto gamma_f = gamma.to(torch::kFloat32).contiguous();
    auto beta_f = beta.to(torch::kFloat32).contiguous();

    const int grid = (int)std::min<long>(rows, 2048);
    hipLaunchKernelGGL(
        ln_fwd_kernel, dim3(grid), dim3(BLOCK), 0,
        c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(x.data_ptr()),
        reinterpret_cast<const floatx4*>(gamma_f.data_ptr()),
        reinterpret_cast<const floatx4*>(beta_f.data_ptr()),
        reinterpret_cast<bf16x8*>(y.data_ptr()),
        mean.data_ptr<float>(), rstd.data_ptr<float>(),
        (int)rows, (int)(H / 8), (float)eps);
    HIP_CHECK_LAST();
    return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd) {
    norm_bwd::check_args(dy, x, gamma, &mean, rstd, 8192, "layernorm bwd");
    auto dyc = dy.contiguous();
    const long H = x.size(-1);
    const long rows = x.numel() / H;

    auto dx = torch::empty_like(x);
    auto f32 = x.options().dtype(torch::kFloat32);
    auto gamma_f = gamma.to(torch::kFloat32).contiguous();
    const int grid = norm_bwd::grid_for<false>(rows, H);
    auto part = torch::empty({2, grid, H}, f32);   // dgamma, dbeta slabs
    float* dgamma_part = part.data_ptr<float>();
    float* dbeta_part = dgamma_part + (long)grid * H;

    auto stream = c10::hip::getCurrentHIPStream().stream();
    norm_bwd::launch_main<false>(
        dyc.data_ptr(), x.data_ptr(), gamma_f.data_ptr<float>(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr(),
        dgamma_part, dbeta_part, rows, H, grid, stream);
    HIP_CHECK_LAST();

    auto dgamma = torch::empty({H}, f32);
    auto dbeta = torch::empty({H}, f32);
    norm_bwd::launch_reduce<false>(
        dgamma_part, dbeta_part, dgamma.data_ptr<float>(),
        dbeta.data_ptr<float>(), grid, (int)H, stream);
    HIP_CHECK_LAST();
    return {dx, dgamma, dbeta};
}
