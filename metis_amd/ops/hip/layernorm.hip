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
    __shared__ float scratch[BLOCK / WAVE_SIZE];

    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const bf16x8* xrow = x + (long)row * hv;

        float sum = 0.f, sumsq = 0.f;
        for (int i = threadIdx.x; i < hv; i += BLOCK) {
            bf16x8 v = xrow[i];
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float f = bf16_bits_to_float(v[k]);
                sum += f;
                sumsq += f * f;
            }
        }
        sum = block_reduce_sum(sum, scratch);
        __syncthreads();
        sumsq = block_reduce_sum(sumsq, scratch);

        const float inv_n = 1.f / (hv * VEC);
        const float mean = sum * inv_n;
        const float var = sumsq * inv_n - mean * mean;
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
    TORCH_CHECK(dy.is_cuda() && dy.dtype() == torch::kBFloat16, "dy must be CUDA bf16");
    TORCH_CHECK(x.is_contiguous() && mean.is_contiguous() && rstd.is_contiguous(),
                "x, mean and rstd must be contiguous");
    auto dyc = dy.contiguous();
    const long H = x.size(-1);
    const long rows = x.numel() / H;
    TORCH_CHECK(H % 8 == 0 && H <= 8192,
                "layernorm bwd supports hidden size % 8 == 0, <= 8192");
    TORCH_CHECK(rows >= 1 && dyc.numel() == x.numel() && mean.numel() == rows
                && rstd.numel() == rows, "layernorm bwd: shape mismatch");

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
