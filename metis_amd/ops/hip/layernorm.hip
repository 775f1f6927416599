// Fused LayerNorm forward/backward for gfx950 (bf16 I/O, fp32 statistics).
//
// The transformer hot-op the Metis profiler times per layer (reference
// README.md:142-186 prescribes the per-layer profiler; the kernel itself is
// new MI355X work). Memory-bound: the design target is the HBM roofline
// (~6.3 TB/s achievable), reached by 16 B/lane vectorized bf16 access and
// one read of every row (guide G13; scalar bf16 is ~2x slower).
//
// Layout: x [rows, H] row-major bf16; gamma/beta fp32[H]; y bf16;
// mean/rstd fp32[rows] saved for backward. Forward: one 256-thread block
// per row (grid-stride over rows) holding the row in registers (ln_row.h),
// H a multiple of 8 up to 8192. The same row body serves
// bias_residual_layernorm_fwd, which forms x = residual + (y + bias) in
// registers first, so the add costs no pass of its own. Backward:
// norm_bwd.h.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "ln_row.h"
#include "norm_bwd.h"

namespace {

using ln_row::BLOCK;
using ln_row::VEC;
constexpr long MAX_H = (long)ln_row::MAX_CHUNKS * BLOCK * VEC;   // 8192

// FUSED = false: z, mean, rstd = LayerNorm(in0), in0 = x.
// FUSED = true:  x_out = bf16(residual + bf16(in0 + bias)), in0 = y, then
//                z, mean, rstd = LayerNorm(x_out) on the rounded x_out.
template <int NC, bool FUSED>
__global__ void __launch_bounds__(BLOCK) ln_fwd_kernel(
    const bf16x8* __restrict__ in0,
    const bf16x8* __restrict__ bias,       // FUSED only
    const bf16x8* __restrict__ residual,   // FUSED only
    bf16x8* __restrict__ x_out,            // FUSED only
    const floatx4* __restrict__ gamma,     // read as float4 pairs
    const floatx4* __restrict__ beta,
    bf16x8* __restrict__ z,
    float* __restrict__ mean_out,
    float* __restrict__ rstd_out,
    int rows,
    int hv,            // H / VEC
    float eps) {
    __shared__ float scratch[3][BLOCK / WAVE_SIZE];
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    bf16x8 bv[NC], b0 = zero8;
    if (FUSED) {
        b0 = bias[0];
        #pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int i = (int)threadIdx.x + c * BLOCK;
            bv[c] = i < hv ? bias[i] : zero8;
        }
    }

    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const long off = (long)row * hv;
        bf16x8 v[NC], v0;
        if (!FUSED) {
            v0 = in0[off];
            #pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int i = (int)threadIdx.x + c * BLOCK;
                v[c] = i < hv ? in0[off + i] : zero8;
            }
        } else {
            // every thread forms the row's first chunk itself (the shift
            // of the variance sums comes from it): one more 16-byte load
            // per input, the same address for the whole workgroup
            bf16x8 yv[NC], rv[NC];
            const bf16x8 y0 = in0[off], r0 = residual[off];
            #pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int i = (int)threadIdx.x + c * BLOCK;
                yv[c] = i < hv ? in0[off + i] : zero8;
                rv[c] = i < hv ? residual[off + i] : zero8;
            }
            v0 = ln_row::bias_residual(y0, b0, r0);
            #pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int i = (int)threadIdx.x + c * BLOCK;
                v[c] = ln_row::bias_residual(yv[c], bv[c], rv[c]);
                if (i < hv) x_out[off + i] = v[c];
            }
        }
        ln_row::normalize<NC>(v, v0, hv, gamma, beta, z + off,
                              mean_out + row, rstd_out + row, eps, scratch);
        __syncthreads();   // scratch is reused by the next row
    }
}

// x = bf16(residual + bf16(y + bias)) alone: thread = one 16-byte chunk,
// grid-stride; the bias column is carried along instead of divided out.
__global__ void __launch_bounds__(BLOCK) bias_residual_add_kernel(
    const bf16x8* __restrict__ y,
    const bf16x8* __restrict__ bias,
    const bf16x8* __restrict__ residual,
    bf16x8* __restrict__ x,
    long n,            // rows * hv
    int hv) {
    const long stride = (long)gridDim.x * BLOCK;
    long idx = (long)blockIdx.x * BLOCK + threadIdx.x;
    int col = (int)(idx % hv);
    const int step = (int)(stride % hv);
    for (; idx < n; idx += stride) {
        x[idx] = ln_row::bias_residual(y[idx], bias[col], residual[idx]);
        col += step;
        if (col >= hv) col -= hv;
    }
}

// Arguments of the forward entries. The kernels read y/x and residual as
// [rows, H] bf16, H bf16 of bias and H floats of gamma and beta through
// raw pointers: sizes, dtypes and devices are pinned here, before anything
// is launched. residual/bias/gamma/beta may be null (not used by the op).
void check_fwd_args(const torch::Tensor& y, const torch::Tensor* bias,
                    const torch::Tensor* residual, const torch::Tensor* gamma,
                    const torch::Tensor* beta, const char* op) {
    TORCH_CHECK(y.is_cuda() && y.dtype() == torch::kBFloat16,
                op, ": input must be CUDA bf16");
    TORCH_CHECK(y.dim() >= 1 && y.is_contiguous(),
                op, ": input must be contiguous");
    const long H = y.size(-1);
    TORCH_CHECK(H > 0 && H % VEC == 0 && H <= MAX_H,
                op, " supports hidden size % 8 == 0, <= ", MAX_H);
    const long rows = y.numel() / H;
    TORCH_CHECK(rows >= 1 && rows < (1L << 31), op, ": row count out of range");
    if (residual)
        TORCH_CHECK(residual->is_cuda() && residual->dtype() == torch::kBFloat16
                    && residual->is_contiguous()
                    && residual->sizes() == y.sizes(),
                    op, ": residual must be contiguous CUDA bf16 of y's shape");
    if (bias)
        TORCH_CHECK(bias->is_cuda() && bias->dtype() == torch::kBFloat16
                    && bias->is_contiguous() && bias->numel() == H,
                    op, ": bias must be a contiguous CUDA bf16 tensor of H elements");
    for (const torch::Tensor* t : {gamma, beta})
        TORCH_CHECK(!t || (t->is_cuda() && t->numel() == H),
                    op, ": gamma and beta must be CUDA tensors of H elements");
    for (const torch::Tensor* t : {bias, residual, gamma, beta})
        TORCH_CHECK(!t || t->get_device() == y.get_device(),
                    op, ": all arguments must be on the input's device");
}

// One resident wave of workgroups striding over the rows, asked of the
// runtime once per instantiation. The result does not depend on the grid: a
// row never leaves its workgroup.
template <int NC, bool FUSED>
void ln_fwd_run(const void* in0, const void* bias, const void* residual,
                void* x, const float* gamma, const float* beta, void* z,
                float* mean, float* rstd, long rows, int hv, float eps,
                hipStream_t stream) {
    static int resident = 0;
    if (resident == 0) {
        int per_cu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, ln_fwd_kernel<NC, FUSED>, BLOCK, 0);
        TORCH_CHECK(e == hipSuccess && per_cu > 0,
                    "layernorm fwd: occupancy query failed");
        resident = per_cu
            * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    }
    const int grid = (int)std::min<long>(rows, resident);
    hipLaunchKernelGGL((ln_fwd_kernel<NC, FUSED>), dim3(grid), dim3(BLOCK), 0,
        stream,
        reinterpret_cast<const bf16x8*>(in0),
        reinterpret_cast<const bf16x8*>(bias),
        reinterpret_cast<const bf16x8*>(residual),
        reinterpret_cast<bf16x8*>(x),
        reinterpret_cast<const floatx4*>(gamma),
        reinterpret_cast<const floatx4*>(beta),
        reinterpret_cast<bf16x8*>(z), mean, rstd, (int)rows, hv, eps);
}

// {x (undefined unless fused), z, mean, rstd}
template <bool FUSED>
std::vector<torch::Tensor> ln_fwd_launch(
    const torch::Tensor& in0, const torch::Tensor* bias,
    const torch::Tensor* residual, const torch::Tensor& gamma,
    const torch::Tensor& beta, double eps) {
    const long H = in0.size(-1);
    const long rows = in0.numel() / H;
    const int hv = (int)(H / VEC);

    auto z = torch::empty_like(in0);
    torch::Tensor x;
    if (FUSED) x = torch::empty_like(in0);
    auto f32 = in0.options().dtype(torch::kFloat32);
    auto mean = torch::empty({rows}, f32);
    auto rstd = torch::empty({rows}, f32);
    auto gamma_f = gamma.to(torch::kFloat32).contiguous();
    auto beta_f = beta.to(torch::kFloat32).contiguous();

    const void* bp = FUSED ? bias->data_ptr() : nullptr;
    const void* rp = FUSED ? residual->data_ptr() : nullptr;
    void* xp = FUSED ? x.data_ptr() : nullptr;
    #define LN_FWD_RUN(NC)                                                     \
        ln_fwd_run<NC, FUSED>(in0.data_ptr(), bp, rp, xp,                      \
            gamma_f.data_ptr<float>(), beta_f.data_ptr<float>(), z.data_ptr(), \
            mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, hv,          \
            (float)eps, c10::hip::getCurrentHIPStream().stream())
    switch ((hv + BLOCK - 1) / BLOCK) {     // chunks per thread
        case 1: LN_FWD_RUN(1); break;
        case 2: LN_FWD_RUN(2); break;
        case 3: LN_FWD_RUN(3); break;
        default: LN_FWD_RUN(4); break;
    }
    #undef LN_FWD_RUN
    HIP_CHECK_LAST();
    return {x, z, mean, rstd};
}

// Backward: norm_bwd.h (streaming kernel shared with rmsnorm.hip).
// ADD: g = dres + dx instead of dx, and optionally the column sums of g.
template <bool ADD>
std::vector<torch::Tensor> ln_bwd_launch(
    const torch::Tensor& dy, const torch::Tensor* dres, const torch::Tensor& x,
    const torch::Tensor& gamma, const torch::Tensor& mean,
    const torch::Tensor& rstd, bool want_colsum) {
    auto dyc = dy.contiguous();
    const long H = x.size(-1);
    const long rows = x.numel() / H;

    auto dx = torch::empty_like(x);
    auto f32 = x.options().dtype(torch::kFloat32);
    auto gamma_f = gamma.to(torch::kFloat32).contiguous();
    // one grid for both kernels: dgamma and dbeta of layernorm_bwd_add are
    // the bits of layernorm_bwd (same rows in the same slabs)
    const int grid = norm_bwd::grid_for<false>(rows, H);
    const int nsl = ADD ? 3 : 2;                     // dgamma, dbeta, colsum
    auto part = torch::empty({nsl, grid, H}, f32);
    float* dgamma_part = part.data_ptr<float>();
    float* dbeta_part = dgamma_part + (long)grid * H;
    float* colsum_part = ADD ? dbeta_part + (long)grid * H : nullptr;

    auto stream = c10::hip::getCurrentHIPStream().stream();
    norm_bwd::launch_main<false, ADD>(
        dyc.data_ptr(), x.data_ptr(), gamma_f.data_ptr<float>(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr(),
        dgamma_part, dbeta_part, rows, H, grid, stream,
        ADD ? dres->data_ptr() : nullptr, colsum_part);
    HIP_CHECK_LAST();

    auto dgamma = torch::empty({H}, f32);
    auto dbeta = torch::empty({H}, f32);
    auto colsum = torch::empty({ADD && want_colsum ? H : 0}, f32);
    if (ADD && want_colsum)
        norm_bwd::launch_reduce<false, true>(
            dgamma_part, dbeta_part, dgamma.data_ptr<float>(),
            dbeta.data_ptr<float>(), grid, (int)H, stream,
            colsum_part, colsum.data_ptr<float>());
    else
        norm_bwd::launch_reduce<false>(
            dgamma_part, dbeta_part, dgamma.data_ptr<float>(),
            dbeta.data_ptr<float>(), grid, (int)H, stream);
    HIP_CHECK_LAST();
    if (ADD) return {dx, dgamma, dbeta, colsum};
    return {dx, dgamma, dbeta};
}

}  // namespace

std::vector<torch::Tensor> layernorm_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta, double eps) {
    check_fwd_args(x, nullptr, nullptr, &gamma, &beta, "layernorm fwd");
    auto out = ln_fwd_launch<false>(x, nullptr, nullptr, gamma, beta, eps);
    return {out[1], out[2], out[3]};
}

// x = bf16(residual + bf16(y + bias)); z, mean, rstd = LayerNorm(x).
std::vector<torch::Tensor> bias_residual_layernorm_fwd(
    torch::Tensor y, torch::Tensor bias, torch::Tensor residual,
    torch::Tensor gamma, torch::Tensor beta, double eps) {
    check_fwd_args(y, &bias, &residual, &gamma, &beta,
                   "bias_residual_layernorm fwd");
    return ln_fwd_launch<true>(y, &bias, &residual, gamma, beta, eps);
}

// x = bf16(residual + bf16(y + bias)).
torch::Tensor bias_residual_add(
    torch::Tensor y, torch::Tensor bias, torch::Tensor residual) {
    check_fwd_args(y, &bias, &residual, nullptr, nullptr, "bias_residual_add");
    const long H = y.size(-1);
    const long n = y.numel() / VEC;
    auto x = torch::empty_like(y);
    const int grid = (int)std::min<long>((n + BLOCK - 1) / BLOCK, 1L << 20);
    hipLaunchKernelGGL(
        bias_residual_add_kernel, dim3(grid), dim3(BLOCK), 0,
        c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(y.data_ptr()),
        reinterpret_cast<const bf16x8*>(bias.data_ptr()),
        reinterpret_cast<const bf16x8*>(residual.data_ptr()),
        reinterpret_cast<bf16x8*>(x.data_ptr()), n, (int)(H / VEC));
    HIP_CHECK_LAST();
    return x;
}

std::vector<torch::Tensor> layernorm_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd) {
    norm_bwd::check_args(dy, x, gamma, &mean, rstd, 8192, "layernorm bwd");
    return ln_bwd_launch<false>(dy, nullptr, x, gamma, mean, rstd, false);
}

// g = bf16(dres + bf16(dx)) with dx, dgamma, dbeta of layernorm_bwd, and
// colsum = sum over rows of g (fp32 [H]; empty unless want_colsum).
std::vector<torch::Tensor> layernorm_bwd_add(
    torch::Tensor dy, torch::Tensor dres, torch::Tensor x, torch::Tensor gamma,
    torch::Tensor mean, torch::Tensor rstd, bool want_colsum) {
    norm_bwd::check_args(dy, x, gamma, &mean, rstd, 8192, "layernorm bwd add");
    TORCH_CHECK(dres.is_cuda() && dres.dtype() == torch::kBFloat16
                && dres.is_contiguous() && dres.dim() >= 1
                && dres.size(-1) == x.size(-1) && dres.numel() == x.numel()
                && dres.get_device() == x.get_device(),
                "layernorm bwd add: dres must be contiguous CUDA bf16 with "
                "x's row length and row count, on x's device");
    return ln_bwd_launch<true>(dy, &dres, x, gamma, mean, rstd, want_colsum);
}
