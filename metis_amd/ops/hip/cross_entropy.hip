// Fused cross entropy over bf16 logits for gfx950.
//
// Replaces logits.float() + torch CE: the [tokens, vocab] fp32 copy is
// never materialized (6.7 GB for the GPT-3 2.7B flagship step at gbs 16).
// Forward: per-row two-pass max / sum-exp streaming the bf16 row
// (vectorized 16 B/lane), emits per-row loss and LSE. Backward: one pass
// writing bf16 dlogits = (softmax - onehot) * grad_scale.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int VEC = 8;

__global__ void ce_fwd_kernel(
    const bf16x8* __restrict__ logits,   // [N, V/8]
    const long* __restrict__ labels,     // [N]
    float* __restrict__ loss,            // [N]
    float* __restrict__ lse,             // [N]
    int rows, int vv) {                  // vv = V / 8
    __shared__ float scratch[BLOCK / WAVE_SIZE];

    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const bf16x8* lrow = logits + (long)row * vv;

        float m = -1e30f;
        for (int i = threadIdx.x; i < vv; i += BLOCK) {
            bf16x8 v = lrow[i];
            #pragma unroll
            for (int k = 0; k < VEC; ++k)
                m = fmaxf(m, bf16_bits_to_float(v[k]));
        }
        // block max via the sum scratch (negate trick not needed: reduce manually)
        m = wave_reduce_max(m);
        const int wv = threadIdx.x / WAVE_SIZE;
        if ((threadIdx.x & 63) == 0) scratch[wv] = m;
        __syncthreads();
        float bm = (threadIdx.x < BLOCK / WAVE_SIZE) ? scratch[threadIdx.x] : -1e30f;
        bm = wave_reduce_max(bm);
        if (threadIdx.x == 0) scratch[0] = bm;
        __syncthreads();
        m = scratch[0];
        __syncthreads();

        float sum = 0.f;
        for (int i = threadIdx.x; i < vv; i += BLOCK) {
            bf16x8 v = lrow[i];
            #pragma unroll
            for (int k = 0; k < VEC; ++k)
                sum += __expf(bf16_bits_to_float(v[k]) - m);
        }
        sum = block_reduce_sum(sum, scratch);

        if (threadIdx.x == 0) {
            // a label outside [0, V) is never dereferenced: lse is written
            // as usual and the row's loss is NaN (loud, no device sync)
            const long tgt = labels[row];
            float tl = __builtin_nanf("");
            if (tgt >= 0 && tgt < (long)vv * VEC)
                tl = bf16_bits_to_float(
                    reinterpret_cast<const short*>(lrow)[tgt]);
            const float ls = __logf(sum);
            lse[row] = m + ls;
            // (m - tl) + log(sum), not lse - tl: m - tl is exact, so a
            // large common offset of the row costs the loss nothing
            loss[row] = (m - tl) + ls;
        }
        __syncthreads();
    }
}

__global__ void ce_bwd_kernel(
    const bf16x8* __restrict__ logits,
    const long* __restrict__ labels,
    const float* __restrict__ lse,
    const float* __restrict__ grad_scale,  // dloss/dmean * 1/N, scalar tensor
    bf16x8* __restrict__ dlogits,
    int rows, int vv) {
    const float gs = *grad_scale;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const bf16x8* lrow = logits + (long)row * vv;
        bf16x8* drow = dlogits + (long)row * vv;
        const float l = lse[row];
        const long tgt = labels[row];
        for (int i = threadIdx.x; i < vv; i += BLOCK) {
            bf16x8 v = lrow[i];
            bf16x8 o;
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float p = __expf(bf16_bits_to_float(v[k]) - l);
                if ((long)i * VEC + k == tgt) p -= 1.f;
                o[k] = float_to_bf16_bits(p * gs);
            }
            drow[i] = o;
        }
    }
}

// --- vocab-parallel building blocks --------------------------------------
// The tp>1 cross entropy keeps its three small all-reduces on the host
// (Megatron flow) but streams the bf16 shard with these row kernels
// instead of materializing a fp32 [T, V/tp] copy; its backward reuses
// ce_bwd_kernel with lse = m_global + log(sumexp_global) and labels
// shifted to the shard (or -1 when another rank owns the target).

__global__ void row_max_kernel(
    const bf16x8* __restrict__ logits, float* __restrict__ out,
    int rows, int vv) {
    __shared__ float scratch[BLOCK / WAVE_SIZE];
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const bf16x8* lrow = logits + (long)row * vv;
        float m = -1e30f;
        for (int i = threadIdx.x; i < vv; i += BLOCK) {
            bf16x8 v = lrow[i];
            #pragma unroll
            for (int k = 0; k < VEC; ++k)
                m = fmaxf(m, bf16_bits_to_float(v[k]));
        }
        m = wave_reduce_max(m);
        const int wv = threadIdx.x / WAVE_SIZE;
        if ((threadIdx.x & 63) == 0) scratch[wv] = m;
        __syncthreads();
        float bm = (threadIdx.x < BLOCK / WAVE_SIZE) ? scratch[threadIdx.x]
                                                     : -1e30f;
        bm = wave_reduce_max(bm);
        if (threadIdx.x == 0) out[row] = bm;
        __syncthreads();
    }
}

__global__ void row_sumexp_kernel(
    const bf16x8* __restrict__ logits, const float* __restrict__ m,
    float* __restrict__ out, int rows, int vv) {
    __shared__ float scratch[BLOCK / WAVE_SIZE];
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const bf16x8* lrow = logits + (long)row * vv;
        const float mr = m[row];
        float sum = 0.f;
        for (int i = threadIdx.x; i < vv; i += BLOCK) {
            bf16x8 v = lrow[i];
            #pragma unroll
            for (int k = 0; k < VEC; ++k)
                sum += __expf(bf16_bits_to_float(v[k]) - mr);
        }
        sum = block_reduce_sum(sum, scratch);
        if (threadIdx.x == 0) out[row] = sum;
        __syncthreads();
    }
}

}  // namespace

torch::Tensor ce_row_max(torch::Tensor logits) {
    TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kBFloat16);
    TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0);
    auto lc = logits.contiguous();
    const long N = logits.size(0), V = logits.size(1);
    auto out = torch::empty({N}, logits.options().dtype(torch::kFloat32));
    const int grid = (int)std::min<long>(N, 2048);
    hipLaunchKernelGGL(row_max_kernel, dim3(grid), dim3(BLOCK), 0,
        c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(lc.data_ptr()),
        out.data_ptr<float>(), (int)N, (int)(V / 8));
    HIP_CHECK_LAST();
    return out;
}

torch::Tensor ce_row_sumexp(torch::Tensor logits, torch::Tensor m) {
    TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kBFloat16);
    auto lc = logits.contiguous();
    const long N = logits.size(0), V = logits.size(1);
    TORCH_CHECK(m.size(0) == N && m.dtype() == torch::kFloat32);
    auto out = torch::empty({N}, logits.options().dtype(torch::kFloat32));
    const int grid = (int)std::min<long>(N, 2048);
    hipLaunchKernelGGL(row_sumexp_kernel, dim3(grid), dim3(BLOCK), 0,
        c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(lc.data_ptr()),
        m.contiguous().data_ptr<float>(),
        out.data_ptr<float>(), (int)N, (int)(V / 8));
    HIP_CHECK_LAST();
    return out;
}

std::vector<torch::Tensor> cross_entropy_fwd(
    torch::Tensor logits, torch::Tensor labels) {
    TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kBFloat16);
    TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0,
                "logits must be [N, V] with V % 8 == 0");
    const long N = logits.size(0), V = logits.size(1);
    TORCH_CHECK(labels.is_cuda() && labels.dtype() == torch::kInt64
                && labels.numel() == N, "labels must be CUDA int64 [N]");
    auto lc = logits.contiguous();

    auto f32 = logits.options().dtype(torch::kFloat32);
    auto loss = torch::empty({N}, f32);
    auto lse = torch::empty({N}, f32);
    const int grid = (int)std::min<long>(N, 2048);
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(grid), dim3(BLOCK), 0,
        c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(lc.data_ptr()),
        labels.contiguous().data_ptr<long>(),
        loss.data_ptr<float>(), lse.data_ptr<float>(),
        (int)N, (int)(V / 8));
    HIP_CHECK_LAST();
    return {loss, lse};
}

torch::Tensor cross_entropy_bwd(
    torch::Tensor logits, torch::Tensor labels, torch::Tensor lse,
    torch::Tensor grad_scale) {
    TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kBFloat16,
                "logits must be CUDA bf16");
    TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0,
                "logits must be [N, V] with V % 8 == 0");
    const long N = logits.size(0), V = logits.size(1);
    TORCH_CHECK(labels.is_cuda() && labels.dtype() == torch::kInt64
                && labels.numel() == N, "labels must be CUDA int64 [N]");
    TORCH_CHECK(lse.is_cuda() && lse.dtype() == torch::kFloat32
                && lse.numel() == N && lse.is_contiguous(),
                "lse must be contiguous CUDA fp32 [N]");
    TORCH_CHECK(grad_scale.is_cuda() && grad_scale.dtype() == torch::kFloat32
                && grad_scale.numel() == 1,
                "grad_scale must be a CUDA fp32 scalar tensor");
    auto lc = logits.contiguous();
    auto dlogits = torch::empty_like(lc);
    const int grid = (int)std::min<long>(N, 2048);
    hipLaunchKernelGGL(ce_bwd_kernel, dim3(grid), dim3(BLOCK), 0,
        c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const bf16x8*>(lc.data_ptr()),
        labels.contiguous().data_ptr<long>(),
        lse.data_ptr<float>(),
        grad_scale.contiguous().data_ptr<float>(),
        reinterpret_cast<bf16x8*>(dlogits.data_ptr()),
        (int)N, (int)(V / 8));
    HIP_CHECK_LAST();
    return dlogits;
}
