// GeLU (tanh approximation) backward with the bias gradient of the linear
// layer in front of it, for gfx950 (bf16 I/O, fp32 math).
//
//   dh    = da * gelu'(h)            one rounding to bf16
//   dbias = sum over rows of the rounded dh, fp32
//
// The column sum of dh is the gradient of the bias that produced h. As a
// kernel of its own it reads dh again (671 MB at 32768 x 10240); here it
// comes from the registers that hold dh anyway. Layout as in norm_bwd.h: a
// thread owns one 16-byte column chunk and walks rows with R independent
// loads of h and da in flight; a workgroup covers a strip of 256 chunks and
// the row groups blockIdx.y, blockIdx.y + gridDim.y, ...; each row range
// leaves one fp32 slab, and norm_bwd_reduce_kernel adds the slabs in its
// fixed order. Threads never exchange anything, so there is no barrier and
// no LDS; deterministic, no atomics.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

#include "common.h"
#include "norm_bwd.h"

namespace {

constexpr int VEC = 8;
constexpr int BLOCK = 256;     // column chunks per strip
constexpr int R = 4;           // rows in flight per thread
constexpr int MAX_SLABS = 1024;

// d/dh [0.5 h (1 + tanh(u))], u = sqrt(2/pi) (h + 0.044715 h^3), as
//   0.5 (1 + t) + 0.5 h (1 - t^2) u'.
// With e = exp(-2|u|): t = sign(u) (1 - e) / (1 + e) and
// 1 - t^2 = 4 e / (1 + e)^2, which has no cancellation at large |u| and
// needs one exp and one reciprocal. h = 0 gives exactly 0.5; e underflows
// to 0 for large |h|, giving exactly 1 and 0.
__device__ __forceinline__ float gelu_tanh_grad(float h) {
    constexpr float kBeta = 0.7978845608028654f;     // sqrt(2/pi)
    constexpr float kKappa = 0.044715f;
    const float h2 = h * h;
    const float u = kBeta * (h + kKappa * h2 * h);
    const float e = __expf(-2.f * fabsf(u));
    const float r = __builtin_amdgcn_rcpf(1.f + e);   // 1 + e in [1, 2]
    const float t = copysignf((1.f - e) * r, u);
    const float sech2 = 4.f * e * r * r;
    const float du = kBeta * (1.f + 3.f * kKappa * h2);
    return 0.5f * (1.f + t) + 0.5f * h * sech2 * du;
}

__global__ void __launch_bounds__(BLOCK) gelu_bwd_bgrad_kernel(
    const bf16x8* __restrict__ h,
    const bf16x8* __restrict__ da,
    bf16x8* __restrict__ dh,
    float* __restrict__ part,     // [gridDim.y, N]
    int rows,
    int nv) {                     // N / VEC
    const int ci = blockIdx.x * BLOCK + threadIdx.x;
    if (ci >= nv) return;         // no barrier below

    float acc[VEC];
    #pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    for (long r0 = (long)blockIdx.y * R; r0 < rows; r0 += (long)gridDim.y * R) {
        bf16x8 hv[R], av[R];
        #pragma unroll
        for (int r = 0; r < R; ++r) {
            // rows past the end re-read the last row and are dropped below
            const long row = (r0 + r < rows) ? r0 + r : (long)rows - 1;
            hv[r] = h[row * nv + ci];
            av[r] = da[row * nv + ci];
        }
        #pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool ok = r0 + r < rows;
            bf16x8 o;
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float v = bf16_bits_to_float(av[r][k])
                    * gelu_tanh_grad(bf16_bits_to_float(hv[r][k]));
                o[k] = float_to_bf16_bits(v);
                acc[k] += ok ? bf16_bits_to_float(o[k]) : 0.f;
            }
            if (ok) dh[(r0 + r) * nv + ci] = o;
        }
    }

    floatx4* pp = reinterpret_cast<floatx4*>(part);
    const long base = ((long)blockIdx.y * nv + ci) * 2;
    pp[base] = floatx4{acc[0], acc[1], acc[2], acc[3]};
    pp[base + 1] = floatx4{acc[4], acc[5], acc[6], acc[7]};
}

// Row ranges (= slabs): about one resident wave of the chip divided among
// the column strips, capped by the row groups there are.
int row_ranges(long rows, int strips) {
    static int resident = 0;
    if (resident == 0) {
        int per_cu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, gelu_bwd_bgrad_kernel, BLOCK, 0);
        TORCH_CHECK(e == hipSuccess && per_cu > 0,
                    "gelu bwd: occupancy query failed");
        resident = per_cu
            * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    }
    const long want = std::max(1, resident / strips);
    return (int)std::min<long>(std::min<long>(want, MAX_SLABS), (rows + R - 1) / R);
}

}  // namespace

// (dh bf16 like h, dbias fp32 [N]) for h, da [rows, N] bf16, N % 8 == 0.
std::vector<torch::Tensor> gelu_tanh_bwd_bgrad(torch::Tensor h, torch::Tensor da) {
    TORCH_CHECK(h.is_cuda() && h.dtype() == torch::kBFloat16,
                "gelu bwd: h must be CUDA bf16");
    TORCH_CHECK(da.is_cuda() && da.dtype() == torch::kBFloat16,
                "gelu bwd: da must be CUDA bf16");
    TORCH_CHECK(h.dim() >= 1 && h.is_contiguous() && da.is_contiguous(),
                "gelu bwd: h and da must be contiguous");
    TORCH_CHECK(da.sizes() == h.sizes() && da.get_device() == h.get_device(),
                "gelu bwd: da must have h's shape and device");
    const long N = h.size(-1);
    TORCH_CHECK(N > 0 && N % VEC == 0 && N / VEC < (1L << 31) - BLOCK,
                "gelu bwd supports a last dimension % 8 == 0");
    const long rows = h.numel() / N;
    TORCH_CHECK(rows >= 1 && rows < (1L << 31), "gelu bwd: row count out of range");

    const int nv = (int)(N / VEC);
    const int strips = (nv + BLOCK - 1) / BLOCK;
    const int ranges = row_ranges(rows, strips);
    auto dh = torch::empty_like(h);
    auto f32 = h.options().dtype(torch::kFloat32);
    auto part = torch::empty({ranges, N}, f32);
    auto dbias = torch::empty({N}, f32);

    auto stream = c10::hip::getCurrentHIPStream().stream();
    hipLaunchKernelGGL(gelu_bwd_bgrad_kernel, dim3(strips, ranges), dim3(BLOCK),
        0, stream,
        reinterpret_cast<const bf16x8*>(h.data_ptr()),
        reinterpret_cast<const bf16x8*>(da.data_ptr()),
        reinterpret_cast<bf16x8*>(dh.data_ptr()), part.data_ptr<float>(),
        (int)rows, nv);
    HIP_CHECK_LAST();
    norm_bwd::launch_reduce<true>(
        part.data_ptr<float>(), nullptr, dbias.data_ptr<float>(), nullptr,
        ranges, (int)N, stream);
    HIP_CHECK_LAST();
    return {dh, dbias};
}
