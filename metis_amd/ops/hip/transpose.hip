// bf16 matrix transpose: wt [C, R] = w [R, C]^T.
//
// Keeps the transposed copy of a linear layer's weight that the data-gradient
// GEMM reads (ops/linear.py): with Wt contiguous, dx = dy @ W is the library's
// TN product, the layout its fastest kernels are written for.
//
// One 256-thread block moves a 64 x 64 tile through LDS. Global traffic is one
// 16-byte load and one 16-byte store per lane and chunk; eight lanes cover a
// 128-byte row segment on both sides. The transposition itself happens in the
// LDS read: a lane gathers the 8 elements of one output chunk from 8 tile
// rows with 2-byte reads.
//
// LDS layout: row r starts at r * 72 + (r / 8) * 8 elements. The pitch of 72
// (64 + one 16-byte access) keeps every row 16-byte aligned for the
// ds_write_b128. In the read a half-wave holds 8 row groups i (rows 8i + j)
// times 4 adjacent columns c; a pitch that is a multiple of 8 elements alone
// would put all 8 groups on one bank (8 rows * 36 dwords = 0 mod 32), so each
// group of 8 rows is shifted by a further 16 bytes: the dword index becomes
// 4 * (i + j) + c / 2 mod 32, distinct over i, and columns c, c + 1 share a
// dword (one address, broadcast).
//
// R and C are multiples of 8, so a 16-byte chunk is either wholly inside the
// matrix or wholly outside; partial tiles at both edges skip the chunks
// outside.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"

namespace {

constexpr int TR_TILE = 64;
constexpr int TR_BLOCK = 256;
constexpr int TR_PITCH = TR_TILE + 8;
constexpr int TR_GROUP_SHIFT = 8;
constexpr int TR_LDS_ELEMS =
    TR_TILE * TR_PITCH + (TR_TILE / 8) * TR_GROUP_SHIFT;
constexpr int TR_CHUNKS = TR_TILE * TR_TILE / 8;  // 16-byte chunks per tile

__device__ __forceinline__ int tr_lds_offset(int r, int c) {
    return r * TR_PITCH + (r >> 3) * TR_GROUP_SHIFT + c;
}

__global__ __launch_bounds__(TR_BLOCK) void transpose_bf16_kernel(
    const short* __restrict__ in, short* __restrict__ out, int R, int C,
    int tiles_c) {
    __shared__ __attribute__((aligned(16))) short tile[TR_LDS_ELEMS];

    const int tile_r = blockIdx.x / tiles_c;
    const int tile_c = blockIdx.x - tile_r * tiles_c;
    const long r_base = (long)tile_r * TR_TILE;
    const long c_base = (long)tile_c * TR_TILE;

    #pragma unroll
    for (int chunk = threadIdx.x; chunk < TR_CHUNKS; chunk += TR_BLOCK) {
        const int r = chunk >> 3, k = chunk & 7;
        const long gr = r_base + r, gc = c_base + k * 8;
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (gr < R && gc < C)
            v = *reinterpret_cast<const bf16x8*>(in + gr * C + gc);
        *reinterpret_cast<bf16x8*>(&tile[tr_lds_offset(r, k * 8)]) = v;
    }
    __syncthreads();

    #pragma unroll
    for (int chunk = threadIdx.x; chunk < TR_CHUNKS; chunk += TR_BLOCK) {
        const int c = chunk >> 3, i = chunk & 7;
        const long gc = c_base + c, gr0 = r_base + i * 8;
        if (gc < C && gr0 < R) {
            bf16x8 v;
            #pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tile[tr_lds_offset(i * 8 + j, c)];
            *reinterpret_cast<bf16x8*>(out + gc * R + gr0) = v;
        }
    }
}

void check_matrix(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t.dtype() == torch::kBFloat16, name, " must be bf16");
    TORCH_CHECK(t.dim() == 2, name, " must be 2-d");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
                " must be 16-byte aligned");
}

}  // namespace

void transpose_bf16_out(torch::Tensor w, torch::Tensor wt) {
    check_matrix(w, "w");
    check_matrix(wt, "wt");
    const long R = w.size(0), C = w.size(1);
    TORCH_CHECK(R > 0 && C > 0 && R % 8 == 0 && C % 8 == 0,
                "transpose_bf16: both sizes must be positive multiples of 8, "
                "got [", R, ", ", C, "]");
    TORCH_CHECK(wt.size(0) == C && wt.size(1) == R, "wt must be [", C, ", ", R,
                "]");
    TORCH_CHECK(w.device() == wt.device(), "w and wt must be on one device");
    TORCH_CHECK(w.data_ptr() != wt.data_ptr(), "w and wt must not alias");
    const long tiles_r = (R + TR_TILE - 1) / TR_TILE;
    const long tiles_c = (C + TR_TILE - 1) / TR_TILE;
    TORCH_CHECK(R <= INT_MAX && C <= INT_MAX && tiles_r * tiles_c <= INT_MAX,
                "transpose_bf16: matrix too large");
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3((unsigned)(tiles_r * tiles_c)),
        dim3(TR_BLOCK), 0, c10::hip::getCurrentHIPStream().stream(),
        reinterpret_cast<const short*>(w.data_ptr()),
        reinterpret_cast<short*>(wt.data_ptr()), (int)R, (int)C, (int)tiles_c);
    HIP_CHECK_LAST();
}

torch::Tensor transpose_bf16(torch::Tensor w) {
    check_matrix(w, "w");
    auto wt = torch::empty({w.size(1), w.size(0)}, w.options());
    transpose_bf16_out(w, wt);
    return wt;
}
