// Writer of the fp8 KV cache for gfx950: quantise bf16 K/V rows to OCP
// e4m3fn with one fp32 scale per row of D elements and store them at
// per-source positions of the padded cache, K and V in one launch.
//
//   kv_quant_store(k, v [N, Hkv, T, D] bf16,
//                  k8, v8 [B, Hkv, cap, D] e4m3fn, k_scale, v_scale
//                  [B, Hkv, cap] fp32, slots [N], pos [N])
//
// Row t of source n goes to position pos[n] + t of batch row slots[n]; a
// destination outside [0, cap) (or a slot outside [0, B)) is skipped.
// slots and pos are read on the device: no host sync. The decode append is
// T = 1, N = max_batch; the prefill splice is N = 1, T = prompt length.
//
// The format is DEFINED by ops/kv8.py quantize_kv_e4m3 evaluated by torch
// on the CPU, and this kernel reproduces it bitwise:
//   scale = max(amax, 2^-100) / 448      (IEEE fp32 division)
//   byte  = e4m3fn(rne(clamp(x / scale, -448, 448)))   (IEEE division)
// One lane group per row with the geometry of the decode kernels
// (decode_ragged_common.h): 8 elements per lane as one bf16x8 load, 8
// lanes at D=64 and 16 at D=80/96/128, amax reduced inside the group with
// DPP row reads. Each lane stores its 8 bytes with one 8-byte vector
// store; lane 0 of the group stores the scale.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"
#include "decode_ragged_common.h"

namespace {

typedef unsigned int uintx2 __attribute__((ext_vector_type(2)));

constexpr float E4M3_MAX = 448.f;
constexpr float AMAX_TINY = 0x1p-100f;

template <int D>
__global__ __launch_bounds__(THREADS) void kv_quant_store_kernel(
    const short* __restrict__ K,        // [N, Hkv, T, D], strides in elements
    const short* __restrict__ V,
    unsigned char* __restrict__ K8,     // [B, Hkv, cap, D] contiguous
    unsigned char* __restrict__ V8,
    float* __restrict__ KS,             // [B, Hkv, cap] contiguous
    float* __restrict__ VS,
    const int64_t* __restrict__ slots,  // [N]
    const int64_t* __restrict__ pos,    // [N]
    long rows, int Hkv, int T, int B, int cap,
    long k_sn, long k_sh, long k_st, long v_sn, long v_sh, long v_st) {
    constexpr int LPR = RowLanes<D>::value;
    constexpr int ROWS_WG = THREADS / LPR;

    const int sub = threadIdx.x % LPR;
    const int d0 = sub * 8;
    const bool is_v = blockIdx.y == 1;
    const long row = (long)blockIdx.x * ROWS_WG + threadIdx.x / LPR;
    const bool in = row < rows;           // uniform over the lane group
    const bool act = in && d0 < D;        // false: surplus lane (D=80/96)

    // row -> (n, h, t)
    const long rr = in ? row : 0;
    const int t = (int)(rr % T);
    const int h = (int)((rr / T) % Hkv);
    const long n = rr / ((long)T * Hkv);

    float x[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    if (act) {
        const short* src = is_v ? V + n * v_sn + (long)h * v_sh + (long)t * v_st
                                : K + n * k_sn + (long)h * k_sh + (long)t * k_st;
        unpack8(*reinterpret_cast<const bf16x8*>(src + d0), x);
    }

    float amax = 0.f;
    #pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(x[j]));
    amax = group_max<LPR>(amax);

    const float scale = __fdiv_rn(fmaxf(amax, AMAX_TINY), E4M3_MAX);
    float qv[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j)
        qv[j] = fminf(fmaxf(__fdiv_rn(x[j], scale), -E4M3_MAX), E4M3_MAX);

    uintx2 bytes;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(qv[4 * i], qv[4 * i + 1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(qv[4 * i + 2], qv[4 * i + 3], w, true);
        bytes[i] = (unsigned int)w;
    }

    if (!in) return;
    const long slot = slots[n];
    const long p = pos[n] + t;
    if (slot < 0 || slot >= B || p < 0 || p >= cap) return;
    const long dst = (slot * Hkv + h) * (long)cap + p;
    if (act)
        *reinterpret_cast<uintx2*>((is_v ? V8 : K8) + dst * D + d0) = bytes;
    if (sub == 0) (is_v ? VS : KS)[dst] = scale;
}

// Source K or V: [N, Hkv, T, D] bf16 with contiguous rows whose starts
// are 16-byte aligned.
void check_kv_source(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16,
                name, " must be CUDA bf16");
    TORCH_CHECK(t.dim() == 4, name, " must be [N, Hkv, T, D]");
    TORCH_CHECK(t.size(3) <= 1 || t.stride(3) == 1,
                name, " rows must be contiguous");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0
                && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0
                && t.stride(2) % 8 == 0,
                name, " rows must start 16-byte aligned");
}

void check_index(const torch::Tensor& t, const char* name,
                 const torch::Tensor& like, long N) {
    TORCH_CHECK(t.is_cuda() && (t.dtype() == torch::kInt64
                                || t.dtype() == torch::kInt32),
                name, " must be a CUDA int32 or int64 tensor");
    TORCH_CHECK(t.get_device() == like.get_device(),
                name, " must be on the same device as k");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == N, name, " must be [N]");
}

}  // namespace

void kv_quant_store(torch::Tensor k, torch::Tensor v, torch::Tensor k8,
                    torch::Tensor v8, torch::Tensor k_scale,
                    torch::Tensor v_scale, torch::Tensor slots,
                    torch::Tensor pos) {
    check_kv_source(k, "k");
    check_kv_source(v, "v");
    TORCH_CHECK(k.sizes() == v.sizes(), "k and v must have the same shape");
    const long N = k.size(0), Hkv = k.size(1), T = k.size(2), D = k.size(3);
    TORCH_CHECK(k8.is_cuda() && k8.dtype() == torch::kFloat8_e4m3fn
                && v8.is_cuda() && v8.dtype() == torch::kFloat8_e4m3fn,
                "k8 and v8 must be CUDA float8_e4m3fn");
    TORCH_CHECK(k8.dim() == 4 && k8.sizes() == v8.sizes(),
                "k8 and v8 must both be [B, Hkv, cap, D]");
    const long B = k8.size(0), cap = k8.size(2);
    TORCH_CHECK(k8.size(1) == Hkv, "cache Hkv must match k/v");
    TORCH_CHECK(k8.size(3) == D, "cache head dim must match k/v");
    check_head_dim(D);
    TORCH_CHECK(k8.is_contiguous() && v8.is_contiguous(),
                "k8 and v8 must be contiguous");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(k8.data_ptr()) % 8 == 0
                && reinterpret_cast<uintptr_t>(v8.data_ptr()) % 8 == 0,
                "k8 and v8 must be 8-byte aligned");
    for (const torch::Tensor* s : {&k_scale, &v_scale}) {
        TORCH_CHECK(s->is_cuda() && s->dtype() == torch::kFloat32,
                    "k_scale and v_scale must be CUDA fp32");
        TORCH_CHECK(s->dim() == 3 && s->size(0) == B && s->size(1) == Hkv
                    && s->size(2) == cap && s->is_contiguous(),
                    "k_scale and v_scale must be contiguous [B, Hkv, cap]");
    }
    check_index(slots, "slots", k, N);
    check_index(pos, "pos", k, N);
    const int dev = k.get_device();
    TORCH_CHECK(v.get_device() == dev && k8.get_device() == dev
                && v8.get_device() == dev && k_scale.get_device() == dev
                && v_scale.get_device() == dev,
                "all operands must be on the same device");
    TORCH_CHECK(B < (1L << 31) && cap < (1L << 31) && Hkv < (1L << 31)
                && T < (1L << 31), "dimension too large");

    const long rows = N * Hkv * T;
    if (rows == 0 || B == 0 || cap == 0) return;
    auto sl = slots.to(torch::kInt64).contiguous();
    auto ps = pos.to(torch::kInt64).contiguous();
    auto stream = c10::hip::getCurrentHIPStream().stream();

    dispatch_head_dim(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        constexpr int ROWS_WG = THREADS / RowLanes<DD>::value;
        const long nblk = (rows + ROWS_WG - 1) / ROWS_WG;
        TORCH_CHECK(nblk < (1L << 31), "too many rows");
        hipLaunchKernelGGL(
            (kv_quant_store_kernel<DD>), dim3((unsigned)nblk, 2),
            dim3(THREADS), 0, stream,
            reinterpret_cast<const short*>(k.data_ptr()),
            reinterpret_cast<const short*>(v.data_ptr()),
            reinterpret_cast<unsigned char*>(k8.data_ptr()),
            reinterpret_cast<unsigned char*>(v8.data_ptr()),
            k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
            sl.data_ptr<int64_t>(), ps.data_ptr<int64_t>(),
            rows, (int)Hkv, (int)T, (int)B, (int)cap,
            (long)k.stride(0), (long)k.stride(1), (long)k.stride(2),
            (long)v.stride(0), (long)v.stride(1), (long)v.stride(2));
    });
    HIP_CHECK_LAST();
}
