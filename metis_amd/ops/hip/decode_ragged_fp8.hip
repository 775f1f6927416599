// Ragged split-S single-query (decode) attention over an fp8 KV cache for
// gfx950 — decode_ragged.hip with K and V held as OCP e4m3fn bytes plus one
// fp32 scale per (batch row, kv head, position):
//
//   o = softmax_j( scale * ks_j * (q . k8_j) ) . ( vs_j * v8_j )
//
// The format is defined by ops/kv8.py (quantize_kv_e4m3) and written by
// kv_quant.hip. Both row scales are applied in fp32 outside the dot
// products: ks_j multiplies the score, vs_j is folded into the probability
// that weights row j of V. K and V are never rescaled element by element;
// the e4m3 -> fp32 decode (v_cvt_pk_f32_fp8) is exact.
//
// Geometry, split rule, masking, merges and pass 2 are those of
// decode_ragged.hip (decode_ragged_common.h): 8 elements per lane, 8 lanes
// per row at D=64 and 16 at D=80/96/128, one 256-thread workgroup per
// (split, kv head, batch row) serving all G query heads of the kv head. A
// lane's load is 8 bytes here, so twice the rows are kept in flight (8 of
// K and 8 of V per lane group, about 128 B per lane as in the bf16
// kernel); at G=8 the q and accumulator registers leave room for 2. Each
// lane group loads its row's two scales with one 4-byte load each (every
// lane of the group reads the same address). A row past the end re-reads
// the last valid row and its scales and gets weight 0: padding bytes and
// padding scales are never loaded.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"
#include "decode_ragged_common.h"

namespace {

typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef unsigned int uintx2 __attribute__((ext_vector_type(2)));

// Rows in flight per lane group, and rows decoded to fp32 and folded into
// the online softmax per rescale. The decoded rows are the larger register
// cost (16 VGPRs per row of K and V) next to q and acc (16 per query
// head). At G=8 every choice with 4 rows in flight, or 2 rows per rescale,
// compiled to 256 VGPRs plus AGPR copies and one wave per SIMD at D=64 and
// 128; (2, 1) is the largest that keeps two waves per SIMD, the bf16
// kernel's occupancy at G=8.
template <int G>
struct RowsInFlight { static constexpr int value = G == 8 ? 2 : 8; };
template <int G>
struct RowsPerRescale { static constexpr int value = G == 8 ? 1 : 4; };

// 8 e4m3fn bytes -> 8 fp32, exact.
__device__ __forceinline__ void decode8(uintx2 raw, float* f) {
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const floatx2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[i], false);
        const floatx2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[i], true);
        f[4 * i] = lo[0];
        f[4 * i + 1] = lo[1];
        f[4 * i + 2] = hi[0];
        f[4 * i + 3] = hi[1];
    }
}

template <int D, int G>
__global__ __launch_bounds__(THREADS) void attn_decode_ragged_fp8_kernel(
    const short* __restrict__ Q,            // [B, H, D] bf16
    const unsigned char* __restrict__ K8,   // [B, Hkv, S, D] view, row stride D
    const unsigned char* __restrict__ V8,
    const float* __restrict__ KS,           // [B, Hkv, S] view, unit stride
    const float* __restrict__ VS,
    const int* __restrict__ kv_lens,        // [B]
    short* __restrict__ Out,                // [B, H, D] (num_splits == 1)
    float* __restrict__ ws_acc,             // [B, H, num_splits, D]
    float* __restrict__ ws_ml,              // [B, H, num_splits, 2]
    int H, int S, int chunk, int num_splits,
    long k_sb, long k_sh, long v_sb, long v_sh,
    long ks_sb, long ks_sh, long vs_sb, long vs_sh, float scale) {
    constexpr int LPR = RowLanes<D>::value;   // lanes per K/V row
    constexpr int RPW = WAVE_SIZE / LPR;      // rows per wave-instruction
    constexpr int ROWS_WG = NWAVE * RPW;
    constexpr int UNROLL = RowsInFlight<G>::value;
    constexpr int SUB = RowsPerRescale<G>::value;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int d0 = sub * 8;
    const bool act = d0 < D;                  // false: surplus lane (D=80/96)

    const int len = min(max(kv_lens[b], 0), S);
    const int begin = min(split * chunk, len);
    const int end = min(begin + chunk, len);

    // q of the G heads in registers, pre-scaled
    float qf[G][8];
    #pragma unroll
    for (int g = 0; g < G; ++g) {
        #pragma unroll
        for (int j = 0; j < 8; ++j) qf[g][j] = 0.f;
        if (act) {
            const long qo = ((long)b * H + kvh * G + g) * D + d0;
            unpack8(*reinterpret_cast<const bf16x8*>(Q + qo), qf[g]);
            #pragma unroll
            for (int j = 0; j < 8; ++j) qf[g][j] *= scale;
        }
    }

    float m[G], l[G], acc[G][8];
    #pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = NEG_BIG;
        l[g] = 0.f;
        #pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    }

    const unsigned char* kbase = K8 + (long)b * k_sb + (long)kvh * k_sh + d0;
    const unsigned char* vbase = V8 + (long)b * v_sb + (long)kvh * v_sh + d0;
    const float* ksbase = KS + (long)b * ks_sb + (long)kvh * ks_sh;
    const float* vsbase = VS + (long)b * vs_sb + (long)kvh * vs_sh;

    for (int base = begin; base < end; base += ROWS_WG * UNROLL) {
        // A row past `end` re-reads row end-1 (valid, in bounds) and gets
        // weight 0 below: padding is never loaded, and no branch diverges.
        bool valid[UNROLL];
        uintx2 kraw[UNROLL], vraw[UNROLL];
        float ks[UNROLL], vs[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int row = base + u * ROWS_WG + wave * RPW + grp;
            valid[u] = row < end;
            const long r = min(row, end - 1);
            kraw[u] = uintx2{0u, 0u};
            vraw[u] = kraw[u];
            if (act) {
                kraw[u] = *reinterpret_cast<const uintx2*>(kbase + r * D);
                vraw[u] = *reinterpret_cast<const uintx2*>(vbase + r * D);
            }
            ks[u] = ksbase[r];
            vs[u] = vsbase[r];
        }

        #pragma unroll
        for (int h = 0; h < UNROLL; h += SUB) {
            float kf[SUB][8], vf[SUB][8];
            #pragma unroll
            for (int u = 0; u < SUB; ++u) {
                decode8(kraw[h + u], kf[u]);
                decode8(vraw[h + u], vf[u]);
            }

            #pragma unroll
            for (int g = 0; g < G; ++g) {
                float s[SUB];
                float m_new = m[g];
                #pragma unroll
                for (int u = 0; u < SUB; ++u) {
                    // even/odd partial sums: packed fp32 FMAs
                    float de = 0.f, dod = 0.f;
                    #pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        de += qf[g][j] * kf[u][j];
                        dod += qf[g][j + 1] * kf[u][j + 1];
                    }
                    const float dot = group_sum<LPR>(de + dod) * ks[h + u];
                    s[u] = valid[h + u] ? dot : NEG_BIG;
                    m_new = fmaxf(m_new, s[u]);
                }
                // one rescale of the accumulator per SUB rows
                const float alpha = __expf(m[g] - m_new);
                float lsum = l[g] * alpha;
                #pragma unroll
                for (int j = 0; j < 8; ++j) acc[g][j] *= alpha;
                #pragma unroll
                for (int u = 0; u < SUB; ++u) {
                    const float p = valid[h + u] ? __expf(s[u] - m_new) : 0.f;
                    lsum += p;
                    const float pv = p * vs[h + u];
                    #pragma unroll
                    for (int j = 0; j < 8; ++j) acc[g][j] += pv * vf[u][j];
                }
                l[g] = lsum;
                m[g] = m_new;
            }
        }
    }

    merge_and_write<D, G>(m, l, acc, Out, ws_acc, ws_ml, H, num_splits,
                          split, kvh, b);
}

// Rows contiguous, 8-byte aligned base and batch/head strides: the kernel
// can read the view in place (one lane loads 8 bytes of a row).
bool bytes_readable_in_place(const torch::Tensor& t, long D) {
    return t.stride(3) == 1 && t.stride(2) == D
        && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0
        && reinterpret_cast<uintptr_t>(t.data_ptr()) % 8 == 0;
}

void check_row_scale(const torch::Tensor& t, const char* name,
                     const torch::Tensor& like, long B, long Hkv, long S) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32,
                name, " must be CUDA fp32");
    TORCH_CHECK(t.get_device() == like.get_device(),
                name, " must be on the same device as q");
    TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(1) == Hkv
                && t.size(2) == S, name, " must be [B, Hkv, S]");
    TORCH_CHECK(S <= 1 || t.stride(2) == 1,
                name, " must have unit stride along S");
}

}  // namespace

torch::Tensor attn_decode_ragged_fp8(torch::Tensor q, torch::Tensor k8,
                                     torch::Tensor v8, torch::Tensor k_scale,
                                     torch::Tensor v_scale,
                                     torch::Tensor kv_lens, double scale,
                                     long num_splits) {
    TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16,
                "q must be CUDA bf16");
    TORCH_CHECK(k8.is_cuda() && k8.dtype() == torch::kFloat8_e4m3fn
                && v8.is_cuda() && v8.dtype() == torch::kFloat8_e4m3fn,
                "k8 and v8 must be CUDA float8_e4m3fn");
    TORCH_CHECK(k8.get_device() == q.get_device()
                && v8.get_device() == q.get_device(),
                "q, k8 and v8 must be on the same device");
    TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, "q must be [B, H, 1, D]");
    TORCH_CHECK(k8.dim() == 4 && v8.dim() == 4, "k8/v8 must be [B, Hkv, S, D]");
    const long B = q.size(0), H = q.size(1), D = q.size(3);
    const long Hkv = k8.size(1), S = k8.size(2);
    TORCH_CHECK(k8.size(0) == B && k8.size(3) == D && v8.sizes() == k8.sizes(),
                "k8/v8 shape mismatch");
    check_row_scale(k_scale, "k_scale", q, B, Hkv, S);
    check_row_scale(v_scale, "v_scale", q, B, Hkv, S);
    TORCH_CHECK(Hkv > 0 && H % Hkv == 0, "H must be a multiple of Hkv");
    TORCH_CHECK(kv_lens.is_cuda() && kv_lens.dtype() == torch::kInt32
                && kv_lens.dim() == 1 && kv_lens.size(0) == B
                && kv_lens.get_device() == q.get_device(),
                "kv_lens must be int32 [B] on q's device");
    TORCH_CHECK(D == 64 || D == 80 || D == 96 || D == 128,
                "unsupported head dim ", D);
    const long G = H / Hkv;
    TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8,
                "unsupported GQA group size ", G);
    TORCH_CHECK(num_splits >= 0 && num_splits <= 1024,
                "num_splits must be in [0, 1024]");
    TORCH_CHECK(B <= 65535 && Hkv <= 65535, "grid dimension too large");
    TORCH_CHECK(S < (1L << 30), "S too large");

    auto qc = q.contiguous();
    if (reinterpret_cast<uintptr_t>(qc.data_ptr()) % 16 != 0) qc = qc.clone();
    auto lens = kv_lens.contiguous();
    auto kc = bytes_readable_in_place(k8, D) ? k8 : k8.contiguous();
    auto vc = bytes_readable_in_place(v8, D) ? v8 : v8.contiguous();
    auto ksc = S <= 1 ? k_scale.contiguous() : k_scale;
    auto vsc = S <= 1 ? v_scale.contiguous() : v_scale;
    auto out = torch::empty_like(qc);
    if (B == 0 || H == 0) return out;
    if (S == 0) return out.zero_();

    const int ns = num_splits > 0 ? (int)num_splits
                                  : auto_num_splits(B, Hkv, S);
    const int chunk = (int)((S + ns - 1) / ns);
    torch::Tensor ws_acc, ws_ml;
    float *acc_p = nullptr, *ml_p = nullptr;
    if (ns > 1) {
        auto opt = q.options().dtype(torch::kFloat32);
        ws_acc = torch::empty({B, H, ns, D}, opt);
        ws_ml = torch::empty({B, H, ns, 2}, opt);
        acc_p = ws_acc.data_ptr<float>();
        ml_p = ws_ml.data_ptr<float>();
    }
    auto stream = c10::hip::getCurrentHIPStream().stream();
    const dim3 grid(ns, (unsigned)Hkv, (unsigned)B);

    dispatch_head_dim(D, [&](auto d) {
        auto launch = [&](auto g) {
            hipLaunchKernelGGL(
                (attn_decode_ragged_fp8_kernel<decltype(d)::value,
                                               decltype(g)::value>),
                grid, dim3(THREADS), 0, stream,
                reinterpret_cast<const short*>(qc.data_ptr()),
                reinterpret_cast<const unsigned char*>(kc.data_ptr()),
                reinterpret_cast<const unsigned char*>(vc.data_ptr()),
                ksc.data_ptr<float>(), vsc.data_ptr<float>(),
                lens.data_ptr<int>(),
                reinterpret_cast<short*>(out.data_ptr()), acc_p, ml_p,
                (int)H, (int)S, chunk, ns,
                (long)kc.stride(0), (long)kc.stride(1),
                (long)vc.stride(0), (long)vc.stride(1),
                (long)ksc.stride(0), (long)ksc.stride(1),
                (long)vsc.stride(0), (long)vsc.stride(1), (float)scale);
        };
        switch (G) {   // checked above: 1, 2, 4 or 8
            case 1: launch(std::integral_constant<int, 1>{}); break;
            case 2: launch(std::integral_constant<int, 2>{}); break;
            case 4: launch(std::integral_constant<int, 4>{}); break;
            default: launch(std::integral_constant<int, 8>{}); break;
        }
    });
    HIP_CHECK_LAST();

    if (ns > 1) {
        hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)(B * H)),
            dim3(COMBINE_THREADS), 0, stream, acc_p, ml_p,
            reinterpret_cast<short*>(out.data_ptr()), (int)D, ns);
        HIP_CHECK_LAST();
    }
    return out;
}
