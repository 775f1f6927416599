// Ragged split-S single-query (decode) attention for gfx950 — the
// continuous-batching hot loop.
//
// Shape: q [B, H, 1, D] against a padded cache K/V [B, Hkv, S, D] whose
// row b is valid only for positions 0 .. min(kv_lens[b], S) - 1. The
// cache may be a strided view (rows contiguous, batch/head strides
// passed in) so the ragged cache's kbuf[:, :, :upto] is read in place.
//
// Pass 1 (attn_decode_ragged_kernel): one 256-thread workgroup per
// (split, kv head, batch row). The sequence is cut into num_splits
// chunks of ceil(S / num_splits) rows, independent of the lengths. The
// workgroup serves all G = H / Hkv query heads of its kv head, so each
// K/V row is fetched once per group. Rows go straight to VGPRs with
// 16-byte loads: a group of LPR lanes owns one row (8 lanes at D=64, 16
// at D=80/96/128 with the surplus lanes' loads predicated off), so one
// wave-instruction fetches 64/LPR consecutive rows and the dot product
// reduces inside the group with DPP row reads. Every lane group carries
// its own fp32 online-softmax state (m, l, acc) per query head, rescaled
// once per UNROLL rows; groups merge by shuffle, waves merge through
// LDS, and the workgroup writes one fp32 partial per (b, h, split) — or
// bf16 output directly when num_splits == 1.
//
// Pass 2 (attn_decode_combine_kernel): merges the partials per (b, h).
// Two plain launches on the stream, no atomics and no inter-workgroup
// hand-off, so the result is bitwise reproducible.
//
// Empty state is (m = -1e30, l = 0, acc = 0) as in decode.hip: its merge
// weight exp(m - gm) is 0 (or multiplies zeros), never inf - inf.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "attn_host.h"
#include "decode_ragged_common.h"

namespace {

constexpr int UNROLL = 4;          // rows in flight per lane group

template <int D, int G>
__global__ __launch_bounds__(THREADS) void attn_decode_ragged_kernel(
    const short* __restrict__ Q,        // [B, H, D]
    const short* __restrict__ K,        // [B, Hkv, S, D] view, row stride D
    const short* __restrict__ V,
    const int* __restrict__ kv_lens,    // [B]
    short* __restrict__ Out,            // [B, H, D] (num_splits == 1)
    float* __restrict__ ws_acc,         // [B, H, num_splits, D]
    float* __restrict__ ws_ml,          // [B, H, num_splits, 2]
    int H, int S, int chunk, int num_splits,
    long k_sb, long k_sh, long v_sb, long v_sh, float scale) {
    constexpr int LPR = D == 64 ? 8 : 16;     // lanes per K/V row
    constexpr int RPW = WAVE_SIZE / LPR;      // rows per wave-instruction
    constexpr int ROWS_WG = NWAVE * RPW;

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

    const short* kbase = K + (long)b * k_sb + (long)kvh * k_sh + d0;
    const short* vbase = V + (long)b * v_sb + (long)kvh * v_sh + d0;

    for (int base = begin; base < end; base += ROWS_WG * UNROLL) {
        // A row past `end` re-reads row end-1 (valid, in bounds) and gets
        // weight 0 below: padding is never loaded, and no branch diverges.
        bool valid[UNROLL];
        bf16x8 kraw[UNROLL], vraw[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int row = base + u * ROWS_WG + wave * RPW + grp;
            valid[u] = row < end;
            const long ro = (long)min(row, end - 1) * D;
            kraw[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            vraw[u] = kraw[u];
            if (act) {
                kraw[u] = *reinterpret_cast<const bf16x8*>(kbase + ro);
                vraw[u] = *reinterpret_cast<const bf16x8*>(vbase + ro);
            }
        }
        float kf[UNROLL][8], vf[UNROLL][8];
        #pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            unpack8(kraw[u], kf[u]);
            unpack8(vraw[u], vf[u]);
        }

        #pragma unroll
        for (int g = 0; g < G; ++g) {
            float s[UNROLL];
            float m_new = m[g];
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                // even/odd partial sums: packed fp32 FMAs
                float de = 0.f, dod = 0.f;
                #pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    de += qf[g][j] * kf[u][j];
                    dod += qf[g][j + 1] * kf[u][j + 1];
                }
                const float dot = group_sum<LPR>(de + dod);
                s[u] = valid[u] ? dot : NEG_BIG;
                m_new = fmaxf(m_new, s[u]);
            }
            // one rescale of the accumulator per UNROLL rows
            const float alpha = __expf(m[g] - m_new);
            float lsum = l[g] * alpha;
            #pragma unroll
            for (int j = 0; j < 8; ++j) acc[g][j] *= alpha;
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const float p = valid[u] ? __expf(s[u] - m_new) : 0.f;
                lsum += p;
                #pragma unroll
                for (int j = 0; j < 8; ++j) acc[g][j] += p * vf[u][j];
            }
            l[g] = lsum;
            m[g] = m_new;
        }
    }

    // merge the lane groups of a wave (butterfly over the group index)
    #pragma unroll
    for (int off = LPR; off < WAVE_SIZE; off <<= 1) {
        #pragma unroll
        for (int g = 0; g < G; ++g) {
            const float m_o = __shfl_xor(m[g], off, WAVE_SIZE);
            const float l_o = __shfl_xor(l[g], off, WAVE_SIZE);
            const float m_n = fmaxf(m[g], m_o);
            const float a = __expf(m[g] - m_n), bb = __expf(m_o - m_n);
            l[g] = l[g] * a + l_o * bb;
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float acc_o = __shfl_xor(acc[g][j], off, WAVE_SIZE);
                acc[g][j] = acc[g][j] * a + acc_o * bb;
            }
            m[g] = m_n;
        }
    }

    // merge the 4 wave-partials through LDS
    __shared__ float sm[NWAVE][G], sl[NWAVE][G];
    __shared__ float sacc[NWAVE][G][D];
    if (grp == 0 && act) {
        #pragma unroll
        for (int g = 0; g < G; ++g) {
            #pragma unroll
            for (int j = 0; j < 8; ++j) sacc[wave][g][d0 + j] = acc[g][j];
        }
    }
    if (lane == 0) {
        #pragma unroll
        for (int g = 0; g < G; ++g) { sm[wave][g] = m[g]; sl[wave][g] = l[g]; }
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < G * D; idx += THREADS) {
        const int g = idx / D, d = idx % D;
        float gm = NEG_BIG;
        #pragma unroll
        for (int w = 0; w < NWAVE; ++w) gm = fmaxf(gm, sm[w][g]);
        float gl = 0.f, ga = 0.f;
        #pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            const float aw = __expf(sm[w][g] - gm);
            gl += sl[w][g] * aw;
            ga += sacc[w][g][d] * aw;
        }
        const long bh = (long)b * H + kvh * G + g;
        if (num_splits == 1) {
            Out[bh * D + d] = float_to_bf16_bits(gl > 0.f ? ga / gl : 0.f);
        } else {
            const long slot = bh * num_splits + split;
            ws_acc[slot * D + d] = ga;
            if (d == 0) { ws_ml[slot * 2] = gm; ws_ml[slot * 2 + 1] = gl; }
        }
    }
}

// Rows contiguous, 16-byte aligned base and batch/head strides: the
// kernel can read the view in place.
bool readable_in_place(const torch::Tensor& t, long D) {
    return t.stride(3) == 1 && t.stride(2) == D
        && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0
        && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

torch::Tensor attn_decode_ragged(torch::Tensor q, torch::Tensor k,
                                 torch::Tensor v, torch::Tensor kv_lens,
                                 double scale, long num_splits) {
    TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16);
    TORCH_CHECK(k.is_cuda() && k.dtype() == torch::kBFloat16);
    TORCH_CHECK(v.is_cuda() && v.dtype() == torch::kBFloat16);
    TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, "q must be [B, H, 1, D]");
    TORCH_CHECK(k.dim() == 4 && v.dim() == 4, "k/v must be [B, Hkv, S, D]");
    const long B = q.size(0), H = q.size(1), D = q.size(3);
    const long Hkv = k.size(1), S = k.size(2);
    TORCH_CHECK(k.size(0) == B && k.size(3) == D && v.sizes() == k.sizes(),
                "k/v shape mismatch");
    TORCH_CHECK(Hkv > 0 && H % Hkv == 0, "H must be a multiple of Hkv");
    TORCH_CHECK(kv_lens.is_cuda() && kv_lens.dtype() == torch::kInt32
                && kv_lens.dim() == 1 && kv_lens.size(0) == B,
                "kv_lens must be int32 [B] on the device");
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
    auto kc = readable_in_place(k, D) ? k : k.contiguous();
    auto vc = readable_in_place(v, D) ? v : v.contiguous();
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
                (attn_decode_ragged_kernel<decltype(d)::value, decltype(g)::value>),
                grid, dim3(THREADS), 0, stream,
                reinterpret_cast<const short*>(qc.data_ptr()),
                reinterpret_cast<const short*>(kc.data_ptr()),
                reinterpret_cast<const short*>(vc.data_ptr()),
                lens.data_ptr<int>(),
                reinterpret_cast<short*>(out.data_ptr()), acc_p, ml_p,
                (int)H, (int)S, chunk, ns,
                (long)kc.stride(0), (long)kc.stride(1),
                (long)vc.stride(0), (long)vc.stride(1), (float)scale);
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
