// Host-side argument checks and head-dim dispatch shared by the attention
// launchers (attention.hip, attention_bwd.hip, decode.hip,
// decode_ragged.hip).
#pragma once

#include <torch/extension.h>

#include <type_traits>

#include "common.h"

struct AttnDims { long B, H, Hkv, S, D; };   // S = kv length

// q rows per block of attn_fwd (QBLK) and attn_bwd (RBLK); S must divide
constexpr int ATTN_SEQ_TILE = 128;

// q [B, H, Sq, D] against k/v [B, Hkv, S, D], all bf16 on q's device. Every
// size a kernel derives an address from is pinned: a k or v smaller than q
// implies would be read out of bounds. Sq is 1 for decode, else S.
inline AttnDims check_attn_qkv(const torch::Tensor& q, const torch::Tensor& k,
                               const torch::Tensor& v, bool decode = false) {
    TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16, "q must be CUDA bf16");
    TORCH_CHECK(q.dim() == 4, "q must be [B, H, S, D] (S = 1 for decode)");
    TORCH_CHECK(k.is_cuda() && k.dtype() == torch::kBFloat16
                && v.is_cuda() && v.dtype() == torch::kBFloat16,
                "k and v must be CUDA bf16");
    TORCH_CHECK(k.get_device() == q.get_device()
                && v.get_device() == q.get_device(),
                "q, k and v must be on the same device");
    TORCH_CHECK(k.dim() == 4 && v.dim() == 4 && k.sizes() == v.sizes(),
                "k and v must both be [B, Hkv, S, D]");
    const AttnDims d{q.size(0), q.size(1), k.size(1), k.size(2), q.size(3)};
    TORCH_CHECK(k.size(0) == d.B, "k/v batch must match q");
    TORCH_CHECK(k.size(3) == d.D, "k/v head dim must match q");
    TORCH_CHECK(d.Hkv > 0 && d.H % d.Hkv == 0, "GQA requires H % Hkv == 0");
    if (decode) {
        TORCH_CHECK(q.size(2) == 1, "q must be [B, H, 1, D]");
    } else {
        TORCH_CHECK(q.size(2) == d.S, "kv length mismatch");
        TORCH_CHECK(d.S % ATTN_SEQ_TILE == 0, "sequence length must be a multiple of 128");
    }
    return d;
}

// The head dims the kernels are instantiated for.
inline void check_head_dim(long D) {
    TORCH_CHECK(D == 64 || D == 80 || D == 96 || D == 128,
                "head dim must be 64/80/96/128, got ", D);
}

// f(std::integral_constant<int, N>{}) with N = D.
template <class F>
void dispatch_head_dim(long D, F&& f) {
    check_head_dim(D);
    switch (D) {
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 80: f(std::integral_constant<int, 80>{}); break;
        case 96: f(std::integral_constant<int, 96>{}); break;
        default: f(std::integral_constant<int, 128>{}); break;
    }
}

inline bf16* bf16_ptr(const torch::Tensor& t) {
    return reinterpret_cast<bf16*>(t.data_ptr());
}
