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

// One operand of the packed attention entry points: a contiguous bf16
// [B, S, width] on the GPU whose base the kernels' 16-B loads can take.
inline void check_attn_packed_operand(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16,
                name, " must be CUDA bf16");
    TORCH_CHECK(t.dim() == 3, name, " must be [B, S, heads * D]");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                name, " must be 16-byte aligned");
}

// Packed mode: qkv [B, S, (H + 2 Hkv) * D], column blocks
// [q heads | k heads | v heads] as qkv_split_transpose defines them. The
// kernels address rows at a pitch of the full width, so the width, S and D
// are pinned here; H == Hkv only (GQA keeps the [B, H, S, D] path, whose
// per-q-head dK/dV the wrapper reduces).
inline AttnDims check_attn_packed_qkv(const torch::Tensor& qkv, long H, long Hkv,
                                      long D) {
    check_attn_packed_operand(qkv, "qkv");
    check_head_dim(D);
    TORCH_CHECK(H > 0 && H == Hkv,
                "packed attention needs H == Hkv > 0, got H=", H, " Hkv=", Hkv);
    TORCH_CHECK(qkv.size(2) == (H + 2 * Hkv) * D,
                "qkv width must be (H + 2 * Hkv) * D");
    const AttnDims d{qkv.size(0), H, Hkv, qkv.size(1), D};
    TORCH_CHECK(d.B > 0 && d.S > 0 && d.S % ATTN_SEQ_TILE == 0,
                "sequence length must be a positive multiple of 128");
    // the kernels keep 128 * pitch in an int (attn_tile.h TileStage)
    TORCH_CHECK(d.B * d.H * d.S < (1L << 31) && qkv.size(2) < (1L << 24),
                "B * H * S must fit an int and the row pitch be below 2^24");
    return d;
}

// o or d_o of the packed mode: [B, S, H * D] on `like`'s device.
inline void check_attn_packed_out(const torch::Tensor& t, const char* name,
                                  const torch::Tensor& like, long B, long S,
                                  long H, long D) {
    check_attn_packed_operand(t, name);
    TORCH_CHECK(t.get_device() == like.get_device(),
                name, " must be on the same device as the other arguments");
    TORCH_CHECK(t.size(0) == B && t.size(1) == S && t.size(2) == H * D,
                name, " must be [B, S, H * D]");
}

// The dKV kernel reads lse and delta four rows (one float4) at a time.
inline void check_attn_rows_aligned(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                name, " must be 16-byte aligned");
}

// lse or delta: fp32 [B, H, S], contiguous, on `like`'s device.
inline void check_attn_rows(const torch::Tensor& t, const char* name,
                            const torch::Tensor& like, long B, long H, long S) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32,
                name, " must be CUDA fp32");
    TORCH_CHECK(t.get_device() == like.get_device(),
                name, " must be on the same device as the other arguments");
    TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(1) == H
                && t.size(2) == S && t.is_contiguous(),
                name, " must be a contiguous [B, H, S]");
    check_attn_rows_aligned(t, name);
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
