// fp8 weight-only decode linear for gfx950: y = scale * (x @ W8^T) + bias
// with x bf16 [M, K], 1 <= M <= 16, and W8 OCP e4m3fn [N, K] quantised
// once per output channel. At M <= 16 the layer is a weight stream; fp8
// weights halve the bytes of the bf16 stream.
//
// Pass 1 (w8_linear_kernel): one 256-thread workgroup per (64 output rows,
// K split). Wave w owns rows n0 + 16w .. +15 and walks the split's K range
// in chunks of KC = 512. Per chunk every lane issues UNROLL = 8 independent
// 16-byte loads — 16 consecutive k of ITS weight row (row = lane & 15,
// k-group = lane >> 4), so one wave-instruction covers 16 rows x 64 k and
// each weight byte is fetched exactly once — straight into VGPRs and
// consumed only after the chunk's x tile is in LDS. A register decodes
// exactly (v_cvt_pk_f32_fp8, then the high half of each fp32 IS the bf16)
// into two B fragments of v_mfma_f32_16x16x32_bf16; the A fragments are the
// matching k of x from LDS. The k order inside an MFMA step is permuted
// (lane group g holds k = 16g .. 16g+7 in the first MFMA of a register and
// 16g+8 .. 16g+15 in the second) identically on both operands.
//
// x tile: [KC/8][16] units of 8 bf16 (16 B), unit (c, m) = x[m][k0 + 8c ..].
// Staged by all 256 threads with 16-byte loads that cover 8 rows x 128 B per
// wave-instruction (full lines), written so 8 consecutive lanes fill 128
// contiguous LDS bytes, and read back as ds_read_b128 with 16 consecutive
// lanes on 256 contiguous bytes. Rows m >= M and k past the split's end are
// zeros written by the kernel: x is never read past row M-1. Two buffers,
// one barrier per chunk.
//
// The accumulator of column m sees only row m of x, the walk over k depends
// on (N, K, num_splits) alone, and the auto split rule reads N and K only:
// row m of y is bitwise independent of M and of the other rows.
//
// Pass 2 (w8_linear_combine_kernel), num_splits > 1: sums the fp32 partials
// [splits, M, N] in split order and applies scale and bias. Two plain
// launches, no atomics, no hand-off between workgroups: bitwise
// reproducible. Scale and bias are applied once, in fp32, after the K sum.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int NWAVE = THREADS / WAVE_SIZE;
constexpr int ROWS_WG = NWAVE * 16;       // output rows per workgroup
constexpr int UNROLL = 8;                 // 16-byte weight loads in flight per lane
constexpr int KSTEP = 64;                 // k per wave-instruction (4 groups x 16)
constexpr int KC = UNROLL * KSTEP;        // k per staged x chunk
constexpr int XUNITS = KC / 8 * 16;       // 16-byte units per x tile
constexpr int XLOADS = XUNITS / THREADS;  // staging loads per thread
constexpr int COMBINE_THREADS = 256;

typedef unsigned int uintx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn bytes -> 8 bf16, exact: every e4m3 value fits bf16's 8
// significand bits, so the fp32 decode has a zero low half.
__device__ __forceinline__ bf16x8 decode8(unsigned int lo, unsigned int hi) {
    const floatx2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false);
    const floatx2 f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const floatx2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false);
    const floatx2 f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    uintx4 p;
    p[0] = (__float_as_uint(f0[0]) >> 16) | (__float_as_uint(f0[1]) & 0xffff0000u);
    p[1] = (__float_as_uint(f1[0]) >> 16) | (__float_as_uint(f1[1]) & 0xffff0000u);
    p[2] = (__float_as_uint(f2[0]) >> 16) | (__float_as_uint(f2[1]) & 0xffff0000u);
    p[3] = (__float_as_uint(f3[0]) >> 16) | (__float_as_uint(f3[1]) & 0xffff0000u);
    return __builtin_bit_cast(bf16x8, p);
}

__global__ __launch_bounds__(THREADS) void w8_linear_kernel(
    const short* __restrict__ X,            // [M, K] bf16
    const unsigned char* __restrict__ W,    // [N, K] e4m3fn
    const float* __restrict__ scale,        // [N]
    const short* __restrict__ bias,         // [N] bf16 or null
    short* __restrict__ Y,                  // [M, N] (num_splits == 1)
    float* __restrict__ part,               // [num_splits, M, N]
    int M, int N, int K, int kchunk, int num_splits) {
    __shared__ uintx4 xs[2][XUNITS];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int j = lane & 15;                // weight row / x row of the fragments
    const int g = lane >> 4;                // k group
    const int split = blockIdx.y;
    const int n0 = blockIdx.x * ROWS_WG + wave * 16;

    const int kbeg = min(split * kchunk, K);
    const int kend = min(kbeg + kchunk, K);

    // a row past N re-reads row N-1 (in bounds) and is never stored
    const unsigned char* wrow = W + (long)min(n0 + j, N - 1) * K;

    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    for (int k0 = kbeg; k0 < kend; k0 += KC, buf ^= 1) {
        // x tile first: the weight loads behind it stay in flight while
        // the tile is written to LDS (loads retire in issue order)
        uintx4 xr[XLOADS];
        int xu[XLOADS];
        #pragma unroll
        for (int i = 0; i < XLOADS; ++i) {
            const int inst = i * NWAVE + wave;          // wave-instruction index
            const int m = (inst & 1) * 8 + (lane & 7);
            const int c = (inst >> 1) * 8 + (lane >> 3);
            const int k = k0 + c * 8;
            xu[i] = c * 16 + m;
            xr[i] = uintx4{0u, 0u, 0u, 0u};
            if (m < M && k < kend)
                xr[i] = *reinterpret_cast<const uintx4*>(X + (long)m * K + k);
        }

        uintx4 wr[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = k0 + u * KSTEP + g * 16;
            wr[u] = uintx4{0u, 0u, 0u, 0u};
            if (k < kend)
                wr[u] = __builtin_nontemporal_load(
                    reinterpret_cast<const uintx4*>(wrow + k));
        }

        #pragma unroll
        for (int i = 0; i < XLOADS; ++i) xs[buf][xu[i]] = xr[i];
        __syncthreads();

        #pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (k0 + u * KSTEP < kend) {                // wave-uniform
                const int c = u * (KSTEP / 8) + g * 2;
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, xs[buf][c * 16 + j]);
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, xs[buf][(c + 1) * 16 + j]);
                const bf16x8 b0 = decode8(wr[u][0], wr[u][1]);
                const bf16x8 b1 = decode8(wr[u][2], wr[u][3]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc, 0, 0, 0);
            }
        }
        // the next chunk writes the other buffer; this one is rewritten
        // only after the next barrier, which every wave reaches after
        // these reads
    }

    // D: lane holds column n = n0 + j, rows m = 4g + r
    const int n = n0 + j;
    if (n >= N) return;
    if (num_splits == 1) {
        const float s = scale[n];
        const float b = bias ? bf16_bits_to_float(bias[n]) : 0.f;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = g * 4 + r;
            if (m < M) Y[(long)m * N + n] = float_to_bf16_bits(fmaf(acc[r], s, b));
        }
    } else {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = g * 4 + r;
            if (m < M) part[((long)split * M + m) * N + n] = acc[r];
        }
    }
}

// One thread per output element: partials summed in split order.
__global__ __launch_bounds__(COMBINE_THREADS) void w8_linear_combine_kernel(
    const float* __restrict__ part,         // [num_splits, M, N]
    const float* __restrict__ scale, const short* __restrict__ bias,
    short* __restrict__ Y, int MN, int N, int num_splits) {
    const int idx = blockIdx.x * COMBINE_THREADS + threadIdx.x;
    if (idx >= MN) return;
    const int n = idx % N;
    float sum = 0.f;
    for (int s0 = 0; s0 < num_splits; s0 += 8) {    // 8 loads in flight
        float v[8];
        #pragma unroll
        for (int i = 0; i < 8; ++i)
            v[i] = s0 + i < num_splits ? part[(long)(s0 + i) * MN + idx] : 0.f;
        #pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
    }
    const float b = bias ? bf16_bits_to_float(bias[n]) : 0.f;
    Y[idx] = float_to_bf16_bits(fmaf(sum, scale[n], b));
}

// Host-side split from N and K only (never M, no device sync): K is cut
// into KC-deep chunks and every split takes the same whole number of them
// (the last may be short), aiming at about three workgroups per CU with
// at most MAX_SPLITS partials. Tuned on the llama3-1b / llama3-8b linears
// (BENCHMARKS.md, "fp8 weight-only decode"). Returns chunks per split.
long auto_split_chunks(long N, long K) {
    constexpr long TARGET_WG = 3 * 256, MAX_SPLITS = 16;
    const long nb = (N + ROWS_WG - 1) / ROWS_WG;
    const long units = (K + KC - 1) / KC;
    const long want = (TARGET_WG + nb - 1) / nb;
    long per = units / std::min({want, units, MAX_SPLITS});
    if ((units + per - 1) / per > MAX_SPLITS)
        per = (units + MAX_SPLITS - 1) / MAX_SPLITS;
    return per;
}

int auto_num_splits(long N, long K) {
    const long chunk = auto_split_chunks(N, K) * KC;
    return (int)((K + chunk - 1) / chunk);
}

bool aligned16(const torch::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

long w8_linear_auto_splits(long N, long K) {
    TORCH_CHECK(N >= 1 && K >= 16, "N >= 1 and K >= 16 required");
    return auto_num_splits(N, K);
}

torch::Tensor w8_linear(torch::Tensor x, torch::Tensor w8, torch::Tensor scale,
                        c10::optional<torch::Tensor> bias, long num_splits) {
    TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16,
                "x must be a bf16 GPU tensor");
    TORCH_CHECK(w8.is_cuda() && w8.dtype() == torch::kFloat8_e4m3fn,
                "w8 must be a float8_e4m3fn GPU tensor");
    TORCH_CHECK(scale.is_cuda() && scale.dtype() == torch::kFloat32,
                "scale must be an fp32 GPU tensor");
    TORCH_CHECK(x.dim() == 2 && w8.dim() == 2, "x must be [M, K], w8 [N, K]");
    const long M = x.size(0), K = x.size(1), N = w8.size(0);
    TORCH_CHECK(M >= 1 && M <= 16, "M must be in [1, 16], got ", M);
    TORCH_CHECK(w8.size(1) == K, "x and w8 disagree on K");
    TORCH_CHECK(K >= 16 && K % 16 == 0, "K must be a positive multiple of 16");
    TORCH_CHECK(N >= 1 && N < (1L << 24) && K < (1L << 24), "N or K out of range");
    TORCH_CHECK(x.is_contiguous() && w8.is_contiguous(),
                "x and w8 must be contiguous");
    TORCH_CHECK(aligned16(x) && aligned16(w8), "x and w8 must be 16-byte aligned");
    TORCH_CHECK(scale.dim() == 1 && scale.size(0) == N && scale.is_contiguous(),
                "scale must be contiguous fp32 [N]");
    TORCH_CHECK(w8.device() == x.device() && scale.device() == x.device(),
                "tensors must be on one device");
    const short* bias_p = nullptr;
    if (bias.has_value() && bias->defined()) {
        TORCH_CHECK(bias->is_cuda() && bias->dtype() == torch::kBFloat16
                    && bias->dim() == 1 && bias->size(0) == N
                    && bias->is_contiguous() && bias->device() == x.device(),
                    "bias must be contiguous bf16 [N] on x's device");
        bias_p = reinterpret_cast<const short*>(bias->data_ptr());
    }
    TORCH_CHECK(num_splits >= 0 && num_splits <= K / 16,
                "num_splits must be in [0, K/16]");

    const int ns = num_splits > 0 ? (int)num_splits : auto_num_splits(N, K);
    // explicit counts cut K into ceil(K/16 / ns) sixteens; the auto rule
    // cuts it into whole KC-deep chunks
    const int kchunk = num_splits > 0
        ? (int)((K / 16 + ns - 1) / ns) * 16
        : (int)(auto_split_chunks(N, K) * KC);
    auto y = torch::empty({M, N}, x.options());
    torch::Tensor part;
    float* part_p = nullptr;
    if (ns > 1) {
        part = torch::empty({ns, M, N}, x.options().dtype(torch::kFloat32));
        part_p = part.data_ptr<float>();
    }
    auto stream = c10::hip::getCurrentHIPStream().stream();
    const dim3 grid((unsigned)((N + ROWS_WG - 1) / ROWS_WG), (unsigned)ns);
    hipLaunchKernelGGL(w8_linear_kernel, grid, dim3(THREADS), 0, stream,
        reinterpret_cast<const short*>(x.data_ptr()),
        reinterpret_cast<const unsigned char*>(w8.data_ptr()),
        scale.data_ptr<float>(), bias_p,
        reinterpret_cast<short*>(y.data_ptr()), part_p,
        (int)M, (int)N, (int)K, kchunk, ns);
    HIP_CHECK_LAST();
    if (ns > 1) {
        const int MN = (int)(M * N);
        hipLaunchKernelGGL(w8_linear_combine_kernel,
            dim3((unsigned)((MN + COMBINE_THREADS - 1) / COMBINE_THREADS)),
            dim3(COMBINE_THREADS), 0, stream, part_p, scale.data_ptr<float>(),
            bias_p, reinterpret_cast<short*>(y.data_ptr()), MN, (int)N, ns);
        HIP_CHECK_LAST();
    }
    return y;
}
