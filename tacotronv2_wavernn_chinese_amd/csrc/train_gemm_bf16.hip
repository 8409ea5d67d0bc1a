// gemm_bf16_kernel<TA,TB>: the batched GEMM of wrnn_train_step in mixed precision (WRNN_TRAIN_BF16).  The contract is sgemm_kernel's
// (train.hip):  C = (beta) C + A.B (+ bias) (relu), fp32 operands in memory with lda / ldb / ldc, optional split-K over blockIdx.z
// (kper / cslice), edges in M, N and K zero-filled.  The one difference: every operand element is rounded ONCE to bfloat16 (round to
// nearest even, v_cvt_pk_bf16_f32) as it is staged into LDS, and the products run on v_mfma_f32_32x32x16_bf16.  A product of two bf16
// values is exact in fp32, the accumulators are fp32, and bias, the beta input, ReLU and the split-K partials are not rounded.
//
// 128 x 128 x 32 block tile, 4 waves x (2 x 2) MFMA tiles of 32 x 32, two k-steps of 16 per tile step.
// LDS image: both operands k-contiguous per row, [128 rows][32 bf16] with a pitch of BG_LD = 40 bf16 (80 bytes = 20 banks).  The
//   fragment of lane l for k-step s -- A[row l & 31][k = 16 s + 8 (l >> 5) + j], B[k][col l & 31], j = 0..7 -- is one ds_read_b128 at
//   row * 80 + 32 s + 16 (l >> 5).  20 banks = 5 four-bank slots per row and 5 is odd, so the 16 lanes of every ds_read_b128 group
//   (rows distinct mod 16, one k half) land on 16 different slots of the 64 banks: conflict-free.
// Global fetch: register double-buffered fp32, as in sgemm_kernel.  The operands are column blocks of weights and conditioning at
//   arbitrary float offsets with odd leading dimensions (I.weight + 1 with ld 113, aux + A), so every global load is a single dword:
//   nothing here assumes more than 4-byte alignment.
//   operand k-contiguous in memory (A of NN / NT, B of NT): a lane loads the k pair (2c, 2c + 1), c = tid & 15, of rows
//     (tid >> 4) + 16 i, i = 0..7, and stores each pair as one packed dword.
//   operand m-contiguous in memory (A of TN, B of NN / TN): a lane loads k = 16 (tid >> 7) + 0..15 of row tid & 127 (every load
//     coalesced over the rows) and stores them as two 16-byte writes -- the transposing stash.
// TT is not built (train_impl has no such product): the host launcher refuses it.
#include "wrnn_internal.h"

namespace {

typedef float bg_f16v __attribute__((ext_vector_type(16)));
typedef float bg_f2v __attribute__((ext_vector_type(2)));
typedef __bf16 bg_bf2v __attribute__((ext_vector_type(2)));
typedef __bf16 bg_bf8v __attribute__((ext_vector_type(8)));

#define BG_M 128
#define BG_N 128
#define BG_K WRNN_GEMM_BF16_KTILE
#define BG_LD 40   // bf16 per LDS row: 32 + 8 of padding

// two floats -> two bf16 in one dword, round to nearest even (v_cvt_pk_bf16_f32); lo in bits 0..15
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    const bg_f2v f = {lo, hi};
    const bg_bf2v b = __builtin_convertvector(f, bg_bf2v);
    return __builtin_bit_cast(unsigned, b);
}

// A(m,k) = TA ? A[k*lda + m] : A[m*lda + k];  B(k,n) = TB ? B[n*ldb + k] : B[k*ldb + n]
template <bool TA, bool TB>
__global__ void __launch_bounds__(256) gemm_bf16_kernel(const float *__restrict__ A, long lda, const float *__restrict__ B, long ldb,
                                                        float *__restrict__ C, long ldc, int M, int N, int K, int beta,
                                                        const float *__restrict__ bias, int relu, int kper, long cslice) {
    // split K as in sgemm_kernel: blockIdx.z owns k in [z * kper, (z + 1) * kper) and writes its partial product to C + z * cslice
    if (kper > 0) {
        const long k_lo = (long)blockIdx.z * kper;
        A += TA ? k_lo * lda : k_lo;
        B += TB ? k_lo : k_lo * ldb;
        C += (long)blockIdx.z * cslice;
        K = K - k_lo < kper ? (int)(K - k_lo) : kper;
        if (K < 0) K = 0;
    }
    __shared__ __attribute__((aligned(16))) unsigned short As[BG_M][BG_LD];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[BG_N][BG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long m0 = (long)blockIdx.y * BG_M, n0 = (long)blockIdx.x * BG_N;
    float ra[16], rb[16];
    // operand rows are m for A and n for B; `kc`: the operand is k-contiguous in memory
    auto fetch_one = [&](const float *__restrict__ P, long ld, bool kc, long r0, int R, int k0, float (&reg)[16]) {
        if (kc) {
            const int c = tid & 15;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const long gr = r0 + (tid >> 4) + 16 * i;
                const int gk = k0 + 2 * c;
                reg[2 * i] = (gr < R && gk < K) ? P[gr * ld + gk] : 0.0f;
                reg[2 * i + 1] = (gr < R && gk + 1 < K) ? P[gr * ld + gk + 1] : 0.0f;
            }
        } else {
            const long gr = r0 + (tid & 127);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int gk = k0 + 16 * (tid >> 7) + j;
                reg[j] = (gr < R && gk < K) ? P[(long)gk * ld + gr] : 0.0f;
            }
        }
    };
    auto stash_one = [&](unsigned short (&S)[BG_M][BG_LD], bool kc, const float (&reg)[16]) {
        if (kc) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *(unsigned *)&S[(tid >> 4) + 16 * i][2 * (tid & 15)] = pack_bf16(reg[2 * i], reg[2 * i + 1]);
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                uint4 v;
                v.x = pack_bf16(reg[8 * q], reg[8 * q + 1]);
                v.y = pack_bf16(reg[8 * q + 2], reg[8 * q + 3]);
                v.z = pack_bf16(reg[8 * q + 4], reg[8 * q + 5]);
                v.w = pack_bf16(reg[8 * q + 6], reg[8 * q + 7]);
                *(uint4 *)&S[tid & 127][16 * (tid >> 7) + 8 * q] = v;
            }
        }
    };
    auto fetch = [&](int k0) {
        fetch_one(A, lda, !TA, m0, M, k0, ra);
        fetch_one(B, ldb, TB, n0, N, k0, rb);
    };
    bg_f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.0f;
    fetch(0);
    const int r = lane & 31, kh = lane >> 5;
    for (int k0 = 0; k0 < K; k0 += BG_K) {
        __syncthreads();
        stash_one(As, !TA, ra);
        stash_one(Bs, TB, rb);
        __syncthreads();
        if (k0 + BG_K < K) fetch(k0 + BG_K);
#pragma unroll
        for (int ks = 0; ks < BG_K; ks += 16) {
            const bg_bf8v a0 = *(const bg_bf8v *)&As[wm * 64 + r][ks + 8 * kh], a1 = *(const bg_bf8v *)&As[wm * 64 + 32 + r][ks + 8 * kh];
            const bg_bf8v b0 = *(const bg_bf8v *)&Bs[wn * 64 + r][ks + 8 * kh], b1 = *(const bg_bf8v *)&Bs[wn * 64 + 32 + r][ks + 8 * kh];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // D[i][j] of a 32x32 tile: j = lane % 32, i = 8 * (v / 4) + 4 * (lane / 32) + v % 4  (the map sgemm_kernel writes with)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const long gn = n0 + wn * 64 + tj * 32 + (lane & 31);
            if (gn >= N) continue;
            const float bv = bias ? bias[gn] : 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const long gm = m0 + wm * 64 + ti * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
                if (gm >= M) continue;
                float o = acc[ti][tj][v] + bv;
                if (beta) o += C[gm * ldc + gn];
                if (relu) o = fmaxf(o, 0.0f);
                C[gm * ldc + gn] = o;
            }
        }
}

}  // namespace

// hipErrorNotSupported: the TT form (not built).  M <= 0 or N <= 0: nothing to do.
hipError_t wrnn_gemm_bf16_launch(hipStream_t s, bool ta, bool tb, const float *A, long lda, const float *B, long ldb, float *C, long ldc, int M,
                                 int N, int K, int beta, const float *bias, int relu, int slices, int kper, long cslice) {
    if (ta && tb) return hipErrorNotSupported;
    if (M <= 0 || N <= 0) return hipSuccess;
    dim3 grid((N + BG_N - 1) / BG_N, (M + BG_M - 1) / BG_M, slices);
    if (ta) hipLaunchKernelGGL((gemm_bf16_kernel<true, false>), grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, M, N, K, beta, bias, relu, kper, cslice);
    else if (tb) hipLaunchKernelGGL((gemm_bf16_kernel<false, true>), grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, M, N, K, beta, bias, relu, kper, cslice);
    else hipLaunchKernelGGL((gemm_bf16_kernel<false, false>), grid, dim3(256), 0, s, A, lda, B, ldb, C, ldc, M, N, K, beta, bias, relu, kper, cslice);
    return hipGetLastError();
}
