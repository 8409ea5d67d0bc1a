// Time alignment on the device: the dynamic-time-warping path of a test clip against a target clip over their mel cepstra, and the
// mel-cepstral distortion, log-mel distance and F0 / voicing errors along that path.  The definitions are in the header's section.
// Plain grid kernels; nothing crosses workgroups, nothing spins, no floating-point atomics, every sum in a fixed order:
//   align_cep_kernel      grid (ceil(T_max / 4), B, 2)                      one wave per frame over the front end's mel: its K cepstra,
//                                                                           target (z = 0) and test (z = 1) through one code path
//   align_cost_kernel     grid (ceil(Tb_max / 32), ceil(Ta_max / 32), B)    a 32 x 32 tile of d(i, j), the cepstra of its frames in LDS
//   align_dp_kernel       grid (B)                                          one workgroup per pair: the accumulated cost along the
//                                                                           anti-diagonals, the choice bytes, the backtrack, the path
//   align_along_kernel    grid (ceil(P_max / 256), B)                       the log-mel distance and the cents of every path pair
//   align_summary_kernel  grid (B)                                          the WRNN_ALIGN_FIELDS summaries of a pair
// Precision: mels, cepstra, costs and F0 tracks are float32; every sum (over the mel rows, over the cepstra, the accumulated cost, the
// summaries) is float64.  A cost is rounded to float32 once, and both clips' cepstra come out of the same instructions, so identical
// frames cost exactly 0.
// The DP.  Cell (i, s - i) of anti-diagonal s needs diagonals s - 1 and s - 2 only: three rolling diagonals of float64 in LDS, indexed
// by the pair's SHORTER side (i when Ta <= Tb, else j), so a diagonal holds at most min(Ta, Tb) <= 4096 values (3 x 4096 x 8 = 96 KiB
// of the 160 KiB).  The threads stride over a diagonal's cells, one barrier per diagonal, Ta + Tb - 1 diagonals.  A thread's first cost
// of the NEXT diagonal is loaded before the barrier (the barrier does not wait for it), so the strided read of the cost matrix is off
// the chain.  Every cell's value is d + one of at most three numbers, picked by comparisons in a fixed order: nothing depends on the
// batch, so a pair of a ragged batch gives the bits of the call on it alone.
// The backtrack is one lane's chain of at most Ta + Tb - 1 dependent byte reads; every step lowers i + j and stays inside the matrix
// whatever the bytes hold, and the loop has that bound of its own.  It writes the path backwards into scratch; the workgroup reverses it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsp_device.h"
#include "dsp_tables.h"
#include "handle_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_WAVES = THREADS / 64;
constexpr int MAX_MELS = 128;             // the front end's own limit
constexpr int TILE = 32;                  // the cost kernel's tile, TILE x TILE cells
constexpr int DP_MAX_SIDE = 4096;         // the shorter side's frames: three float64 diagonals of it are 96 KiB of LDS
constexpr int64_t MAX_CELLS = 1LL << 28;  // B Ta_max Tb_max: a cell index fits 32 bits; 1 GiB of costs and 256 MiB of choices at most

__device__ inline int clamp_frames(int t, int t_max) { return t < 0 ? 0 : t > t_max ? t_max : t; }

struct AlignCepArgs {
    const float *mel[2];          // target, test: (B, n_mels, T_max[z]) in [0, 1]
    const int32_t *n_samples[2];  // [B] each
    float *cep[2];                // (B, T_max[z], K)
    int32_t *frames[2];           // [B] each: the clip's own frame count, written here for the kernels after this one
    const float *dct_t;           // (n_mels, K): C[k, m] at [m * K + k - 1]
    int64_t n_max[2];
    int32_t T_max[2];
    int32_t n_mels, hop, K, min_samples;
    double scale;                 // -min_level_db ln 10 / 20
};

// One wave per frame; lane l holds mel rows l and l + 64, then DCT rows l + 1 and l + 65.  z = 0: the target, 1: the test.
__global__ void __launch_bounds__(THREADS) align_cep_kernel(AlignCepArgs g) {
    __shared__ float e[MAX_WAVES][MAX_MELS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y, z = blockIdx.z;
    const int T_max = g.T_max[z];
    long n = g.n_samples[z][b];
    if (n > g.n_max[z]) n = g.n_max[z];
    const int T_b = n >= g.min_samples ? clamp_frames((int)(1 + n / g.hop), T_max) : 0;   // a clip too short to pad has no frames
    if (blockIdx.x == 0 && threadIdx.x == 0) g.frames[z][b] = T_b;
    const int t = blockIdx.x * MAX_WAVES + wave;
    if (t >= T_max) return;                 // wave-uniform; no workgroup barrier below, every wave keeps to its own row of `e`
    float *out = g.cep[z] + ((long)b * T_max + t) * g.K;
    if (t >= T_b) {
        for (int k = lane; k < g.K; k += 64) out[k] = 0.0f;
        return;
    }
    const float *mel = g.mel[z] + (long)b * g.n_mels * T_max + t;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = lane + 64 * h;
        if (m < g.n_mels) e[wave][m] = mel[(long)m * T_max];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;        // DCT row k + 1
        if (k < g.K) {
            double c = 0.0;
            for (int m = 0; m < g.n_mels; ++m) c = fma((double)g.dct_t[m * g.K + k], (double)e[wave][m], c);
            out[k] = (float)(c * g.scale);
        }
    }
}

struct AlignCostArgs {
    const float *cep_a, *cep_b;   // (B, Ta_max, K), (B, Tb_max, K)
    const int32_t *ta, *tb;       // [B] the pairs' own frame counts
    float *cost;                  // (B, Ta_max, Tb_max)
    int32_t Ta_max, Tb_max, K;
};

// A TILE x TILE tile of one pair.  Thread (tid >> 5, tid & 31) takes rows tid >> 5, + 8, + 16, + 24 of column tid & 31: the row's cepstra
// are one broadcast read, the column's lie KS = K | 1 floats apart (an odd stride: no bank conflict).  The sum over k ascends, in float64.
__global__ void __launch_bounds__(THREADS) align_cost_kernel(AlignCostArgs g) {
    extern __shared__ float tile[];         // TILE x KS of the target's frames, then of the test's
    const int KS = g.K | 1;
    float *sa = tile, *sb = tile + TILE * KS;
    const int tid = threadIdx.x, b = blockIdx.z, i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    const int Ta = clamp_frames(g.ta[b], g.Ta_max), Tb = clamp_frames(g.tb[b], g.Tb_max);
    const bool live = i0 < Ta && j0 < Tb;   // workgroup-uniform: a tile wholly outside the pair's own matrix is zeros
    if (live) {
        const float *ca = g.cep_a + (long)b * g.Ta_max * g.K, *cb = g.cep_b + (long)b * g.Tb_max * g.K;
        for (int x = tid; x < TILE * g.K; x += THREADS) {
            const int r = x / g.K, k = x - r * g.K;
            sa[r * KS + k] = i0 + r < Ta ? ca[(long)(i0 + r) * g.K + k] : 0.0f;
            sb[r * KS + k] = j0 + r < Tb ? cb[(long)(j0 + r) * g.K + k] : 0.0f;
        }
        __syncthreads();
    }
    const int tj = tid & (TILE - 1), j = j0 + tj;
    float *out = g.cost + (long)b * g.Ta_max * g.Tb_max;
#pragma unroll
    for (int r = 0; r < TILE / 8; ++r) {
        const int ti = (tid >> 5) + 8 * r, i = i0 + ti;
        if (i >= g.Ta_max || j >= g.Tb_max) continue;
        float d = 0.0f;
        if (live && i < Ta && j < Tb) {
            double s = 0.0;
            for (int k = 0; k < g.K; ++k) {
                const double df = (double)sa[ti * KS + k] - (double)sb[tj * KS + k];
                s = fma(df, df, s);
            }
            d = (float)(4.342944819032518 * sqrt(2.0 * s));   // 10 / ln 10
        }
        out[(long)i * g.Tb_max + j] = d;
    }
}

struct AlignDpArgs {
    const float *cost;            // (B, Ta_max, Tb_max)
    const int32_t *ta, *tb;       // [B]
    uint8_t *choice;              // (B, Ta_max, Tb_max) scratch: 0 diagonal, 1 (i - 1, j), 2 (i, j - 1), 3 the cell (0, 0)
    int2 *rev;                    // (B, P_max) scratch: the path as the backtrack meets it
    int2 *path;                   // (B, P_max): (i_p, j_p) ascending, (-1, -1) past P
    int32_t *path_len;            // [B]
    double *total;                // [B]
    int32_t Ta_max, Tb_max, L;    // L = min(Ta_max, Tb_max): the length of an LDS diagonal
};

__global__ void __launch_bounds__(THREADS) align_dp_kernel(AlignDpArgs g) {
    extern __shared__ double diag[];        // 3 x L
    __shared__ int P_sh;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Ta = clamp_frames(g.ta[b], g.Ta_max), Tb = clamp_frames(g.tb[b], g.Tb_max);
    const int P_max = g.Ta_max + g.Tb_max - 1;
    int2 *path = g.path + (long)b * P_max;
    if (Ta == 0 || Tb == 0) {               // workgroup-uniform: a clip without frames has no path
        for (int p = tid; p < P_max; p += THREADS) path[p] = make_int2(-1, -1);
        if (tid == 0) {
            g.path_len[b] = 0;
            g.total[b] = 0.0;
        }
        return;
    }
    const float *cost = g.cost + (long)b * g.Ta_max * g.Tb_max;
    uint8_t *ch = g.choice + (long)b * g.Ta_max * g.Tb_max;
    const int Tbm = g.Tb_max;
    const bool by_i = Ta <= Tb;             // the diagonals are indexed by the shorter side: idx < min(Ta, Tb) <= L
    const int S = Ta + Tb - 1;
    int o2 = 0, o1 = g.L, o0 = 2 * g.L;     // diagonals s - 2, s - 1, s
    // One diagonal.  This thread's first cell of diagonal s is (lo + tid, s - lo - tid); its cost arrives in `cur`, loaded one diagonal
    // ahead, and the one of diagonal s + 1 is requested into `nxt` before the barrier, which does not wait for it.
    auto step = [&](int s, float &cur, float &nxt) {
        const int lo = s - (Tb - 1) > 0 ? s - (Tb - 1) : 0, hi = s < Ta - 1 ? s : Ta - 1;
        {
            const int s1 = s + 1, lo1 = s1 - (Tb - 1) > 0 ? s1 - (Tb - 1) : 0, hi1 = s1 < Ta - 1 ? s1 : Ta - 1, i1 = lo1 + tid;
            nxt = s1 < S && i1 <= hi1 ? cost[i1 * Tbm + (s1 - i1)] : 0.0f;
        }
        const double *d2 = diag + o2, *d1 = diag + o1;
        double *d0 = diag + o0;
        for (int i = lo + tid; i <= hi; i += THREADS) {
            const int j = s - i, idx = by_i ? i : j;
            const float d = i == lo + tid ? cur : cost[i * Tbm + j];
            // D_{s-1}[idx - 1] is (i - 1, j) when indexed by i and (i, j - 1) when indexed by j; D_{s-1}[idx] the other; D_{s-2}[idx - 1] the diagonal
            double best = 0.0;
            uint8_t c = 3;
            if (i > 0 && j > 0) {
                const double up = by_i ? d1[idx - 1] : d1[idx], left = by_i ? d1[idx] : d1[idx - 1];
                best = d2[idx - 1];
                c = 0;
                if (up < best) {
                    best = up;
                    c = 1;
                }
                if (left < best) {
                    best = left;
                    c = 2;
                }
            } else if (i > 0) {
                best = by_i ? d1[idx - 1] : d1[idx];
                c = 1;
            } else if (j > 0) {
                best = by_i ? d1[idx] : d1[idx - 1];
                c = 2;
            }
            const double D = c == 3 ? (double)d : (double)d + best;
            d0[idx] = D;
            ch[i * Tbm + j] = c;
            if (s == S - 1) g.total[b] = D;
        }
        __syncthreads();
        const int o = o2;
        o2 = o1;
        o1 = o0;
        o0 = o;
    };
    // two diagonals per trip, so that the cost in flight across a barrier is never copied (a copy would wait for it)
    float d_even = tid == 0 ? cost[0] : 0.0f, d_odd = 0.0f;
    for (int s = 0; s < S; s += 2) {
        step(s, d_even, d_odd);
        if (s + 1 < S) step(s + 1, d_odd, d_even);
    }
    // the choice bytes of the whole workgroup, visible to the one lane that walks them (the waits are written out: the loop above
    // leaves stores in flight on purpose)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int2 *rev = g.rev + (long)b * P_max;
    if (tid == 0) {
        int i = Ta - 1, j = Tb - 1, n = 0;
        while (n < S) {                     // the bound of its own: Ta + Tb - 1 steps whatever the bytes hold
            rev[n++] = make_int2(i, j);
            if (i == 0 && j == 0) break;
            const uint8_t c = ch[i * Tbm + j];
            // every arm lowers i + j and keeps i, j >= 0
            if (c == 0 && i > 0 && j > 0) {
                --i;
                --j;
            } else if (c == 2 && j > 0) {
                --j;
            } else if (i > 0) {
                --i;
            } else {
                --j;
            }
        }
        P_sh = n;
        g.path_len[b] = n;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int P = P_sh;
    for (int p = tid; p < P_max; p += THREADS) path[p] = p < P ? rev[P - 1 - p] : make_int2(-1, -1);
}

struct AlignAlongArgs {
    const float *mel_a, *mel_b;   // (B, n_mels, Ta_max), (B, n_mels, Tb_max)
    const int2 *path;             // (B, P_max)
    const int32_t *path_len;      // [B]
    const float *f0_a, *f0_b;     // (B, f0_stride) each, or both NULL
    double *pp;                   // (B, 2, P_max): lsd_p | cents_p, zeros past P
    const int32_t *ta, *tb;       // [B]
    const double *total;          // [B]
    double *summary;              // (B, WRNN_ALIGN_FIELDS)
    int64_t f0_stride;
    int32_t Ta_max, Tb_max, n_mels;
    double range_db, gpe_ratio;
};

__global__ void __launch_bounds__(THREADS) align_along_kernel(AlignAlongArgs g) {
    const int p = blockIdx.x * THREADS + threadIdx.x, b = blockIdx.y;
    const int P_max = g.Ta_max + g.Tb_max - 1;
    if (p >= P_max) return;
    double lsd = 0.0, cents = 0.0;
    if (p < g.path_len[b]) {
        const int2 ij = g.path[(long)b * P_max + p];
        const float *ma = g.mel_a + (long)b * g.n_mels * g.Ta_max + ij.x, *mb = g.mel_b + (long)b * g.n_mels * g.Tb_max + ij.y;
        double s = 0.0;
        for (int m = 0; m < g.n_mels; ++m) {
            const double df = ((double)ma[(long)m * g.Ta_max] - (double)mb[(long)m * g.Tb_max]) * g.range_db;
            s = fma(df, df, s);
        }
        lsd = sqrt(s / (double)g.n_mels);
        if (g.f0_a) {
            const double ft = (double)g.f0_a[(long)b * g.f0_stride + ij.x], fs = (double)g.f0_b[(long)b * g.f0_stride + ij.y];
            if (ft > 0.0 && fs > 0.0) cents = 1200.0 * log2(fs / ft);
        }
    }
    g.pp[((long)b * 2) * P_max + p] = lsd;
    g.pp[((long)b * 2 + 1) * P_max + p] = cents;
}

// One workgroup per pair.  Thread i takes path pairs i, i + 256, ... in ascending order, then the threads are added in a fixed tree: the
// order depends on a pair's place on the path alone.  Two passes, as the pitch summaries: the counts, the squares and the means of
// log2 f0, then the central moments.
__global__ void __launch_bounds__(THREADS) align_summary_kernel(AlignAlongArgs g) {
    __shared__ double acc[7 * THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int P_max = g.Ta_max + g.Tb_max - 1, P = g.path_len[b];
    const int2 *path = g.path + (long)b * P_max;
    const double *lsd = g.pp + ((long)b * 2) * P_max, *cents = lsd + P_max;
    const float *fa = g.f0_a ? g.f0_a + (long)b * g.f0_stride : nullptr, *fb = g.f0_a ? g.f0_b + (long)b * g.f0_stride : nullptr;
    double n_v = 0.0, n_vde = 0.0, n_gpe = 0.0, c2 = 0.0, lt = 0.0, ls = 0.0, sl = 0.0;
    for (int p = tid; p < P; p += THREADS) {
        sl += lsd[p];
        if (fa) {
            const int2 ij = path[p];
            const double ft = (double)fa[ij.x], fs = (double)fb[ij.y];
            const bool vt = ft > 0.0, vs = fs > 0.0;
            n_vde += vt != vs ? 1.0 : 0.0;
            if (vt && vs) {
                const double c = cents[p];
                n_v += 1.0;
                n_gpe += fabs(fs / ft - 1.0) > g.gpe_ratio ? 1.0 : 0.0;
                c2 += c * c;
                lt += log2(ft);
                ls += log2(fs);
            }
        }
    }
    double first[7] = {n_v, n_vde, n_gpe, c2, lt, ls, sl};
    block_sums<THREADS>(first, acc);
    n_v = first[0]; n_vde = first[1]; n_gpe = first[2]; c2 = first[3]; lt = first[4]; ls = first[5]; sl = first[6];
    const double mt = n_v > 0.0 ? lt / n_v : 0.0, ms = n_v > 0.0 ? ls / n_v : 0.0;
    double cov = 0.0, var_t = 0.0, var_s = 0.0;
    if (fa) {
        for (int p = tid; p < P; p += THREADS) {
            const int2 ij = path[p];
            const double ft = (double)fa[ij.x], fs = (double)fb[ij.y];
            if (ft > 0.0 && fs > 0.0) {
                const double a = log2(ft) - mt, c = log2(fs) - ms;
                cov += a * c;
                var_t += a * a;
                var_s += c * c;
            }
        }
    }
    double second[3] = {cov, var_t, var_s};
    block_sums<THREADS>(second, acc);
    cov = second[0]; var_t = second[1]; var_s = second[2];
    if (tid != 0) return;
    double *o = g.summary + (long)b * WRNN_ALIGN_FIELDS;
    for (int i = 0; i < WRNN_ALIGN_FIELDS; ++i) o[i] = 0.0;
    if (P == 0) return;
    const double Pd = (double)P;
    o[WRNN_ALIGN_TOTAL_COST] = g.total[b];
    o[WRNN_ALIGN_PATH_LEN] = Pd;
    o[WRNN_ALIGN_FRAMES_TARGET] = (double)clamp_frames(g.ta[b], g.Ta_max);
    o[WRNN_ALIGN_FRAMES_TEST] = (double)clamp_frames(g.tb[b], g.Tb_max);
    o[WRNN_ALIGN_MCD_DTW_DB] = g.total[b] / Pd;
    o[WRNN_ALIGN_MEL_LSD_DTW_DB] = sl / Pd;
    if (n_v > 0.0) {
        o[WRNN_ALIGN_F0_RMSE_CENTS] = sqrt(c2 / n_v);
        o[WRNN_ALIGN_GPE] = n_gpe / n_v;
    }
    o[WRNN_ALIGN_VDE] = n_vde / Pd;
    o[WRNN_ALIGN_FFE] = (n_gpe + n_vde) / Pd;
    if (n_v >= 2.0 && var_t > 0.0 && var_s > 0.0) o[WRNN_ALIGN_F0_CORR] = cov / sqrt(var_t * var_s);
    o[WRNN_ALIGN_VOICED_BOTH] = n_v;
}

}  // namespace

// ---- the C entries ----------------------------------------------------------------------------------------------------------------------

struct wrnn_align_handle {
    wrnn_mel_config cfg{};
    wrnn_mel_features feat{};
    wrnn_align_config acfg{};
    bool ok = false;                  // false while the configuration is refused
    int min_samples = 0;              // the shortest clip the front end can pad
    wrnn_mel_handle *mel = nullptr;   // the front end the mels come from: its own handle, its own launch path
    std::vector<float> dct;           // (K, n_mels): dsp_tables.h's rows rounded to float32, what wrnn_score_tables hands out
    void *dct_dev = nullptr;          // its transpose, uploaded by the first call that needs it
    bool lds_set = false;             // the DP kernel's dynamic LDS limit is raised once
    WrnnScratch ws;                   // the scratch of a call, grown on demand
    std::string err;
};

namespace {
// The scratch of a call over (B, Ta_max, Tb_max), region by region; a call takes the regions it needs, in this order.
struct AlLayout {
    size_t mel_a = 0, mel_b = 0, cep_a = 0, cep_b = 0, frames = 0, cost = 0, choice = 0, rev = 0, path = 0, plen = 0, total = 0, pp = 0, bytes = 0;
};
enum { AL_MELS = 1, AL_COST = 2, AL_DP = 4, AL_PATH = 8, AL_ALONG = 16 };

AlLayout al_layout(const wrnn_align_handle *h, int64_t B, int64_t Ta, int64_t Tb, int what) {
    AlLayout l;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += wrnn_up256(bytes);
        return o;
    };
    const size_t n_mels = (size_t)h->cfg.n_mels, K = (size_t)h->acfg.mcd_order, P = (size_t)(Ta + Tb - 1);
    if (what & AL_MELS) {
        l.mel_a = take((size_t)B * n_mels * Ta * 4);
        l.mel_b = take((size_t)B * n_mels * Tb * 4);
        l.cep_a = take((size_t)B * Ta * K * 4);
        l.cep_b = take((size_t)B * Tb * K * 4);
        l.frames = take((size_t)B * 2 * 4);
    }
    if (what & AL_COST) l.cost = take((size_t)B * Ta * Tb * 4);
    if (what & AL_DP) {
        l.choice = take((size_t)B * Ta * Tb);
        l.rev = take((size_t)B * P * 8);
    }
    if (what & AL_PATH) {
        l.path = take((size_t)B * P * 8);
        l.plen = take((size_t)B * 4);
        l.total = take((size_t)B * 8);
    }
    if (what & AL_ALONG) l.pp = take((size_t)B * 2 * P * 8);
    l.bytes = at;
    return l;
}

// WRNN_OK, or the status and the text of the refusal of a call over (B, Ta_max, Tb_max) frames.
int al_check_shape(wrnn_align_handle *h, int64_t B, int64_t Ta, int64_t Tb) {
    if (B < 1 || B > WRNN_MAX_GRID_Y || Ta < 1 || Tb < 1 || Ta > INT32_MAX / 2 || Tb > INT32_MAX / 2)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad shape: 1 <= B <= %d, Ta_max and Tb_max at least 1, got B = %lld, Ta_max = %lld, Tb_max = %lld", WRNN_MAX_GRID_Y,
                       (long long)B, (long long)Ta, (long long)Tb);
    if ((Ta < Tb ? Ta : Tb) > DP_MAX_SIDE)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "min(Ta_max, Tb_max) = %lld frames: three float64 anti-diagonals of the shorter side fit the LDS up to %d frames",
                       (long long)(Ta < Tb ? Ta : Tb), DP_MAX_SIDE);
    if (Ta * Tb > MAX_CELLS || B * Ta * Tb > MAX_CELLS)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "B Ta_max Tb_max = %lld x %lld x %lld cells: a call holds at most 2^28 (32-bit cell indices, 1 GiB of costs)",
                       (long long)B, (long long)Ta, (long long)Tb);
    return WRNN_OK;
}

int64_t al_frames(const wrnn_align_handle *h, int64_t n) { return 1 + n / h->cfg.hop_length; }

// The two mels, the cepstra and the frame counts into the scratch, then the cost matrices into `cost`.
int al_launch_cost(wrnn_align_handle *h, const AlLayout &l, const float *target_dev, int64_t na_max, const int32_t *na_dev, const float *test_dev,
                   int64_t nb_max, const int32_t *nb_dev, int B, int Ta, int Tb, float *cost, hipStream_t s) {
    const int n_mels = h->cfg.n_mels, K = h->acfg.mcd_order;
    if (!h->dct_dev) {
        WrnnImage img;
        float *t = img.at<float>(img.take((size_t)n_mels * K * 4));
        for (int k = 0; k < K; ++k)
            for (int m = 0; m < n_mels; ++m) t[(size_t)m * K + k] = h->dct[(size_t)k * n_mels + m];
        const hipError_t e = img.upload(&h->dct_dev);
        if (e != hipSuccess) return wrnn_failf(h, WRNN_ERR_HIP, "uploading the DCT table: %s", hipGetErrorString(e));
    }
    float *mel_a = (float *)(h->ws.p + l.mel_a), *mel_b = (float *)(h->ws.p + l.mel_b);
    if (wrnn_melspectrogram(h->mel, target_dev, na_max, na_dev, B, Ta, mel_a, (void *)s) != WRNN_OK ||
        wrnn_melspectrogram(h->mel, test_dev, nb_max, nb_dev, B, Tb, mel_b, (void *)s) != WRNN_OK)
        return wrnn_failf(h, WRNN_ERR_HIP, "the mel front end: %s", wrnn_mel_last_error(h->mel));
    AlignCepArgs c{};
    c.mel[0] = mel_a; c.mel[1] = mel_b; c.n_samples[0] = na_dev; c.n_samples[1] = nb_dev;
    c.cep[0] = (float *)(h->ws.p + l.cep_a); c.cep[1] = (float *)(h->ws.p + l.cep_b);
    c.frames[0] = (int32_t *)(h->ws.p + l.frames); c.frames[1] = c.frames[0] + B;
    c.dct_t = (const float *)h->dct_dev; c.n_max[0] = na_max; c.n_max[1] = nb_max; c.T_max[0] = Ta; c.T_max[1] = Tb;
    c.n_mels = n_mels; c.hop = h->cfg.hop_length; c.K = K; c.min_samples = h->min_samples;
    c.scale = (double)(-h->cfg.min_level_db) * (2.302585092994046 / 20.0);
    const int T = Ta > Tb ? Ta : Tb;
    hipLaunchKernelGGL(align_cep_kernel, dim3((unsigned)((T + MAX_WAVES - 1) / MAX_WAVES), (unsigned)B, 2u), dim3(THREADS), 0, s, c);
    WRNN_TRY(h, hipGetLastError());
    AlignCostArgs a{};
    a.cep_a = c.cep[0]; a.cep_b = c.cep[1]; a.ta = c.frames[0]; a.tb = c.frames[1]; a.cost = cost; a.Ta_max = Ta; a.Tb_max = Tb; a.K = K;
    const size_t lds = (size_t)2 * TILE * (K | 1) * 4;   // at most 2 x 32 x 127 floats = 32 KiB
    hipLaunchKernelGGL(align_cost_kernel, dim3((unsigned)((Tb + TILE - 1) / TILE), (unsigned)((Ta + TILE - 1) / TILE), (unsigned)B), dim3(THREADS), lds, s, a);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}

int al_launch_dp(wrnn_align_handle *h, const AlLayout &l, const float *cost, const int32_t *ta, const int32_t *tb, int B, int Ta, int Tb, int2 *path,
                 int32_t *path_len, double *total, hipStream_t s) {
    AlignDpArgs d{};
    d.cost = cost; d.ta = ta; d.tb = tb; d.choice = (uint8_t *)(h->ws.p + l.choice); d.rev = (int2 *)(h->ws.p + l.rev);
    d.path = path; d.path_len = path_len; d.total = total; d.Ta_max = Ta; d.Tb_max = Tb; d.L = Ta < Tb ? Ta : Tb;
    if (!h->lds_set) {
        WRNN_TRY(h, hipFuncSetAttribute((const void *)align_dp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * DP_MAX_SIDE * 8));
        h->lds_set = true;
    }
    hipLaunchKernelGGL(align_dp_kernel, dim3((unsigned)B), dim3(THREADS), (size_t)3 * d.L * 8, s, d);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}
}  // namespace

extern "C" {

int wrnn_align_create(const wrnn_mel_config *cfg, const wrnn_mel_features *f, const wrnn_align_config *ac, wrnn_align_handle **out) {
    if (!cfg || !ac || !out) return WRNN_ERR_INVALID;
    wrnn_align_handle *h = new wrnn_align_handle();
    *out = h;
    h->cfg = *cfg;
    if (!f) f = &WRNN_DEFAULT_MEL_FEATURES;
    if (ac->struct_size != sizeof(wrnn_align_config))
        return wrnn_failf(h, WRNN_ERR_INVALID, "align.struct_size = %u, this library's wrnn_align_config has %zu bytes", ac->struct_size, sizeof(wrnn_align_config));
    h->acfg = *ac;
    // the front end checks its own configuration (struct_size of the features included) and builds its own tables; no device is touched
    const int rc = wrnn_mel_create_features(cfg, f, &h->mel);
    if (rc != WRNN_OK) return wrnn_failf(h, rc, "%s", h->mel ? wrnn_mel_last_error(h->mel) : "wrnn_mel_create_features failed");
    h->feat = *f;
    if (ac->mcd_order < 1 || ac->mcd_order > cfg->n_mels - 1)
        return wrnn_failf(h, WRNN_ERR_INVALID, "mcd_order = %d: 1 <= mcd_order <= n_mels - 1 = %d", ac->mcd_order, cfg->n_mels - 1);
    if (!(ac->gpe_ratio > 0.0) || !std::isfinite(ac->gpe_ratio)) return wrnn_failf(h, WRNN_ERR_INVALID, "gpe_ratio = %g: finite and above 0", ac->gpe_ratio);
    // the DCT rows are the score section's own: the same builder, the same one rounding to float32
    const std::vector<double> dct = wrnn_dsp::dct_rows(cfg->n_mels, ac->mcd_order);
    h->dct.assign(dct.begin(), dct.end());
    h->min_samples = f->pad_mode == WRNN_MEL_PAD_REFLECT ? cfg->n_fft / 2 + 1 : 1;
    h->ok = true;
    return WRNN_OK;
}

int64_t wrnn_align_frames(const wrnn_align_handle *h, int64_t n) {
    if (!h || !h->ok || n < h->min_samples || n > INT32_MAX) return WRNN_ERR_INVALID;
    return al_frames(h, n);
}

int64_t wrnn_align_workspace_bytes(wrnn_align_handle *h, int32_t B, int64_t na_max, int64_t nb_max) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_align_create");
    if (na_max < h->min_samples || nb_max < h->min_samples || na_max > INT32_MAX || nb_max > INT32_MAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: %d <= na_max, nb_max < 2^31", h->min_samples);
    const int64_t Ta = al_frames(h, na_max), Tb = al_frames(h, nb_max);
    const int rc = al_check_shape(h, B, Ta, Tb);
    if (rc != WRNN_OK) return rc;
    return (int64_t)al_layout(h, B, Ta, Tb, AL_MELS | AL_COST | AL_DP | AL_PATH | AL_ALONG).bytes;
}

int wrnn_align_cost(wrnn_align_handle *h, const float *target_dev, int64_t na_max, const int32_t *na_dev, const float *test_dev, int64_t nb_max,
                    const int32_t *nb_dev, int32_t B, float *cost_dev, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_align_create");
    if (!target_dev || !test_dev || !na_dev || !nb_dev || !cost_dev || na_max < h->min_samples || nb_max < h->min_samples || na_max > INT32_MAX ||
        nb_max > INT32_MAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, %d <= na_max, nb_max < 2^31", h->min_samples);
    const int64_t Ta = al_frames(h, na_max), Tb = al_frames(h, nb_max);
    const int rc = al_check_shape(h, B, Ta, Tb);
    if (rc != WRNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    const AlLayout l = al_layout(h, B, Ta, Tb, AL_MELS);
    WRNN_TRY(h, h->ws.reserve(l.bytes, s));
    return al_launch_cost(h, l, target_dev, na_max, na_dev, test_dev, nb_max, nb_dev, B, (int)Ta, (int)Tb, cost_dev, s);
}

int wrnn_align_path(wrnn_align_handle *h, const float *cost_dev, int32_t B, int32_t Ta_max, int32_t Tb_max, const int32_t *ta_dev, const int32_t *tb_dev,
                    int32_t *path_dev, int32_t *path_len_dev, double *total_dev, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_align_create");
    if (!cost_dev || !ta_dev || !tb_dev || !path_dev || !path_len_dev || !total_dev)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: cost_dev, ta_dev, tb_dev, path_dev, path_len_dev and total_dev are device pointers");
    const int rc = al_check_shape(h, B, Ta_max, Tb_max);
    if (rc != WRNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    const AlLayout l = al_layout(h, B, Ta_max, Tb_max, AL_DP);
    WRNN_TRY(h, h->ws.reserve(l.bytes, s));
    return al_launch_dp(h, l, cost_dev, ta_dev, tb_dev, B, Ta_max, Tb_max, (int2 *)path_dev, path_len_dev, total_dev, s);
}

int wrnn_align_score(wrnn_align_handle *h, const float *target_dev, int64_t na_max, const int32_t *na_dev, const float *test_dev, int64_t nb_max,
                     const int32_t *nb_dev, int32_t B, const float *f0_target_dev, const float *f0_test_dev, int64_t f0_stride, double *summary_dev,
                     int32_t *path_dev, int32_t *path_len_dev, double *per_path_dev, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_align_create");
    if (!target_dev || !test_dev || !na_dev || !nb_dev || !summary_dev || na_max < h->min_samples || nb_max < h->min_samples || na_max > INT32_MAX ||
        nb_max > INT32_MAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, %d <= na_max, nb_max < 2^31", h->min_samples);
    if ((f0_target_dev == nullptr) != (f0_test_dev == nullptr))
        return wrnn_failf(h, WRNN_ERR_INVALID, "f0_target_dev and f0_test_dev are both NULL or both set");
    const int64_t Ta = al_frames(h, na_max), Tb = al_frames(h, nb_max);
    if (f0_target_dev && f0_stride < (Ta > Tb ? Ta : Tb))
        return wrnn_failf(h, WRNN_ERR_INVALID, "f0_stride = %lld: a row of the F0 tracks holds max(Ta_max, Tb_max) = %lld frames", (long long)f0_stride,
                       (long long)(Ta > Tb ? Ta : Tb));
    const int rc = al_check_shape(h, B, Ta, Tb);
    if (rc != WRNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    const AlLayout l = al_layout(h, B, Ta, Tb, AL_MELS | AL_COST | AL_DP | AL_PATH | AL_ALONG);
    WRNN_TRY(h, h->ws.reserve(l.bytes, s));
    int r = al_launch_cost(h, l, target_dev, na_max, na_dev, test_dev, nb_max, nb_dev, B, (int)Ta, (int)Tb, (float *)(h->ws.p + l.cost), s);
    if (r != WRNN_OK) return r;
    const int32_t *ta = (const int32_t *)(h->ws.p + l.frames), *tb = ta + B;
    int2 *path = path_dev ? (int2 *)path_dev : (int2 *)(h->ws.p + l.path);
    int32_t *plen = path_len_dev ? path_len_dev : (int32_t *)(h->ws.p + l.plen);
    double *total = (double *)(h->ws.p + l.total);
    r = al_launch_dp(h, l, (const float *)(h->ws.p + l.cost), ta, tb, B, (int)Ta, (int)Tb, path, plen, total, s);
    if (r != WRNN_OK) return r;
    AlignAlongArgs g{};
    g.mel_a = (const float *)(h->ws.p + l.mel_a); g.mel_b = (const float *)(h->ws.p + l.mel_b); g.path = path; g.path_len = plen;
    g.f0_a = f0_target_dev; g.f0_b = f0_test_dev; g.pp = per_path_dev ? per_path_dev : (double *)(h->ws.p + l.pp); g.ta = ta; g.tb = tb; g.total = total;
    g.summary = summary_dev; g.f0_stride = f0_stride; g.Ta_max = (int)Ta; g.Tb_max = (int)Tb; g.n_mels = h->cfg.n_mels;
    g.range_db = (double)(-h->cfg.min_level_db); g.gpe_ratio = h->acfg.gpe_ratio;
    const int P_max = (int)(Ta + Tb - 1);
    hipLaunchKernelGGL(align_along_kernel, dim3((unsigned)((P_max + THREADS - 1) / THREADS), (unsigned)B), dim3(THREADS), 0, s, g);
    WRNN_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(align_summary_kernel, dim3((unsigned)B), dim3(THREADS), 0, s, g);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}

const char *wrnn_align_last_error(const wrnn_align_handle *h) { return wrnn_last_error_of(h); }

void wrnn_align_destroy(wrnn_align_handle *h) {
    if (!h) return;
    if (h->dct_dev || h->ws.p) {
        (void)hipSetDevice(h->cfg.device);
        if (h->dct_dev) (void)hipFree(h->dct_dev);
        h->ws.release();
    }
    if (h->mel) wrnn_mel_destroy(h->mel);
    delete h;
}

}  // extern "C"
