// Device helpers of the analysis kernels (header-only, inlined: every file compiles them under its own flags).
#pragma once
#include <hip/hip_runtime.h>

// T2: float2 or double2
template <class T2, class T>
__device__ inline T2 cplx(T x, T y) {
    return T2{x, y};
}

template <class T2>
__device__ inline T2 cmul(T2 a, T2 b) {
    return cplx<T2>(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// base-4 digit reversal of a 10-bit index: bit reversal, then the two bits of every digit swapped back
__device__ inline int rev4(int k) {
    const unsigned r = __brev((unsigned)k) >> 22;
    return (int)(((r & 0x2AAu) >> 1) | ((r & 0x155u) << 1));
}

// 1024-point complex transform in place in LDS by 256 threads, input digit-reversed (rev4): five radix-4 passes, one butterfly per
// thread and pass; W_4 = -i.  `twiddle` is the 2048-point table (cos, -sin).  Starts with a barrier (the caller's stores), ends with one.
template <class T2>
__device__ inline void radix4_1024(T2 *z, const T2 *twiddle, int tid) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        __syncthreads();
        const int q = 1 << (2 * s);
        const int pos = tid & (q - 1), base = ((tid >> (2 * s)) << (2 * s + 2)) + pos;
        T2 a0 = z[base], a1 = z[base + q], a2 = z[base + 2 * q], a3 = z[base + 3 * q];
        if (s > 0) {
            const int ts = pos * (512 >> (2 * s));   // W_L^pos as an index into the n_fft-point table, L = 4 q
            a1 = cmul(a1, twiddle[ts]);
            a2 = cmul(a2, twiddle[2 * ts]);
            a3 = cmul(a3, twiddle[3 * ts]);
        }
        const T2 s02 = cplx<T2>(a0.x + a2.x, a0.y + a2.y), d02 = cplx<T2>(a0.x - a2.x, a0.y - a2.y);
        const T2 s13 = cplx<T2>(a1.x + a3.x, a1.y + a3.y), d13 = cplx<T2>(a1.x - a3.x, a1.y - a3.y);
        z[base] = cplx<T2>(s02.x + s13.x, s02.y + s13.y);
        z[base + q] = cplx<T2>(d02.x + d13.y, d02.y - d13.x);       // d02 - i d13
        z[base + 2 * q] = cplx<T2>(s02.x - s13.x, s02.y - s13.y);
        z[base + 3 * q] = cplx<T2>(d02.x - d13.y, d02.y + d13.x);   // d02 + i d13
    }
    __syncthreads();
}

// The sums of N values per thread, to every thread of a workgroup of THREADS: one fixed pairwise tree over the thread index for all N
// (acc holds N * THREADS doubles of LDS).
template <int THREADS, int N>
__device__ inline void block_sums(double (&v)[N], double *acc) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k * THREADS + tid] = v[k];
    for (int d = THREADS / 2; d > 0; d >>= 1) {
        __syncthreads();
        if (tid < d) {
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k * THREADS + tid] += acc[k * THREADS + tid + d];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = acc[k * THREADS];
    __syncthreads();
}
