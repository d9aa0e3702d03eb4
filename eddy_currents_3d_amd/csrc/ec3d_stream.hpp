// ec3d_stream.hpp — the fixed-order sums and the streaming idiom of every kernel outside the iteration's hot path
// (ec3d_guess.hip, ec3d_null.hip, ec3d_integrals.hip, ec3d_mg.hip, ec3d_outer.hip; DESIGN.md "Fixed-order sums").
// The hot path's own block_sum (ec3d_kernels.hip) is another function: no leading 0.0, valid in every thread.
//
// Summation chain (no float atomics: a result is a pure function of its inputs; tests/device_sums_numpy.py restates it):
//   a thread adds its own terms in order, from 0.0;
//   the workgroup of 256 threads (stream_block_sum): per wave six levels of the shuffle tree (lane l takes lane l + 32,
//   + 16, ... + 1), then thread 0 adds the four waves' sums in order from 0.0 -- one partial per workgroup and sum;
//   one workgroup collapses the partials: thread t adds the partials t, t + 256, ... in order from 0.0
//   (stream_strided_sum), then the same tree.
// Every addition is written a = a + b.
//
// Streaming launch.  A vector of n_pad rows is cut into chunks of EC3D_TILE rows; G = ec3d_stream_wgs(n_pad) workgroups,
// workgroup b takes the chunks b, b + G, ..., thread t the rows 2t and 2t + 1 of a chunk as one 16-byte access:
//     for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
//         const int64_t r = stream_chunk_row(ch);
//         ...
//     }
// Rows r >= n -- the padding up to n_pad, which a bad solve may have left as 0 + NaN * 0 in the work vectors -- enter
// every sum as +0.0 (stream_mask) and are never stored (stream_store).
#pragma once
#include "ec3d_internal.hpp"

#define EC3D_STREAM_WGS 1024 /* workgroups of a streaming launch, at most */

inline int ec3d_stream_wgs(int64_t n_pad) { return (int)std::min<int64_t>(n_pad / EC3D_TILE, EC3D_STREAM_WGS); }

typedef double stream_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int64_t stream_chunk_row(int64_t ch) { return ch * EC3D_TILE + 2 * (int64_t)threadIdx.x; }

// rows r and r + 1 as stored (r even, r + 1 < n_pad: inside every vector)
__device__ __forceinline__ stream_d2 stream_load(const double *p, int64_t r) { return *reinterpret_cast<const stream_d2 *>(p + r); }
__device__ __forceinline__ stream_d2 stream_mask(stream_d2 v, int64_t r, int64_t n)
{
    if (r >= n) v.x = 0.0;
    if (r + 1 >= n) v.y = 0.0;
    return v;
}
__device__ __forceinline__ void stream_store(double *p, int64_t r, int64_t n, stream_d2 v)
{
    if (r + 1 < n) *reinterpret_cast<stream_d2 *>(p + r) = v;
    else if (r < n) p[r] = v.x;
}

// NV sums over a workgroup of 256 threads, valid in thread 0.  lds: NV * 4 doubles, free again on return.
template <int NV> __device__ __forceinline__ void stream_block_sum(double (&v)[NV], double *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double t = v[k];
        for (int o = 32; o > 0; o >>= 1) t = t + __shfl_down(t, o, 64);
        if (lane == 0) lds[k * 4 + w] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = (((0.0 + lds[k * 4 + 0]) + lds[k * 4 + 1]) + lds[k * 4 + 2]) + lds[k * 4 + 3];
    }
    __syncthreads();
}
__device__ __forceinline__ double stream_block_sum(double v, double *lds)
{
    double a[1] = {v};
    stream_block_sum<1>(a, lds);
    return a[0];
}

// The collapse step's own terms: v[c] = entries t, t + 256, ... (< count) of sum c, added in order from 0.0; entry i of
// sum c at part[c * sum_stride + i * entry_stride].  stream_block_sum follows.
template <int NV>
__device__ __forceinline__ void stream_strided_sum(double (&v)[NV], const double *__restrict__ part, int64_t count,
                                                   int64_t sum_stride, int64_t entry_stride = 1)
{
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += EC3D_THREADS) {
#pragma unroll
        for (int c = 0; c < NV; ++c) v[c] = v[c] + part[c * sum_stride + i * entry_stride];
    }
}
__device__ __forceinline__ double stream_strided_sum(const double *__restrict__ part, int64_t count)
{
    double a[1];
    stream_strided_sum<1>(a, part, count, 0);
    return a[0];
}
