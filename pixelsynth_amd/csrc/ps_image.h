// What the units that read a strided image batch share (metrics.hip, percsim.hip, consistency.hip, fid.hip, content_loss.hip): the
// batch as a kernel argument, TF.to_tensor's value of an element, the 2 x 2 max-pool's window (percsim.hip, content_loss.hip), PNet's
// input constants, the argument requirements and the dtype dispatch of their entry points, and the fixed-order block sum of their fp64
// partial sums.  gfx950 only.
#pragma once
#include "ps_common.h"

namespace ps {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (B, C, H, W) elements of PS_DTYPE_F32 / PS_DTYPE_U8 read in place through element strides (NCHW or channels-last storage)
struct Img {
    const void *p;
    long long sB, sC, sH, sW;            // element strides
    Img(const void *ptr, const int64_t *strides) : p(ptr), sB(strides[0]), sC(strides[1]), sH(strides[2]), sW(strides[3]) {}
};

template <typename T> __device__ __forceinline__ float to_unit(T v);
template <> __device__ __forceinline__ float to_unit<float>(float v) { return v; }
// true division, as TF.to_tensor's float().div(255) on the host (not a multiply by the reciprocal)
template <> __device__ __forceinline__ float to_unit<uint8_t>(uint8_t v) { return (float)v / 255.0f; }

// The maximum of a 2 x 2 window as F.max_pool2d gives it: NaN where the window holds one.  __builtin_elementwise_max is IEEE maxNum
// (v_max_f32), which returns its other operand for a NaN; __builtin_elementwise_maximum is IEEE 754-2019's maximum (v_maximum3_f32 on
// gfx950: two instructions a channel, as many as the maxNum took), which hands the NaN on and gives maxNum's bits for anything else.
__device__ __forceinline__ f32x4 max4_keep_nan(f32x4 a, f32x4 b, f32x4 c, f32x4 d)
{
    return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), __builtin_elementwise_maximum(c, d));
}

// PNet's shift / scale (pretrained_networks.py:45-46) as the fp32 values torch.Tensor([...]) holds.  static: a copy per unit that
// includes this header, as __constant__ data needs (no unit shares device symbols with another)
static __constant__ float c_pnet_shift[3] = {-0.030f, -0.088f, -0.188f};
static __constant__ float c_pnet_scale[3] = {0.458f, 0.448f, 0.450f};

// The requirements the entry points share, in `what`'s name: `pointers` (every pointer the call needs is there), a dtype code, a batch
// that fits one grid dimension, no negative stride (strides2: a second batch's, or NULL).  -> PS_OK, or the error as ps::fail left it
inline int require_images(const char *what, bool pointers, int dtype, int B, const int64_t *strides1, const int64_t *strides2)
{
    PS_REQUIRE(pointers, "%s: null pointer", what);
    PS_REQUIRE(dtype == PS_DTYPE_F32 || dtype == PS_DTYPE_U8, "%s: dtype must be PS_DTYPE_F32 or PS_DTYPE_U8 (got %d)", what, dtype);
    PS_REQUIRE(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 required (B = %d)", what, B);
    for (int i = 0; i < 4; ++i)
        PS_REQUIRE(strides1[i] >= 0 && (!strides2 || strides2[i] >= 0), "%s: negative stride", what);
    return PS_OK;
}

#define PS_REQUIRE_IMAGES(...)                                      \
    do {                                                            \
        if (int _rc = ps::require_images(__VA_ARGS__)) return _rc;  \
    } while (0)

// f(T()) with T the element type of a dtype code that passed require_images: the launch of a kernel template on T
template <typename F> inline void for_dtype(int dtype, F &&f)
{
    if (dtype == PS_DTYPE_F32)
        f(float());
    else
        f(uint8_t());
}

}  // namespace ps

// K sums over the N threads of a workgroup (N a power of two, tid = threadIdx.x), each thread's terms already in the LDS array
// red[k * N + tid]: afterwards red[k * N] holds sum k, added in the fixed order red[t] += red[t + h], h = N / 2, N / 4, ..., 1.
// A macro, not a function: an inlined callee is simplified on its own first, and the unrolled last steps then come out as other
// (equivalent) instructions in some kernels; as part of the kernel's own body the loop compiles the same wherever it is written.
#define PS_BLOCK_TREE_SUM(red, tid, K, N)                                                       \
    do {                                                                                        \
        __syncthreads();                                                                        \
        for (int h = (N) / 2; h > 0; h >>= 1) {                                                 \
            if ((tid) < h) {                                                                    \
                _Pragma("unroll") for (int k = 0; k < (K); ++k) (red)[k * (N) + (tid)] += (red)[k * (N) + (tid) + h]; \
            }                                                                                   \
            __syncthreads();                                                                    \
        }                                                                                       \
    } while (0)
