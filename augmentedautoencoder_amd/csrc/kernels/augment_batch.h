// Dataset.batch as one launch: one workgroup per batch image, the image held in LDS from the composite to the store.
//
// LDS: two buffers of ceil(H*W*C / 4) dwords in the interleaved [H][W][C] byte order of the global arrays, no padding.  The
// composite, the pointwise ops and the store move one dword (four consecutive bytes) per lane: consecutive lanes touch consecutive
// banks.  The spatial ops (affine, blur) gather single bytes from one buffer (ds_read_u8) and write whole dwords into the other; the
// 32 lanes of a half-wave cover 128 consecutive output bytes, so a blur tap reads a span of 32-33 consecutive dwords (at most two
// lanes' dwords on one bank) and the affine a span of 128 / scale bytes.  The buffers swap after a spatial op.
//
// The program of an image (op codes, parameters, aux offsets) is the same for every lane.  Every read-only array is a
// `const T* __restrict__` kernel parameter, so the blockIdx-indexed reads of the indices, the op count and the 32-byte op records are
// scalar loads; each op dword additionally passes through readfirstlane, which pins it to an SGPR whatever the compiler proved.  The
// op switch is a scalar branch.  A blur's k weights are read into SGPRs before the pixel loop and the tap loops are unrolled for
// the op's k (aug_blur_dispatch), so the tap loop holds LDS byte gathers and FMAs only, no global load.
//
// Nothing a device-resident index can say makes a lane leave its buffers: an image whose training or background index is out of
// range is left unwritten, an op whose table or weight range does not lie inside the aux pool is skipped, a mask bit outside
// the pool reads as "kept".
#pragma once

#include <hip/hip_runtime.h>

#include "augment_core.h"

namespace aae_augment {

constexpr int AUG_BLOCK = 1024;

struct AugDims {
    int N, M, H, W, C, aux_words;
    float rcp_C, rcp_W;
    int vec4;                    // H*W*C % 4 == 0 and every image pointer 16-byte aligned: dword loads, float4 stores
};

__device__ __forceinline__ int aug_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float aug_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// bytes [4i, 4i+4) of an image of `total` bytes as one dword; bytes past the end read as 0
__device__ __forceinline__ uint32_t aug_load4(const uint8_t* __restrict__ img, int i, int total, int vec4) {
    if (vec4) return reinterpret_cast<const uint32_t*>(img)[i];
    uint32_t v = 0;
    for (int j = 0; j < 4; ++j)
        if (4 * i + j < total) v |= (uint32_t)img[4 * i + j] << (8 * j);
    return v;
}

__device__ __forceinline__ void aug_store4_unit(float* __restrict__ out, int i, int total, int vec4, uint32_t v) {
    if (vec4) {
        reinterpret_cast<float4*>(out)[i] = make_float4(aug_unit(v & 255u), aug_unit((v >> 8) & 255u), aug_unit((v >> 16) & 255u), aug_unit(v >> 24));
        return;
    }
    for (int j = 0; j < 4; ++j)
        if (4 * i + j < total) out[4 * i + j] = aug_unit((v >> (8 * j)) & 255u);
}

__device__ __forceinline__ void aug_store4_u8(uint8_t* __restrict__ out, int i, int total, int vec4, uint32_t v) {
    if (vec4) {
        reinterpret_cast<uint32_t*>(out)[i] = v;
        return;
    }
    for (int j = 0; j < 4; ++j)
        if (4 * i + j < total) out[4 * i + j] = (uint8_t)(v >> (8 * j));
}

// a pointwise op over the whole buffer, in place: fn(value, channel) -> value
template <class Fn>
__device__ __forceinline__ void aug_pointwise_pass(uint32_t* buf, int nd, int C, float rcp_C, const Fn& fn) {
    for (int i = threadIdx.x; i < nd; i += AUG_BLOCK) {
        int pix, c;
        aug_divmod(4 * i, C, rcp_C, &pix, &c);
        const uint32_t v = buf[i];
        uint32_t o = 0;
        for (int j = 0; j < 4; ++j) {
            o |= (uint32_t)fn((uint8_t)(v >> (8 * j)), c) << (8 * j);
            c = c + 1 == C ? 0 : c + 1;
        }
        buf[i] = o;
    }
}

// a spatial op from src into dst: fn(y, x, c) -> value.  Bytes past the end of the image are written as 0.
template <class Fn>
__device__ __forceinline__ void aug_spatial_pass(uint32_t* dst, int nd, int total, int W, int C, float rcp_W, float rcp_C, const Fn& fn) {
    for (int i = threadIdx.x; i < nd; i += AUG_BLOCK) {
        int pix, c, y, x;
        aug_divmod(4 * i, C, rcp_C, &pix, &c);
        aug_divmod(pix, W, rcp_W, &y, &x);
        uint32_t o = 0;
        for (int j = 0; j < 4; ++j) {
            if (4 * i + j < total) o |= (uint32_t)fn(y, x, c) << (8 * j);
            if (++c == C) {
                c = 0;
                if (++x == W) { x = 0; ++y; }
            }
        }
        dst[i] = o;
    }
}

// train_x / train_y [N,H,W,C], mask_x [N,H,W] (non-zero = background), bg [M,H,W,C]; train_idx / bg_idx / n_ops [B]; ops
// [B,AUG_MAX_OPS]; aux [aux_words]; out_u8 / out_x / out_y [B,H,W,C], each may be null
__global__ __launch_bounds__(AUG_BLOCK) void augment_batch_kernel(const uint8_t* __restrict__ train_x, const uint8_t* __restrict__ mask_x,
                                                                  const uint8_t* __restrict__ train_y, const uint8_t* __restrict__ bg,
                                                                  const int32_t* __restrict__ train_idx, const int32_t* __restrict__ bg_idx,
                                                                  const int32_t* __restrict__ n_ops_in, const AugOp* __restrict__ ops_in,
                                                                  const uint32_t* __restrict__ aux, uint8_t* __restrict__ out_u8,
                                                                  float* __restrict__ out_x, float* __restrict__ out_y, const AugDims a) {
    extern __shared__ uint32_t aug_lds[];
    const int b = blockIdx.x;
    const int H = a.H, W = a.W, C = a.C;
    const int total = H * W * C, nd = (total + 3) >> 2;
    const int ti = aug_uniform(train_idx[b]), bi = aug_uniform(bg_idx[b]);
    if ((unsigned)ti >= (unsigned)a.N || (unsigned)bi >= (unsigned)a.M) return;
    const uint8_t* __restrict__ tx = train_x + (size_t)ti * total;
    const uint8_t* __restrict__ mk = mask_x + (size_t)ti * (H * W);
    const uint8_t* __restrict__ bgp = bg + (size_t)bi * total;

    if (out_y) {
        const uint8_t* __restrict__ ty = train_y + (size_t)ti * total;
        float* __restrict__ oy = out_y + (size_t)b * total;
        for (int i = threadIdx.x; i < nd; i += AUG_BLOCK) aug_store4_unit(oy, i, total, a.vec4, aug_load4(ty, i, total, a.vec4));
    }
    if (!out_u8 && !out_x) return;

    uint32_t* cur = aug_lds;
    uint32_t* other = aug_lds + nd;
    for (int i = threadIdx.x; i < nd; i += AUG_BLOCK) {
        const uint32_t o = aug_load4(tx, i, total, a.vec4), g = aug_load4(bgp, i, total, a.vec4);
        int pix, c;
        aug_divmod(4 * i, C, a.rcp_C, &pix, &c);
        uint32_t v = 0;
        for (int j = 0; j < 4; ++j) {
            const uint8_t m = 4 * i + j < total ? mk[pix] : (uint8_t)0;
            v |= (uint32_t)aug_composite((uint8_t)(o >> (8 * j)), (uint8_t)(g >> (8 * j)), m) << (8 * j);
            if (++c == C) { c = 0; ++pix; }
        }
        cur[i] = v;
    }
    __syncthreads();

    int n_ops = aug_uniform(n_ops_in[b]);
    n_ops = n_ops < 0 ? 0 : (n_ops > AUG_MAX_OPS ? AUG_MAX_OPS : n_ops);
    const AugOp* __restrict__ ops = ops_in + (size_t)b * AUG_MAX_OPS;
    for (int k = 0; k < n_ops; ++k) {
        // the op in SGPRs
        const int code = aug_uniform(ops[k].code);
        const int i0 = aug_uniform(ops[k].i[0]), i1 = aug_uniform(ops[k].i[1]), i2 = aug_uniform(ops[k].i[2]), i3 = aug_uniform(ops[k].i[3]);
        const float f0 = aug_uniform(ops[k].f[0]), f1 = aug_uniform(ops[k].f[1]), f2 = aug_uniform(ops[k].f[2]);
        const uint8_t* src = reinterpret_cast<const uint8_t*>(cur);
        auto at = [&](int y, int x, int c) -> uint8_t { return src[(y * W + x) * C + c]; };
        auto pick_f = [&](int c) -> float { return c == 0 ? f0 : (c == 1 ? f1 : f2); };
        auto pick_i = [&](int c) -> int { return c == 0 ? i0 : (c == 1 ? i1 : i2); };
        bool swap = false;
        if (code == AUG_AFFINE) {
            aug_spatial_pass(other, nd, total, W, C, a.rcp_W, a.rcp_C, [&](int y, int x, int c) { return aug_affine_pixel(at, y, x, c, H, W, f0); });
            swap = true;
        } else if (code == AUG_BLUR) {
            const int kk = i0, w0 = i1;
            if (kk >= 1 && kk <= AUG_MAX_BLUR_K && (kk >> 1) < H && (kk >> 1) < W && w0 >= 0 && w0 <= a.aux_words - kk)
                swap = aug_blur_dispatch(kk, [&](auto K) {
                    float w[K.value];
                    AUG_UNROLL
                    for (int t = 0; t < K.value; ++t) w[t] = aug_uniform(__uint_as_float(aux[w0 + t]));
                    aug_spatial_pass(other, nd, total, W, C, a.rcp_W, a.rcp_C, [&](int y, int x, int c) { return aug_blur_pixel<K.value>(at, w, y, x, c, H, W); });
                });
        } else if (code == AUG_DROPOUT) {
            const int m0 = i0, r0 = i1, c0 = i2, plane = i3;
            if (m0 >= 0 && r0 >= 0 && c0 >= 0 && plane >= 0 && r0 <= a.aux_words - H && c0 <= a.aux_words - W) {
                const uint32_t words = a.aux_words > m0 ? (uint32_t)(a.aux_words - m0) : 0u;
                auto bit_set = [&](uint32_t bit) -> bool { return (bit >> 5) < words && ((aux[m0 + (bit >> 5)] >> (bit & 31u)) & 1u); };
                aug_spatial_pass(other, nd, total, W, C, a.rcp_W, a.rcp_C,
                                 [&](int y, int x, int c) { return aug_dropout_pixel(at(y, x, c), bit_set, aux[r0 + y], aux[c0 + x], c, (uint32_t)plane); });
                swap = true;
            }
        } else if (code == AUG_ADD) {
            aug_pointwise_pass(cur, nd, C, a.rcp_C, [&](uint8_t v, int c) { return aug_add(v, pick_f(c)); });
        } else if (code == AUG_INVERT) {
            aug_pointwise_pass(cur, nd, C, a.rcp_C, [&](uint8_t v, int c) { return aug_invert(v, pick_i(c)); });
        } else if (code == AUG_MULTIPLY) {
            aug_pointwise_pass(cur, nd, C, a.rcp_C, [&](uint8_t v, int c) { return aug_multiply(v, pick_f(c)); });
        } else if (code == AUG_CONTRAST) {
            aug_pointwise_pass(cur, nd, C, a.rcp_C, [&](uint8_t v, int c) { return aug_contrast(v, pick_f(c)); });
        }
        if (swap) {
            uint32_t* t = cur;
            cur = other;
            other = t;
        }
        __syncthreads();
    }

    uint8_t* __restrict__ o8 = out_u8 ? out_u8 + (size_t)b * total : nullptr;
    float* __restrict__ ox = out_x ? out_x + (size_t)b * total : nullptr;
    for (int i = threadIdx.x; i < nd; i += AUG_BLOCK) {
        const uint32_t v = cur[i];
        if (o8) aug_store4_u8(o8, i, total, a.vec4, v);
        if (ox) aug_store4_unit(ox, i, total, a.vec4, v);
    }
}

}  // namespace aae_augment
