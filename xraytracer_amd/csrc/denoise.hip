// denoise.hip — edge-avoiding a-trous wavelet filter over a frame and its first-hit guide buffers
// (xrt_denoise; Dammertz et al. 2010).  `iterations` passes of a 5 x 5 B3-spline kernel with tap
// spacing s = 1, 2, 4, ...; each tap is weighted by how far colour, shading normal, depth and
// albedo are from the centre pixel's and cut to zero across an object-id boundary.  include/xrt.h
// states the arithmetic operation for operation; dn_tap / dn_pixel below are that statement, and
// both filter kernels run them, so they agree bit for bit with each other and with the float32
// restatement in tests/denoise_restatement.py (expf is device_math.h's glibc_expf).
//
// k_dn_pack gathers the caller's planes once into three 16-byte records per pixel,
//   col = {c.r, c.g, c.b, depth}   nrm = {n.x, n.y, n.z, object bits}   alb = {a.r, a.g, a.b, 0}
// (a NULL plane packs as zeros), so a tap is three 16-byte loads, the filter has one form, and the
// caller's colour has been read in full before anything is written: out may be the colour buffer.
// Every iteration reads col and writes the other of two col buffers (depth carried along); the last
// one writes the caller's packed float3 image instead.
//
// k_dn_direct: one lane per pixel, 32 x 8 pixels per block, taps from global memory (the frame's
// records stay in L2 / the Infinity Cache).  k_dn_tiled<S>: the same block first stages its tile
// and a halo of 2 S pixels of all three records in LDS and takes the 25 taps from there.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "launch.h"

namespace xrt {

struct DnPix {
    f4 c, n, a;   // the three records of one pixel
};

// one tap q of centre p: its weight into ws, its weighted colour into acc
__device__ __forceinline__ void dn_tap(const DnPix& p, const DnPix& q, float hw, const DenoiseK& K, v3& acc, float& ws) {
    const float cx = p.c.x - q.c.x, cy = p.c.y - q.c.y, cz = p.c.z - q.c.z;
    const float d2c = (cx * cx + cy * cy) + cz * cz;
    const float nx = p.n.x - q.n.x, ny = p.n.y - q.n.y, nz = p.n.z - q.n.z;
    const float d2n = (nx * nx + ny * ny) + nz * nz;
    const float ax = p.a.x - q.a.x, ay = p.a.y - q.a.y, az = p.a.z - q.a.z;
    const float d2a = (ax * ax + ay * ay) + az * az;
    const float dz = p.c.w - q.c.w;
    const float d2z = dz * dz;
    const float e = ((d2c * K.kc + d2n * K.kn) + d2z * K.kz) + d2a * K.ka;
    float w = glibc_expf(-e) * hw;
    if (__float_as_uint(p.n.w) != __float_as_uint(q.n.w)) w = 0.0f;   // another object
    acc.x = acc.x + q.c.x * w;
    acc.y = acc.y + q.c.y * w;
    acc.z = acc.z + q.c.z * w;
    ws = ws + w;
}

// the 25 taps of pixel (x, y) in the order dy outer, dx inner; taps outside the image are
// skipped; fetch(dx, dy) returns the records of the pixel at (x + s dx, y + s dy)
template <typename Fetch>
__device__ __forceinline__ v3 dn_pixel(const DnPix& p, int x, int y, int w, int h, int s, const DenoiseK& K, Fetch&& fetch) {
    constexpr float kH[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    v3 acc = mk(0.0f, 0.0f, 0.0f);
    float ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= w) continue;
            dn_tap(p, fetch(dx, dy), kH[dy + 2] * kH[dx + 2], K, acc, ws);
        }
    }
    return mk(acc.x / ws, acc.y / ws, acc.z / ws);
}

// the iteration's result for pixel i: a col record for the next iteration, or the caller's image
__device__ __forceinline__ void dn_store(const DenoiseIter& I, size_t i, v3 r, float depth) {
    if (I.out3) {
        I.out3[3 * i] = r.x, I.out3[3 * i + 1] = r.y, I.out3[3 * i + 2] = r.z;
    } else {
        I.cout[i] = make_float4(r.x, r.y, r.z, depth);
    }
}

__global__ __launch_bounds__(256) void k_dn_pack(const float* __restrict__ color, const float* __restrict__ albedo,
                                                 const float* __restrict__ normal, const float* __restrict__ depth,
                                                 const int32_t* __restrict__ object, size_t npix, f4* __restrict__ col,
                                                 f4* __restrict__ nrm, f4* __restrict__ alb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    col[i] = make_float4(color[3 * i], color[3 * i + 1], color[3 * i + 2], depth ? depth[i] : 0.0f);
    const float ob = __int_as_float(object ? object[i] : 0);
    nrm[i] = normal ? make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], ob) : make_float4(0.0f, 0.0f, 0.0f, ob);
    alb[i] = albedo ? make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(kDnBlock) void k_dn_direct(DenoiseIter I) {
    const int x = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x % kDnTileW);
    const int y = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
    const int w = (int)I.width, h = (int)I.height, s = I.step;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)x + (size_t)w * y;
    const DnPix p{I.cin[i], I.nrm[i], I.alb[i]};
    const v3 r = dn_pixel(p, x, y, w, h, s, I.K, [&](int dx, int dy) {
        const size_t q = (size_t)(x + s * dx) + (size_t)w * (y + s * dy);   // inside the image (dn_pixel)
        return DnPix{I.cin[q], I.nrm[q], I.alb[q]};
    });
    dn_store(I, i, r, p.c.w);
}

// S = I.step.  LDS: three planes of (32 + 4 S) x (8 + 4 S) records, one 16-byte record per lane
// and load, rows of consecutive lanes contiguous: 20,736 B (S = 1), 30,720 B (S = 2).  At S = 4 the
// halo is 3.5 times the tile and the direct kernel is faster, so there is no such form.
template <int S>
__global__ __launch_bounds__(kDnBlock) void k_dn_tiled(DenoiseIter I) {
    constexpr int HS = 2 * S, LW = kDnTileW + 2 * HS, LH = kDnTileH + 2 * HS;
    __shared__ f4 sc[LW * LH], sn[LW * LH], sa[LW * LH];
    const int w = (int)I.width, h = (int)I.height;
    const int x0 = (int)blockIdx.x * kDnTileW - HS, y0 = (int)blockIdx.y * kDnTileH - HS;
    for (int k = (int)threadIdx.x; k < LW * LH; k += kDnBlock) {
        const int gx = x0 + k % LW, gy = y0 + k / LW;
        f4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = c, a = c;   // outside the image: never a tap
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = (size_t)gx + (size_t)w * gy;
            c = I.cin[g], n = I.nrm[g], a = I.alb[g];
        }
        sc[k] = c, sn[k] = n, sa[k] = a;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const int x = x0 + HS + tx, y = y0 + HS + ty;
    if (x >= w || y >= h) return;
    const int l = (tx + HS) + LW * (ty + HS);
    const DnPix p{sc[l], sn[l], sa[l]};
    const v3 r = dn_pixel(p, x, y, w, h, S, I.K, [&](int dx, int dy) {
        const int q = l + S * dx + LW * S * dy;   // |S dx|, |S dy| <= HS: inside the staged halo
        return DnPix{sc[q], sn[q], sa[q]};
    });
    dn_store(I, (size_t)x + (size_t)w * y, r, p.c.w);
}

hipError_t launch_denoise_pack(const float* color, const float* albedo, const float* normal, const float* depth,
                               const int32_t* object, size_t npix, f4* col, f4* nrm, f4* alb, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_pack, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, color, albedo, normal, depth, object,
                       npix, col, nrm, alb);
    return hipGetLastError();
}

bool denoise_has_tiled(int step) { return step == 1 || step == 2; }

hipError_t launch_denoise_iter(const DenoiseIter& I, bool tiled, hipStream_t st) {
    const dim3 grid((I.width + kDnTileW - 1) / kDnTileW, (I.height + kDnTileH - 1) / kDnTileH), block(kDnBlock);
    if (tiled && !denoise_has_tiled(I.step)) return hipErrorInvalidValue;
    if (!tiled) hipLaunchKernelGGL(k_dn_direct, grid, block, 0, st, I);
    else if (I.step == 1) hipLaunchKernelGGL(k_dn_tiled<1>, grid, block, 0, st, I);
    else hipLaunchKernelGGL(k_dn_tiled<2>, grid, block, 0, st, I);
    return hipGetLastError();
}

}  // namespace xrt
