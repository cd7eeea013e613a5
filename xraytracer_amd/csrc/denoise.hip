// denoise.hip — the two a-trous wavelet filters over a frame and its first-hit guide buffers:
//   plain (xrt_denoise; Dammertz et al. 2010): `iterations` passes of a 5 x 5 B3-spline kernel with
//     tap spacing s = 1, 2, 4, ...; each tap is weighted by how far colour, shading normal, depth and
//     albedo are from the centre pixel's and cut to zero across an object-id boundary;
//   var (xrt_denoise_var; the spatial filter of SVGF, Schied et al. 2017): the same passes with the
//     absolute colour stop replaced by a luminance difference measured in standard deviations of the
//     centre pixel's noise, and the per-pixel variance filtered along with the colour.
// include/xrt.h states the arithmetic operation for operation; dnv_estimate's loop, dn_kl, dn_tap and
// dn_pixel below are that statement, and both filter kernels run the latter three, so they agree bit
// for bit with each other and with the float32 restatements in tests/denoise_restatement.py and
// tests/denoise_var_restatement.py (expf is device_math.h's glibc_expf).
//
// k_dn_pack gathers the caller's planes once into three 16-byte records per pixel,
//   col = {c.r, c.g, c.b, var}   nrm = {n.x, n.y, n.z, object bits}   alb = {a.r, a.g, a.b, depth}
// (a NULL plane packs as zeros; the plain filter has no variance and carries +0), so a tap is three
// 16-byte loads, each filter has one form, and the caller's colour and variance have been read in
// full before anything is written: out may be the colour buffer and out_variance the variance
// buffer.  The variance changes per pass, so it lives with the colour and the depth with the albedo.
// k_dnv_estimate (var, only when the caller gives no variance) reads the packed rgb and the object
// ids and writes the OTHER col buffer whole, {rgb, estimate}: no lane reads a word the launch
// writes.  Every iteration reads col and writes the other of two col buffers; the last one writes
// the caller's packed float3 image and (var) variance plane instead.
//
// k_dn_direct<VAR>: one lane per pixel, 32 x 8 pixels per block, taps from global memory (the
// frame's records stay in L2 / the Infinity Cache).  k_dn_tiled<VAR, S>: the same block first stages
// its tile and a halo of 2 S pixels of all three records in LDS and takes the 25 taps from there;
// the halo of 2 S >= 2 pixels covers the 3 x 3 variance prefilter.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "launch.h"

namespace xrt {

constexpr int kDnvMaxRadius = XRT_DENOISE_VAR_MAX_RADIUS;

struct DnPix {
    f4 c, n, a;   // the three records of one pixel
};

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// var: the luminance factor of centre pixel p from the 3 x 3 Gaussian of the variance round it, taps
// in the order dy outer, dx inner, those outside the image skipped; var(dx, dy) is the variance at
// (x + dx, y + dy)
template <typename Var>
__device__ __forceinline__ float dn_kl(int x, int y, int w, int h, float sigma_l, Var&& var) {
    if (!(sigma_l > 0.0f)) return 0.0f;
    constexpr float kG[3] = {0.25f, 0.5f, 0.25f};
    float vs = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (x + dx < 0 || x + dx >= w) continue;
            const float gw = kG[dy + 1] * kG[dx + 1];
            vs = vs + var(dx, dy) * gw;
            gs = gs + gw;
        }
    }
    const float vg = vs / gs;
    return 1.0f / (sigma_l * __builtin_sqrtf(vg) + 1e-8f);
}

// one tap q of centre p: its weight into ws, its weighted colour into acc and (var) its variance
// under the squared weight into vacc.  k0 is the factor on the colour stop: plain K.k0 on the squared
// colour distance, var the luminance factor on |lp - luminance of q|, lp being p's luminance.
template <bool VAR>
__device__ __forceinline__ void dn_tap(const DnPix& p, float lp, float k0, const DnPix& q, float hw, const DenoiseK& K, v3& acc,
                                       float& vacc, float& ws) {
    float d0;
    if constexpr (VAR) {
        d0 = __builtin_fabsf(lp - dn_lum(q.c.x, q.c.y, q.c.z));
    } else {
        const float cx = p.c.x - q.c.x, cy = p.c.y - q.c.y, cz = p.c.z - q.c.z;
        d0 = (cx * cx + cy * cy) + cz * cz;
    }
    const float nx = p.n.x - q.n.x, ny = p.n.y - q.n.y, nz = p.n.z - q.n.z;
    const float d2n = (nx * nx + ny * ny) + nz * nz;
    const float ax = p.a.x - q.a.x, ay = p.a.y - q.a.y, az = p.a.z - q.a.z;
    const float d2a = (ax * ax + ay * ay) + az * az;
    const float dz = p.a.w - q.a.w;
    const float d2z = dz * dz;
    const float e = ((d0 * k0 + d2n * K.kn) + d2z * K.kz) + d2a * K.ka;
    float w = glibc_expf(-e) * hw;
    if (__float_as_uint(p.n.w) != __float_as_uint(q.n.w)) w = 0.0f;   // another object
    acc.x = acc.x + q.c.x * w;
    acc.y = acc.y + q.c.y * w;
    acc.z = acc.z + q.c.z * w;
    if constexpr (VAR) vacc = vacc + q.c.w * (w * w);
    ws = ws + w;
}

// the 25 taps of pixel (x, y) in the order dy outer, dx inner; taps outside the image are skipped;
// fetch(dx, dy) returns the records of the pixel at (x + s dx, y + s dy).  Returns {colour, variance
// (plain: +0)}.
template <bool VAR, typename Fetch>
__device__ __forceinline__ f4 dn_pixel(const DnPix& p, float k0, int x, int y, int w, int h, int s, const DenoiseK& K, Fetch&& fetch) {
    constexpr float kH[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float lp = VAR ? dn_lum(p.c.x, p.c.y, p.c.z) : 0.0f;
    v3 acc = mk(0.0f, 0.0f, 0.0f);
    float vacc = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= w) continue;
            dn_tap<VAR>(p, lp, k0, fetch(dx, dy), kH[dy + 2] * kH[dx + 2], K, acc, vacc, ws);
        }
    }
    return make_float4(acc.x / ws, acc.y / ws, acc.z / ws, VAR ? vacc / (ws * ws) : 0.0f);
}

// the iteration's result for pixel i: a col record for the next iteration, or the caller's planes
__device__ __forceinline__ void dn_store(const DenoiseIter& I, size_t i, f4 r) {
    if (I.out3) {
        I.out3[3 * i] = r.x, I.out3[3 * i + 1] = r.y, I.out3[3 * i + 2] = r.z;
        if (I.outv) I.outv[i] = r.w;
    } else {
        I.cout[i] = r;
    }
}

__global__ __launch_bounds__(256) void k_dn_pack(const float* __restrict__ color, const float* __restrict__ variance,
                                                 const float* __restrict__ albedo, const float* __restrict__ normal,
                                                 const float* __restrict__ depth, const int32_t* __restrict__ object,
                                                 size_t npix, f4* __restrict__ col, f4* __restrict__ nrm, f4* __restrict__ alb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    col[i] = make_float4(color[3 * i], color[3 * i + 1], color[3 * i + 2], variance ? variance[i] : 0.0f);
    const float ob = __int_as_float(object ? object[i] : 0);
    nrm[i] = normal ? make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], ob) : make_float4(0.0f, 0.0f, 0.0f, ob);
    const float z = depth ? depth[i] : 0.0f;
    alb[i] = albedo ? make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], z) : make_float4(0.0f, 0.0f, 0.0f, z);
}

// The variance estimate: the block stages {luminance, object bits} of its 32 x 8 tile and a halo of
// 3 pixels in LDS (38 x 14 x 8 B = 4,256 B); a lane then takes the (2 r + 1)^2 taps of its pixel
// from there.  cin is read, cout (another buffer) is written whole.
__global__ __launch_bounds__(kDnBlock) void k_dnv_estimate(const f4* __restrict__ cin, const f4* __restrict__ nrm,
                                                           f4* __restrict__ cout, int w, int h, int r) {
    constexpr int HS = kDnvMaxRadius, LW = kDnTileW + 2 * HS, LH = kDnTileH + 2 * HS;
    __shared__ float2 sl[LW * LH];
    const int x0 = (int)blockIdx.x * kDnTileW - HS, y0 = (int)blockIdx.y * kDnTileH - HS;
    for (int k = (int)threadIdx.x; k < LW * LH; k += kDnBlock) {
        const int gx = x0 + k % LW, gy = y0 + k / LW;
        float2 v = make_float2(0.0f, 0.0f);   // outside the image: never a tap
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = (size_t)gx + (size_t)w * gy;
            const f4 c = cin[g];
            v = make_float2(dn_lum(c.x, c.y, c.z), nrm[g].w);
        }
        sl[k] = v;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const int x = x0 + HS + tx, y = y0 + HS + ty;
    if (x >= w || y >= h) return;
    const int l = (tx + HS) + LW * (ty + HS);
    const uint32_t ob = __float_as_uint(sl[l].y);
    float n = 0.0f, m1 = 0.0f, m2 = 0.0f;
    for (int dy = -r; dy <= r; ++dy) {   // r <= HS: inside the staged halo
        if (y + dy < 0 || y + dy >= h) continue;
        for (int dx = -r; dx <= r; ++dx) {
            if (x + dx < 0 || x + dx >= w) continue;
            const float2 q = sl[l + dx + LW * dy];
            if (__float_as_uint(q.y) != ob) continue;
            n = n + 1.0f;
            m1 = m1 + q.x;
            m2 = m2 + q.x * q.x;
        }
    }
    const float mean = m1 / n;
    const float v = m2 / n - mean * mean;
    const size_t i = (size_t)x + (size_t)w * y;
    const f4 c = cin[i];
    cout[i] = make_float4(c.x, c.y, c.z, v > 0.0f ? v : 0.0f);
}

template <bool VAR>
__global__ __launch_bounds__(kDnBlock) void k_dn_direct(DenoiseIter I) {
    const int x = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x % kDnTileW);
    const int y = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
    const int w = (int)I.width, h = (int)I.height, s = I.step;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)x + (size_t)w * y;
    const DnPix p{I.cin[i], I.nrm[i], I.alb[i]};
    float k0 = I.K.k0;
    if constexpr (VAR)
        k0 = dn_kl(x, y, w, h, I.K.k0, [&](int dx, int dy) {
            return I.cin[(size_t)(x + dx) + (size_t)w * (y + dy)].w;   // inside the image (dn_kl)
        });
    const f4 r = dn_pixel<VAR>(p, k0, x, y, w, h, s, I.K, [&](int dx, int dy) {
        const size_t q = (size_t)(x + s * dx) + (size_t)w * (y + s * dy);   // inside the image (dn_pixel)
        return DnPix{I.cin[q], I.nrm[q], I.alb[q]};
    });
    dn_store(I, i, r);
}

// S = I.step.  LDS: three planes of (32 + 4 S) x (8 + 4 S) records, one 16-byte record per lane
// and load, rows of consecutive lanes contiguous: 20,736 B (S = 1), 30,720 B (S = 2).  At S = 4 the
// halo is 3.5 times the tile and the direct kernel is faster, so there is no such form.
template <bool VAR, int S>
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
    float k0 = I.K.k0;
    if constexpr (VAR) k0 = dn_kl(x, y, w, h, I.K.k0, [&](int dx, int dy) { return sc[l + dx + LW * dy].w; });   // 1 <= HS
    const f4 r = dn_pixel<VAR>(p, k0, x, y, w, h, S, I.K, [&](int dx, int dy) {
        const int q = l + S * dx + LW * S * dy;   // |S dx|, |S dy| <= HS: inside the staged halo
        return DnPix{sc[q], sn[q], sa[q]};
    });
    dn_store(I, (size_t)x + (size_t)w * y, r);
}

static dim3 dn_grid(uint32_t width, uint32_t height) {
    return dim3((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
}

hipError_t launch_denoise_pack(const float* color, const float* variance, const float* albedo, const float* normal,
                               const float* depth, const int32_t* object, size_t npix, f4* col, f4* nrm, f4* alb,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_dn_pack, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, color, variance, albedo, normal, depth,
                       object, npix, col, nrm, alb);
    return hipGetLastError();
}

hipError_t launch_dnv_estimate(const f4* cin, const f4* nrm, f4* cout, uint32_t width, uint32_t height, int radius,
                               hipStream_t st) {
    if (radius < 1 || radius > kDnvMaxRadius || cin == cout) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dnv_estimate, dn_grid(width, height), dim3(kDnBlock), 0, st, cin, nrm, cout, (int)width, (int)height,
                       radius);
    return hipGetLastError();
}

bool denoise_has_tiled(int step) { return step == 1 || step == 2; }

hipError_t launch_denoise_iter(DenoiseFilter filter, const DenoiseIter& I, bool tiled, hipStream_t st) {
    // [filter][0 = direct, S = tiled with step S]
    static void (*const kernel[2][3])(DenoiseIter) = {{k_dn_direct<false>, k_dn_tiled<false, 1>, k_dn_tiled<false, 2>},
                                                      {k_dn_direct<true>, k_dn_tiled<true, 1>, k_dn_tiled<true, 2>}};
    if (tiled && !denoise_has_tiled(I.step)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel[filter == DenoiseFilter::Var][tiled ? I.step : 0], dn_grid(I.width, I.height), dim3(kDnBlock), 0,
                       st, I);
    return hipGetLastError();
}

}  // namespace xrt
