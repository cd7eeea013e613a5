// denoise_var.hip — the variance-guided a-trous filter (xrt_denoise_var; the spatial filter of SVGF,
// Schied et al. 2017): denoise.hip's 5 x 5 B3-spline passes with the absolute colour stop replaced by
// a luminance difference measured in standard deviations of the centre pixel's noise, and the
// per-pixel variance filtered along with the colour.  include/xrt.h states the arithmetic operation
// for operation; dnv_estimate_pixel, dnv_tap and dnv_pixel below are that statement, both filter
// kernels run the latter two, so they agree bit for bit with each other and with the float32
// restatement in tests/denoise_var_restatement.py.
//
// The variance changes per pass, so it lives with the colour; the depth moves to the albedo record:
//   col = {c.r, c.g, c.b, var}   nrm = {n.x, n.y, n.z, object bits}   alb = {a.r, a.g, a.b, depth}
// A tap is three 16-byte loads, as in denoise.hip.  k_dnv_pack gathers the caller's planes (a NULL
// plane packs as zeros), so colour and variance have been read in full before anything is written:
// out may be the colour buffer and out_variance the variance buffer.  k_dnv_estimate (only when the
// caller gives no variance) reads the packed rgb and the object ids and writes the OTHER col buffer
// whole, {rgb, estimate}: no lane reads a word the launch writes.  Every iteration reads col and
// writes the other col buffer; the last one writes the caller's float3 image and variance plane.
//
// k_dnv_direct / k_dnv_tiled<S>: one lane per pixel, 32 x 8 pixels per block, as k_dn_direct /
// k_dn_tiled<S>; the tiled form's halo of 2 S >= 2 pixels covers the 3 x 3 variance prefilter.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "launch.h"

namespace xrt {

constexpr int kDnvMaxRadius = XRT_DENOISE_VAR_MAX_RADIUS;

struct DnvPix {
    f4 c, n, a;   // the three records of one pixel
};

__device__ __forceinline__ float dnv_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the luminance factor of centre pixel p from the 3 x 3 Gaussian of the variance round it, taps in
// the order dy outer, dx inner, those outside the image skipped; var(dx, dy) is the variance at
// (x + dx, y + dy)
template <typename Var>
__device__ __forceinline__ float dnv_kl(int x, int y, int w, int h, float sigma_l, Var&& var) {
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

// one tap q of centre p (luminance lp, luminance factor kl): its weight into ws, its weighted
// colour into acc, its variance under the squared weight into vacc
__device__ __forceinline__ void dnv_tap(const DnvPix& p, float lp, float kl, const DnvPix& q, float hw, const DnvK& K, v3& acc,
                                        float& vacc, float& ws) {
    const float dl = __builtin_fabsf(lp - dnv_lum(q.c.x, q.c.y, q.c.z));
    const float nx = p.n.x - q.n.x, ny = p.n.y - q.n.y, nz = p.n.z - q.n.z;
    const float d2n = (nx * nx + ny * ny) + nz * nz;
    const float ax = p.a.x - q.a.x, ay = p.a.y - q.a.y, az = p.a.z - q.a.z;
    const float d2a = (ax * ax + ay * ay) + az * az;
    const float dz = p.a.w - q.a.w;
    const float d2z = dz * dz;
    const float e = ((dl * kl + d2n * K.kn) + d2z * K.kz) + d2a * K.ka;
    float w = glibc_expf(-e) * hw;
    if (__float_as_uint(p.n.w) != __float_as_uint(q.n.w)) w = 0.0f;   // another object
    acc.x = acc.x + q.c.x * w;
    acc.y = acc.y + q.c.y * w;
    acc.z = acc.z + q.c.z * w;
    vacc = vacc + q.c.w * (w * w);
    ws = ws + w;
}

// the 25 taps of pixel (x, y) in the order dy outer, dx inner; taps outside the image are skipped;
// fetch(dx, dy) returns the records of the pixel at (x + s dx, y + s dy).  Returns {colour, variance}.
template <typename Fetch>
__device__ __forceinline__ f4 dnv_pixel(const DnvPix& p, float kl, int x, int y, int w, int h, int s, const DnvK& K, Fetch&& fetch) {
    constexpr float kH[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float lp = dnv_lum(p.c.x, p.c.y, p.c.z);
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
            dnv_tap(p, lp, kl, fetch(dx, dy), kH[dy + 2] * kH[dx + 2], K, acc, vacc, ws);
        }
    }
    return make_float4(acc.x / ws, acc.y / ws, acc.z / ws, vacc / (ws * ws));
}

// the iteration's result for pixel i: a col record for the next iteration, or the caller's planes
__device__ __forceinline__ void dnv_store(const DnvIter& I, size_t i, f4 r) {
    if (I.out3) {
        I.out3[3 * i] = r.x, I.out3[3 * i + 1] = r.y, I.out3[3 * i + 2] = r.z;
        if (I.outv) I.outv[i] = r.w;
    } else {
        I.cout[i] = r;
    }
}

__global__ __launch_bounds__(256) void k_dnv_pack(const float* __restrict__ color, const float* __restrict__ variance,
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
            v = make_float2(dnv_lum(c.x, c.y, c.z), nrm[g].w);
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

__global__ __launch_bounds__(kDnBlock) void k_dnv_direct(DnvIter I) {
    const int x = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x % kDnTileW);
    const int y = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
    const int w = (int)I.width, h = (int)I.height, s = I.step;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)x + (size_t)w * y;
    const DnvPix p{I.cin[i], I.nrm[i], I.alb[i]};
    const float kl = dnv_kl(x, y, w, h, I.K.sl, [&](int dx, int dy) {
        return I.cin[(size_t)(x + dx) + (size_t)w * (y + dy)].w;   // inside the image (dnv_kl)
    });
    const f4 r = dnv_pixel(p, kl, x, y, w, h, s, I.K, [&](int dx, int dy) {
        const size_t q = (size_t)(x + s * dx) + (size_t)w * (y + s * dy);   // inside the image (dnv_pixel)
        return DnvPix{I.cin[q], I.nrm[q], I.alb[q]};
    });
    dnv_store(I, i, r);
}

// S = I.step.  LDS as k_dn_tiled<S>: three planes of (32 + 4 S) x (8 + 4 S) records, 20,736 B (S = 1),
// 30,720 B (S = 2).
template <int S>
__global__ __launch_bounds__(kDnBlock) void k_dnv_tiled(DnvIter I) {
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
    const DnvPix p{sc[l], sn[l], sa[l]};
    const float kl = dnv_kl(x, y, w, h, I.K.sl, [&](int dx, int dy) { return sc[l + dx + LW * dy].w; });   // 1 <= HS
    const f4 r = dnv_pixel(p, kl, x, y, w, h, S, I.K, [&](int dx, int dy) {
        const int q = l + S * dx + LW * S * dy;   // |S dx|, |S dy| <= HS: inside the staged halo
        return DnvPix{sc[q], sn[q], sa[q]};
    });
    dnv_store(I, (size_t)x + (size_t)w * y, r);
}

hipError_t launch_dnv_pack(const float* color, const float* variance, const float* albedo, const float* normal,
                           const float* depth, const int32_t* object, size_t npix, f4* col, f4* nrm, f4* alb, hipStream_t st) {
    hipLaunchKernelGGL(k_dnv_pack, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, color, variance, albedo, normal, depth,
                       object, npix, col, nrm, alb);
    return hipGetLastError();
}

hipError_t launch_dnv_estimate(const f4* cin, const f4* nrm, f4* cout, uint32_t width, uint32_t height, int radius,
                               hipStream_t st) {
    if (radius < 1 || radius > kDnvMaxRadius || cin == cout) return hipErrorInvalidValue;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH), block(kDnBlock);
    hipLaunchKernelGGL(k_dnv_estimate, grid, block, 0, st, cin, nrm, cout, (int)width, (int)height, radius);
    return hipGetLastError();
}

bool dnv_has_tiled(int step) { return step == 1 || step == 2; }

hipError_t launch_dnv_iter(const DnvIter& I, bool tiled, hipStream_t st) {
    const dim3 grid((I.width + kDnTileW - 1) / kDnTileW, (I.height + kDnTileH - 1) / kDnTileH), block(kDnBlock);
    if (tiled && !dnv_has_tiled(I.step)) return hipErrorInvalidValue;
    if (!tiled) hipLaunchKernelGGL(k_dnv_direct, grid, block, 0, st, I);
    else if (I.step == 1) hipLaunchKernelGGL(k_dnv_tiled<1>, grid, block, 0, st, I);
    else hipLaunchKernelGGL(k_dnv_tiled<2>, grid, block, 0, st, I);
    return hipGetLastError();
}

}  // namespace xrt
