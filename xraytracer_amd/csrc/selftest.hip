// selftest.hip — device self-tests of the restated arithmetic (the RNG stream and its refill,
// the glibc trigonometry / log / exp / pow, the fast divisions) and of the medium's density
// lookup and samplers (medium.h's own functions, not copies), run by the test suite against the
// host's results.
#include "launch.h"
#include "medium.h"
#include "path_common.h"

namespace xrt {

// ============================================================== self-tests ====
__global__ __launch_bounds__(kBlock) void k_test_rng(const uint32_t* seeds, uint32_t n_seeds, uint32_t skip,
                                                      uint32_t n, float* out, uint32_t* rings) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < n_seeds;
    uint32_t* ring = rings + (size_t)s * kRing;
    if (valid) {
        uint32_t x = seeds[s];
        ring[0] = x;
        for (uint32_t i = 1; i < kMT; ++i) {
            x = 1812433253u * (x ^ (x >> 30)) + i;
            ring[i] = x;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    uint32_t g = kMT;
    Rng rng{ring, kMT};
    // consume skip + n draws, refilling cooperatively like k_shade does
    const uint32_t total = skip + n;
    for (uint32_t done = 0; done < total;) {
        wave_refill(valid && (g - rng.c) < kRngMin, s, g, rings, lane);
        const uint32_t chunk = min(32u, total - done);   // < kRngMin: never reads past g
        if (valid) {
            for (uint32_t q = 0; q < chunk; ++q) {
                const uint32_t idx = done + q;
                const float f = rng.next();
                if (idx >= skip) out[(size_t)s * n + (idx - skip)] = f;
            }
        }
        done += chunk;
    }
}

__global__ void k_test_trig(const float* x, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out[2 * i] = glibc_sinf(x[i]);
        out[2 * i + 1] = glibc_cosf(x[i]);
    }
}

// every float r in [0,1) with bit pattern in [first, first+count) that the sampler can
// produce (r * 2^32 integral): phi = 2*PI*r -> (sin, cos); others -> NaN marker in out_r
__global__ void k_test_trig_domain(uint32_t first, uint32_t count, float* out_sin, float* out_cos, float* out_r) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float r = __uint_as_float(first + i);
    const double sc = (double)r * 4294967296.0;
    const bool reach = r >= 0.0f && r < 1.0f && sc == __builtin_floor(sc);
    const float phi = kPI_MUL_2 * r;
    out_r[i] = reach ? r : __builtin_nanf("");
    out_sin[i] = glibc_sinf(phi);
    out_cos[i] = glibc_cosf(phi);
}

// fast-division self-test over every 32-bit pattern in [first, first + count): mode 0 checks
// rcp_rn(b) against 1.0f / b; mode 1 checks div_const(x, c, rc) against x / c.  Counts
// mismatches (NaN == NaN) and records the first 16.
__global__ void k_test_fastdiv(uint32_t mode, float c, float rc, uint32_t first, uint32_t count,
                               unsigned long long* nbad, uint32_t* bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float x = __uint_as_float(first + i);
    float f, r;
    if (mode == 0) {
        f = rcp_rn(x);
        r = 1.0f / x;
    } else {
        f = div_const(x, c, rc);
        r = x / c;
    }
    const bool same = __float_as_uint(f) == __float_as_uint(r) || (f != f && r != r);
    if (!same) {
        const unsigned long long k = atomicAdd(nbad, 1ull);
        if (k < 16) bad[k] = first + i;
    }
}

__global__ void k_test_logexp(const float* x, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out[2 * i] = glibc_logf(x[i]);
        out[2 * i + 1] = glibc_expf(x[i]);
    }
}

__global__ void k_test_powf(const float* x, uint32_t n, float y, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = glibc_powf(x[i], y);
}

// medium_density of the medium M at pts[i] = {x, y, z}, one lane per point
__global__ void k_test_density(DMedium M, const float* pts, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = medium_density(M, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
}

// hg_sample / sample_wavelength with the item's draws chosen by the caller: the stream is the
// item's own eight raw (untempered) words, cursor 0
__global__ void k_test_hg(float g, const float* wo, const uint32_t* words, uint32_t n, float* wi) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng{words + (size_t)i * 8, 0u};
    v3 w;
    hg_sample(g, mk(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]), rng, w);
    wi[3 * i] = w.x, wi[3 * i + 1] = w.y, wi[3 * i + 2] = w.z;
}

__global__ void k_test_wavelength(const float* thr, const float* albedo, const uint32_t* words, uint32_t n,
                                  uint32_t* channel, float* pmf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng{words + (size_t)i * 8, 0u};
    v3 p;
    channel[i] = sample_wavelength(mk(thr[3 * i], thr[3 * i + 1], thr[3 * i + 2]),
                                   mk(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]), rng, p);
    pmf[3 * i] = p.x, pmf[3 * i + 1] = p.y, pmf[3 * i + 2] = p.z;
}

hipError_t launch_test_rng(const uint32_t* seeds, uint32_t n_seeds, uint32_t skip, uint32_t n, float* out,
                           uint32_t* rings, hipStream_t st) {
    const uint32_t blocks = (n_seeds + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_test_rng, dim3(blocks), dim3(kBlock), 0, st, seeds, n_seeds, skip, n, out, rings);
    return hipGetLastError();
}

hipError_t launch_test_trig(const float* x, uint32_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_test_trig, dim3((n + 255) / 256), dim3(256), 0, st, x, n, out);
    return hipGetLastError();
}

hipError_t launch_test_trig_domain(uint32_t first, uint32_t count, float* s, float* c, float* r, hipStream_t st) {
    hipLaunchKernelGGL(k_test_trig_domain, dim3((count + 255) / 256), dim3(256), 0, st, first, count, s, c, r);
    return hipGetLastError();
}

hipError_t launch_test_fastdiv(uint32_t mode, float c, float rc, uint32_t first, uint32_t count,
                               unsigned long long* nbad, uint32_t* bad, hipStream_t st) {
    hipLaunchKernelGGL(k_test_fastdiv, dim3((count + 255) / 256), dim3(256), 0, st, mode, c, rc, first, count, nbad,
                       bad);
    return hipGetLastError();
}

hipError_t launch_test_logexp(const float* x, uint32_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_test_logexp, dim3((n + 255) / 256), dim3(256), 0, st, x, n, out);
    return hipGetLastError();
}

hipError_t launch_test_powf(const float* x, uint32_t n, float y, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_test_powf, dim3((n + 255) / 256), dim3(256), 0, st, x, n, y, out);
    return hipGetLastError();
}

hipError_t launch_test_density(const DMedium& M, const float* pts, uint32_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_test_density, dim3((n + 255) / 256), dim3(256), 0, st, M, pts, n, out);
    return hipGetLastError();
}

hipError_t launch_test_hg(float g, const float* wo, const uint32_t* words, uint32_t n, float* wi, hipStream_t st) {
    hipLaunchKernelGGL(k_test_hg, dim3((n + 255) / 256), dim3(256), 0, st, g, wo, words, n, wi);
    return hipGetLastError();
}

hipError_t launch_test_wavelength(const float* thr, const float* albedo, const uint32_t* words, uint32_t n,
                                  uint32_t* channel, float* pmf, hipStream_t st) {
    hipLaunchKernelGGL(k_test_wavelength, dim3((n + 255) / 256), dim3(256), 0, st, thr, albedo, words, n, channel, pmf);
    return hipGetLastError();
}

}  // namespace xrt
