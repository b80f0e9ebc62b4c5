// The training step's X-ray augmentations for MI355X (gfx950): xvr's XrayAugmentations (a kornia AugmentationSequential,
// /root/reference/src/xvr/model/augmentations.py:7-68) after its Standardize, forward only, in two launches.
// C ABI: include/xvr_sim.h (xvr_sim_augment_*).  Semantics, the recalled conventions and their knobs: DESIGN.md "Augmentations";
// the torch restatement the kernels are checked against: tests/augment_restated.py.
//
//   k_aug_clahe_lut   one workgroup per (tile, image) of the images CLAHE selects: the tile's 256-bin histogram in LDS (integer
//                     adds, exact), clip + redistribute, a one-wave prefix sum, LUT = floor(clamp(cdf * (255 / tile_px), 0, 255)).
//   k_aug_chain       one 16 x 64 output tile per workgroup: CLAHE-mapped + gamma'd values of the tile and a 2-pixel halo in LDS,
//                     then box blur + noise on the 1-pixel halo, sharpness, erasing and the border crop; each pixel written once.
//
// Every op is per image, so its flag is uniform over a workgroup.  No fused multiply-adds anywhere in this file: the noise is
// bit-equal to its host restatement and the other ops follow one fixed operation order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "xvr_drr.h"
#include "xvr_sim.h"

#pragma clang fp contract(off)

extern "C" void xvr_drr_set_last_error(const char* msg);  // drr_api.hip

namespace {

constexpr int TB = 256;
constexpr int GRID = 8;          // CLAHE tiles per side
constexpr int BINS = 256;
constexpr int OT_H = 16, OT_W = 64;                 // output tile of k_aug_chain
constexpr int A_H = OT_H + 4, A_W = OT_W + 4;       // CLAHE + gamma, halo 2
constexpr int B_H = OT_H + 2, B_W = OT_W + 2;       // blur + noise, halo 1
constexpr int A_LD = A_W + 1, B_LD = B_W + 1;       // (odd row strides: a column step is not a bank multiple)

int aug_fail(int code, const char* msg) {
    xvr_drr_set_last_error(msg);
    return code;
}

// kornia's CLAHE tiling (recalled): tile side ceil(n / 8), rounded up to even; the image is reflect-padded bottom / right to 8 tiles
__host__ __device__ inline int clahe_tile(int n) {
    const int t = (n + GRID - 1) / GRID;
    return t + (t & 1);
}

// ---------------------------------------------------------------------------------------------
// Philox-4x32-10 (Salmon et al., SC'11) + Box-Muller in doubles from + - * / sqrt alone (own log and cos series), so that the
// host restatement (tests/augment_restated.py) reproduces every bit.
// ---------------------------------------------------------------------------------------------
__device__ inline uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

__device__ inline double aug_log(double u) {   // u in (0, 1]
    int e;
    double m = frexp(u, &e);                     // [0.5, 1)
    if (m < 0.7071067811865476) { m = m * 2.0; e -= 1; }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double p = 0.047619047619047616;             // 1 / 21 ... 1 / 3, 1: 2 atanh(s) = log(m)
    p = p * s2 + 0.05263157894736842;
    p = p * s2 + 0.058823529411764705;
    p = p * s2 + 0.06666666666666667;
    p = p * s2 + 0.07692307692307693;
    p = p * s2 + 0.09090909090909091;
    p = p * s2 + 0.1111111111111111;
    p = p * s2 + 0.14285714285714285;
    p = p * s2 + 0.2;
    p = p * s2 + 0.3333333333333333;
    p = p * s2 + 1.0;
    return (double)e * 0.6931471805599453 + (2.0 * s) * p;
}

__device__ inline double aug_cos_poly(double x) {   // |x| <= pi / 4
    const double x2 = x * x;
    double p = -1.5619206968586225e-16;
    p = p * x2 + 4.779477332387385e-14;
    p = p * x2 + -1.1470745597729725e-11;
    p = p * x2 + 2.08767569878681e-09;
    p = p * x2 + -2.755731922398589e-07;
    p = p * x2 + 2.48015873015873e-05;
    p = p * x2 + -0.001388888888888889;
    p = p * x2 + 0.041666666666666664;
    p = p * x2 + -0.5;
    return p * x2 + 1.0;
}

__device__ inline double aug_sin_poly(double x) {   // |x| <= pi / 4
    const double x2 = x * x;
    double p = -8.22063524662433e-18;
    p = p * x2 + 2.8114572543455206e-15;
    p = p * x2 + -7.647163731819816e-13;
    p = p * x2 + 1.6059043836821613e-10;
    p = p * x2 + -2.505210838544172e-08;
    p = p * x2 + 2.7557319223985893e-06;
    p = p * x2 + -0.0001984126984126984;
    p = p * x2 + 0.008333333333333333;
    p = p * x2 + -0.16666666666666666;
    p = p * x2 + 1.0;
    return p * x;
}

__device__ inline double aug_cos2pi(double u) {   // cos(2 pi u), u in [0, 1) (a multiple of 2^-32: every reduction is exact)
    const double a = fabs(u >= 0.5 ? u - 1.0 : u);
    if (a <= 0.125) return aug_cos_poly(6.283185307179586 * a);
    if (a <= 0.375) return aug_sin_poly(6.283185307179586 * (0.25 - a));
    return -aug_cos_poly(6.283185307179586 * (0.5 - a));
}

__device__ inline float aug_normal(unsigned seed_lo, unsigned seed_hi, unsigned b, unsigned y, unsigned x) {
    const uint4 r = philox4x32_10(make_uint4(x, y, b, 0u), make_uint2(seed_lo, seed_hi));
    const double u1 = ((double)r.x + 1.0) * 2.3283064365386963e-10;   // (0, 1]   (2^-32)
    const double u2 = (double)r.y * 2.3283064365386963e-10;           // [0, 1)
    return (float)(sqrt(-2.0 * aug_log(u1)) * aug_cos2pi(u2));
}

// ---------------------------------------------------------------------------------------------
// CLAHE LUTs
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void k_aug_clahe_lut(const float* __restrict__ s, const float* __restrict__ params, int B, int H, int W,
                                                      int clip_per_image, unsigned char* __restrict__ lut) {
    __shared__ unsigned hist[BINS];
    __shared__ unsigned wsum[TB / 64];
    __shared__ int first;
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const float* P = params + (size_t)b * XVR_SIM_AUG_COLS;
    if (P[XVR_SIM_AUG_CLAHE] == 0.f) return;   // (uniform over the workgroup)
    hist[tid] = 0u;
    if (tid == 0) first = B;
    __syncthreads();
    float clip = P[XVR_SIM_AUG_CLIP];
    if (!clip_per_image) {   // the clip limit of the first selected image
        int f = B;
        for (int i = tid; i < B; i += TB)
            if (params[(size_t)i * XVR_SIM_AUG_COLS + XVR_SIM_AUG_CLAHE] != 0.f) { f = i; break; }
        atomicMin(&first, f);
        __syncthreads();
        clip = params[(size_t)first * XVR_SIM_AUG_COLS + XVR_SIM_AUG_CLIP];
    }
    const int TH = clahe_tile(H), TW = clahe_tile(W), px = TH * TW;
    const int y0 = (tile / GRID) * TH, x0 = (tile % GRID) * TW;
    const float* img = s + (size_t)b * H * W;
    for (int i = tid; i < px; i += TB) {
        int y = y0 + i / TW, x = x0 + i % TW;
        if (y >= H) y = 2 * (H - 1) - y;   // reflect padding (the host checks that it stays inside the image)
        if (x >= W) x = 2 * (W - 1) - x;
        const float v = img[(size_t)y * W + x];
        if (v >= 0.f && v <= 1.f) atomicAdd(&hist[min((int)(v * 256.f), BINS - 1)], 1u);   // torch.histc(bins=256, min=0, max=1)
    }
    __syncthreads();
    unsigned h = hist[tid];
    if (clip > 0.f) {
        const double mv = floor((double)clip * px / BINS);
        const unsigned maxv = mv < 1.0 ? 1u : (unsigned)mv;
        h = min(h, maxv);
        unsigned t = h;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((tid & 63) == 0) wsum[tid >> 6] = t;
        __syncthreads();
        const unsigned clipped = (unsigned)px - (wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        h += clipped / BINS + ((unsigned)tid < clipped % BINS ? 1u : 0u);
    }
    hist[tid] = h;
    __syncthreads();
    if (tid < 64) {   // one wave: lane l scans bins 4l .. 4l + 3
        const unsigned c0 = hist[4 * tid], c1 = c0 + hist[4 * tid + 1], c2 = c1 + hist[4 * tid + 2], c3 = c2 + hist[4 * tid + 3];
        unsigned run = c3;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(run, o);
            if (tid >= o) run += up;
        }
        const unsigned base = run - c3;
        const float scale = (float)(255.0 / px);
        unsigned word = 0u;
        const unsigned cs[4] = {base + c0, base + c1, base + c2, base + c3};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = fminf(fmaxf((float)cs[j] * scale, 0.f), 255.f);
            word |= (unsigned)floorf(v) << (8 * j);
        }
        reinterpret_cast<unsigned*>(lut + ((size_t)b * GRID * GRID + tile) * BINS)[tid] = word;
    }
}

// ---------------------------------------------------------------------------------------------
// The chain
// ---------------------------------------------------------------------------------------------
struct Interp {   // the two LUT rows (columns) of a pixel row (column) and the weight of the first
    int t0, t1;
    float w;
};

__device__ inline Interp clahe_axis(int y, int T) {
    const int half = T / 2, sub = y / half;
    if (sub == 0) return {0, 0, 1.f};
    if (sub >= 2 * GRID - 1) return {GRID - 1, GRID - 1, 1.f};
    const int t0 = (sub - 1) / 2, k = y - (2 * t0 + 1) * half;
    return {t0, t0 + 1, (float)(2 * half - 1 - k) / (float)(2 * half - 1)};
}

__device__ inline float clahe_map(float v, int y, int x, int TH, int TW, const unsigned char* __restrict__ L) {
    const Interp iy = clahe_axis(y, TH), ix = clahe_axis(x, TW);
    const int idx = min(max((int)(v * 255.f), 0), BINS - 1);
    const float tl = L[(iy.t0 * GRID + ix.t0) * BINS + idx], tr = L[(iy.t0 * GRID + ix.t1) * BINS + idx];
    const float bl = L[(iy.t1 * GRID + ix.t0) * BINS + idx], br = L[(iy.t1 * GRID + ix.t1) * BINS + idx];
    const float t = tr + ix.w * (tl - tr), bo = br + ix.w * (bl - br);
    return (bo + iy.w * (t - bo)) / 255.f;
}

__device__ inline int reflect(int i, int n) {   // one reflection, then clamped (positions the chain never reads from still load in bounds)
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(TB) void k_aug_chain(const float* __restrict__ s, const float* __restrict__ params,
                                                  const unsigned char* __restrict__ lut, int H, int W, float noise_std, float erase_value,
                                                  float* __restrict__ out) {
    __shared__ float A[A_H * A_LD];
    __shared__ float Bv[B_H * B_LD];
    const int b = blockIdx.z, ty0 = blockIdx.y * OT_H, tx0 = blockIdx.x * OT_W, tid = threadIdx.x;
    const float* P = params + (size_t)b * XVR_SIM_AUG_COLS;
    const bool clahe = P[XVR_SIM_AUG_CLAHE] != 0.f, gamma_on = P[XVR_SIM_AUG_GAMMA_ON] != 0.f, blur = P[XVR_SIM_AUG_BLUR] != 0.f;
    const bool noise = P[XVR_SIM_AUG_NOISE] != 0.f, sharp = P[XVR_SIM_AUG_SHARP_ON] != 0.f;
    const float gamma = P[XVR_SIM_AUG_GAMMA];
    const float* img = s + (size_t)b * H * W;
    const unsigned char* L = lut + (size_t)b * GRID * GRID * BINS;
    const int TH = clahe_tile(H), TW = clahe_tile(W);

    // 1. CLAHE, gamma on the tile + halo 2 (reflected coordinates: the blur's reflect border comes for free)
    for (int i = tid; i < A_H * A_W; i += TB) {
        const int r = i / A_W, c = i % A_W;
        const int y = reflect(ty0 - 2 + r, H), x = reflect(tx0 - 2 + c, W);
        float v = img[(size_t)y * W + x];
        if (clahe) v = clahe_map(v, y, x, TH, TW, L);
        if (gamma_on) v = fminf(fmaxf(powf(v, gamma), 0.f), 1.f);
        A[r * A_LD + c] = v;
    }
    __syncthreads();

    // 2. box blur + noise on the tile + halo 1 (values outside the image are never read by step 3)
    const unsigned seed_lo = (unsigned)P[XVR_SIM_AUG_SEED_LO], seed_hi = (unsigned)P[XVR_SIM_AUG_SEED_HI];
    for (int i = tid; i < B_H * B_W; i += TB) {
        const int r = i / B_W, c = i % B_W;
        const float* a = A + r * A_LD + c;   // the 3 x 3 window, top-left corner
        float v = a[A_LD + 1];
        if (blur) {
            const float w = 1.f / 9.f;
            v = a[0] * w + a[1] * w + a[2] * w + a[A_LD] * w + a[A_LD + 1] * w + a[A_LD + 2] * w + a[2 * A_LD] * w + a[2 * A_LD + 1] * w +
                a[2 * A_LD + 2] * w;
        }
        const int y = ty0 - 1 + r, x = tx0 - 1 + c;
        if (noise && y >= 0 && y < H && x >= 0 && x < W) v = v + aug_normal(seed_lo, seed_hi, (unsigned)b, (unsigned)y, (unsigned)x) * noise_std;
        Bv[r * B_LD + c] = v;
    }
    __syncthreads();

    // 3. sharpness, erasing, crop; one store per pixel
    const float f = P[XVR_SIM_AUG_SHARP];
    const bool erase = P[XVR_SIM_AUG_ERASE] != 0.f, crop_on = P[XVR_SIM_AUG_CROP_ON] != 0.f;
    const int ey = (int)P[XVR_SIM_AUG_ERASE_Y], ex = (int)P[XVR_SIM_AUG_ERASE_X], eh = (int)P[XVR_SIM_AUG_ERASE_H], ew = (int)P[XVR_SIM_AUG_ERASE_W];
    const int k = (int)P[XVR_SIM_AUG_CROP];
    for (int i = tid; i < OT_H * OT_W; i += TB) {
        const int r = i / OT_W, c = i % OT_W, y = ty0 + r, x = tx0 + c;
        if (y >= H || x >= W) continue;
        const float* q = Bv + r * B_LD + c;   // the 3 x 3 window, top-left corner
        float v = q[B_LD + 1];
        if (sharp) {
            float deg = v;   // border pixels keep their value
            if (y > 0 && y < H - 1 && x > 0 && x < W - 1) {
                const float w1 = 1.f / 13.f, w5 = 5.f / 13.f;
                deg = q[0] * w1 + q[1] * w1 + q[2] * w1 + q[B_LD] * w1 + q[B_LD + 1] * w5 + q[B_LD + 2] * w1 + q[2 * B_LD] * w1 +
                      q[2 * B_LD + 1] * w1 + q[2 * B_LD + 2] * w1;
                deg = fminf(fmaxf(deg, 0.f), 1.f);
            }
            if (f == 0.f) v = deg;
            else if (f != 1.f) {
                const float blend = deg + (v - deg) * f;
                v = (f > 0.f && f < 1.f) ? blend : fminf(fmaxf(blend, 0.f), 1.f);
            }
        }
        if (erase && y >= ey && y < ey + eh && x >= ex && x < ex + ew) v = erase_value;
        if (crop_on && (y < k || y >= H - k || x < k || x >= W - k)) v = 0.f;
        out[((size_t)b * H + y) * W + x] = v;
    }
}

int aug_check(const float* s, const float* params, int B, int H, int W) {
    if (!s || !params) return aug_fail(XVR_DRR_E_ARG, "null pointer argument");
    if (B <= 0 || B > 65535 || H < 2 || W < 2) return aug_fail(XVR_DRR_E_ARG, "bad size (B in [1, 65535], H, W >= 2)");
    if (GRID * clahe_tile(H) - H >= H || GRID * clahe_tile(W) - W >= W)
        return aug_fail(XVR_DRR_E_UNSUPPORTED, "image too small for the CLAHE tiles' reflect padding");
    if ((size_t)clahe_tile(H) * clahe_tile(W) >= (1u << 24)) return aug_fail(XVR_DRR_E_UNSUPPORTED, "CLAHE tile of 2^24 pixels or more");
    return XVR_DRR_OK;
}

}  // namespace

extern "C" {

int xvr_sim_augment_param_cols(void) { return XVR_SIM_AUG_COLS; }

size_t xvr_sim_augment_lut_bytes(int B) { return B > 0 ? (size_t)B * GRID * GRID * BINS : 0; }

int xvr_sim_augment_clahe_lut(const float* s, const float* params, int B, int H, int W, int clip_per_image, unsigned char* lut,
                              void* stream) {
    const int rc = aug_check(s, params, B, H, W);
    if (rc != XVR_DRR_OK) return rc;
    if (!lut) return aug_fail(XVR_DRR_E_ARG, "null pointer argument");
    if (reinterpret_cast<uintptr_t>(lut) & 3u) return aug_fail(XVR_DRR_E_ARG, "lut must be 4-byte aligned");
    hipLaunchKernelGGL(k_aug_clahe_lut, dim3(GRID * GRID, B), dim3(TB), 0, (hipStream_t)stream, s, params, B, H, W, clip_per_image, lut);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? XVR_DRR_OK : aug_fail(XVR_DRR_E_LAUNCH, hipGetErrorString(e));
}

int xvr_sim_augment_chain(const float* s, const float* params, const unsigned char* lut, int B, int H, int W, float noise_std,
                          float erase_value, float* out, void* stream) {
    const int rc = aug_check(s, params, B, H, W);
    if (rc != XVR_DRR_OK) return rc;
    if (!lut || !out) return aug_fail(XVR_DRR_E_ARG, "null pointer argument");
    const dim3 grid((W + OT_W - 1) / OT_W, (H + OT_H - 1) / OT_H, B);
    hipLaunchKernelGGL(k_aug_chain, grid, dim3(TB), 0, (hipStream_t)stream, s, params, lut, H, W, noise_std, erase_value, out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? XVR_DRR_OK : aug_fail(XVR_DRR_E_LAUNCH, hipGetErrorString(e));
}

}  // extern "C"
