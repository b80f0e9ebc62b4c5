// Volume reconstruction on the device for MI355X (gfx950): what consumes dL/dvoxel.  C ABI: include/xvr_drr.h
// (xvr_drr_tv_smooth, xvr_drr_volume_adam_step); formulas, the two-launch argument and the NaN contract: DESIGN.md section 4.7; the
// torch restatements the kernels are checked against: tests/recon_restated.py.
//
//   k_tv_smooth     smoothed isotropic total variation (forward differences, Neumann faces), value AND gradient in one pass: a
//                   workgroup stages a 4 x 8 x 64 tile of V with a one-voxel halo in LDS, computes n for the tile and its back
//                   halo, then GATHERS each voxel's gradient (no atomics) and adds lambda x it into the caller's buffer.
//   k_tv_sum        the value: one fixed-order sum of the workgroups' double partials (same bits on every run).
//   k_volume_adam   projected Adam over the voxels, in place: reads p, g, m, v and writes p, m, v once; a non-finite g leaves
//                   its voxel untouched and is counted (the brick-local splats poison a voxel with NaN on overflow).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "xvr_drr.h"

extern "C" void xvr_drr_set_last_error(const char* msg);  // drr_api.hip

namespace {

constexpr int TB = 256;
constexpr int TX = 4, TY = 8, TZ = 64;                 // output tile (z is contiguous: the long side)
constexpr int VX = TX + 2, VY = TY + 2, VZ = TZ + 2;   // V with a one-voxel halo on every side
constexpr int NX = TX + 1, NY = TY + 1, NZ = TZ + 1;   // n on the tile and its back halo
constexpr int V_LD = VZ + 1, N_LD = NZ;                // (odd row strides: a row step is not a bank multiple)
static_assert(V_LD % 2 == 1 && N_LD % 2 == 1, "odd LDS row strides");
static_assert(TZ % 4 == 0, "16-byte accesses along z");

int rfail(int code, const char* msg) {
    xvr_drr_set_last_error(msg);
    return code;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct TvDoubles {   // the factors as the caller gave them: the value's terms are evaluated in doubles
    double w0, w1, w2, eps;
};

// Coordinates outside the volume are CLAMPED when the tile is staged, which is the whole boundary rule: a forward difference across
// the far face reads the voxel itself and is 0 (Neumann), and a back-halo cell outside the volume has a zero difference along the
// axis it is a halo of, so the term "i - e_a outside" drops out of the gather by itself.
// VEC: D2 % 4 == 0 and 16-byte aligned buffers -- the tile's rows are loaded, and the gradient is updated, 16 bytes at a time.
template <bool VEC>
__global__ __launch_bounds__(TB) void k_tv_smooth(const float* __restrict__ V, int D0, int D1, int D2, float w0, float w1, float w2, float eps,
                                                  float lambda, TvDoubles dd, float* __restrict__ G, double* __restrict__ partial, int nby, int nbz) {
    __shared__ float Vs[VX * VY * V_LD];
    __shared__ float Ns[NX * NY * N_LD];
    __shared__ double wpart[TB / 64];
    const int tid = threadIdx.x;
    const int bz = (int)(blockIdx.x % (unsigned)nbz), by = (int)((blockIdx.x / (unsigned)nbz) % (unsigned)nby);
    const int bx = (int)(blockIdx.x / ((unsigned)nbz * (unsigned)nby));
    const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZ;

    // 1. the tile and its halo, clamped: local (lx, ly, lz) in [0, VX) x [0, VY) x [0, VZ) holds V at (x0 - 1 + lx, ...)
    auto row_of = [&](int r) {   // -> element offset of the (clamped) row r = lx * VY + ly
        const int x = min(max(x0 - 1 + r / VY, 0), D0 - 1), y = min(max(y0 - 1 + r % VY, 0), D1 - 1);
        return ((long long)x * D1 + y) * D2;
    };
    if (VEC) {
        for (int i = tid; i < VX * VY * (TZ / 4); i += TB) {   // the rows' interiors: z0 is a multiple of 4, and so is D2
            const int r = i / (TZ / 4), z = z0 + 4 * (i % (TZ / 4));
            const float* row = V + row_of(r);
            float4 v;
            if (z < D2) v = *reinterpret_cast<const float4*>(row + z);
            else { const float e = row[D2 - 1]; v = make_float4(e, e, e, e); }
            float* dst = Vs + r * V_LD + 1 + (z - z0);
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        for (int i = tid; i < VX * VY * 2; i += TB) {          // the two z-halo voxels of every row
            const int r = i >> 1, lz = (i & 1) ? VZ - 1 : 0;
            Vs[r * V_LD + lz] = V[row_of(r) + min(max(z0 - 1 + lz, 0), D2 - 1)];
        }
    } else {
        for (int i = tid; i < VX * VY * VZ; i += TB) {
            const int r = i / VZ, lz = i % VZ;
            Vs[r * V_LD + lz] = V[row_of(r) + min(max(z0 - 1 + lz, 0), D2 - 1)];
        }
    }
    __syncthreads();

    // 2. n on the tile and its back halo: cell (cx, cy, cz) in [0, NX) x [0, NY) x [0, NZ) is the voxel (x0 - 1 + cx, ...), i.e.
    //    Vs (cx, cy, cz); the value sums the cells of the tile proper that lie inside the volume
    const float eps2 = eps * eps;
    double acc = 0.0;
    for (int i = tid; i < NX * NY * NZ; i += TB) {
        const int cz = i % NZ, cy = (i / NZ) % NY, cx = i / (NZ * NY);
        const float* q = Vs + (cx * VY + cy) * V_LD + cz;
        const float c = q[0];
        const float d0 = w0 * (q[VY * V_LD] - c), d1 = w1 * (q[V_LD] - c), d2 = w2 * (q[1] - c);
        const float n = sqrtf(d0 * d0 + d1 * d1 + d2 * d2 + eps2);
        Ns[(cx * NY + cy) * N_LD + cz] = n;
        if (partial && cx >= 1 && cy >= 1 && cz >= 1 && x0 - 1 + cx < D0 && y0 - 1 + cy < D1 && z0 - 1 + cz < D2) {
            // the value's terms in doubles from the float voxels (the sum is then right to the rounding of its one float result;
            // n - eps from a float n would carry 1e-7 n / (n - eps) per term).  A constant volume: sqrt(eps^2) - eps == 0 exactly.
            const double e0 = dd.w0 * ((double)q[VY * V_LD] - (double)c), e1 = dd.w1 * ((double)q[V_LD] - (double)c);
            const double e2 = dd.w2 * ((double)q[1] - (double)c);
            acc += sqrt(e0 * e0 + e1 * e1 + e2 * e2 + dd.eps * dd.eps) - dd.eps;
        }
    }
    if (partial) {   // fixed order: lanes -> wave (butterfly), waves -> workgroup, workgroups -> k_tv_sum
        const double t = wave_sum_d(acc);
        if ((tid & 63) == 0) wpart[tid >> 6] = t;
    }
    __syncthreads();
    if (partial && tid == 0) partial[blockIdx.x] = (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);
    if (!G) return;

    // 3. the gather: voxel (lx, ly, lz) of the tile is Vs (lx + 1, ly + 1, lz + 1) and cell (lx + 1, ly + 1, lz + 1)
    auto grad_at = [&](int lx, int ly, int lz) {
        const float* q = Vs + ((lx + 1) * VY + ly + 1) * V_LD + lz + 1;
        const float* n = Ns + ((lx + 1) * NY + ly + 1) * N_LD + lz + 1;
        const float c = q[0];
        const float d0 = w0 * (q[VY * V_LD] - c), d1 = w1 * (q[V_LD] - c), d2 = w2 * (q[1] - c);
        const float own = (w0 * d0 + w1 * d1 + w2 * d2) / n[0];
        const float b0 = w0 * (w0 * (c - q[-VY * V_LD])) / n[-NY * N_LD];
        const float b1 = w1 * (w1 * (c - q[-V_LD])) / n[-N_LD];
        const float b2 = w2 * (w2 * (c - q[-1])) / n[-1];
        return ((b0 + b1) + b2) - own;
    };
    if (VEC) {
        for (int i = tid; i < TX * TY * (TZ / 4); i += TB) {
            const int lz = 4 * (i % (TZ / 4)), ly = (i / (TZ / 4)) % TY, lx = i / ((TZ / 4) * TY);
            const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= D0 || y >= D1 || z >= D2) continue;
            float4* g = reinterpret_cast<float4*>(G + ((long long)x * D1 + y) * D2 + z);
            float4 o = *g;
            o.x += lambda * grad_at(lx, ly, lz);
            o.y += lambda * grad_at(lx, ly, lz + 1);
            o.z += lambda * grad_at(lx, ly, lz + 2);
            o.w += lambda * grad_at(lx, ly, lz + 3);
            *g = o;
        }
    } else {
        for (int i = tid; i < TX * TY * TZ; i += TB) {
            const int lz = i % TZ, ly = (i / TZ) % TY, lx = i / (TZ * TY);
            const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= D0 || y >= D1 || z >= D2) continue;
            G[((long long)x * D1 + y) * D2 + z] += lambda * grad_at(lx, ly, lz);
        }
    }
}

// value[0] = lambda x the sum of the workgroups' partials: thread t adds partials t, t + TB, ... in order, then one fixed tree
__global__ __launch_bounds__(TB) void k_tv_sum(const double* __restrict__ partial, long long nblk, double lambda, float* __restrict__ value) {
    __shared__ double wpart[TB / 64];
    double t = 0.0;
    for (long long k = threadIdx.x; k < nblk; k += TB) t += partial[k];
    t = wave_sum_d(t);
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) value[0] = (float)(lambda * ((wpart[0] + wpart[1]) + (wpart[2] + wpart[3])));
}

struct AdamArgs {
    float one_minus_b1, b1, one_minus_b2, b2;
    float step;        // lr / bc1
    float bc2_sqrt;    // sqrt(bc2)
    float eps, lo, hi;
    float sign;        // -1 with maximize
};

// -> true if the voxel was skipped (non-finite gradient: p, m, v stay as they are)
__device__ __forceinline__ bool adam_one(float& p, float g, float& m, float& v, const AdamArgs& a) {
    g *= a.sign;
    if (!isfinite(g)) return true;
    m = a.b1 * m + a.one_minus_b1 * g;
    v = a.b2 * v + a.one_minus_b2 * (g * g);
    const float q = p - a.step * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
    p = q < a.lo ? a.lo : (q > a.hi ? a.hi : q);   // (a NaN p stays NaN)
    return false;
}

// VEC: the four buffers are 16-byte aligned -- float4 accesses over n / 4, the n % 4 tail by scalars
template <bool VEC>
__global__ __launch_bounds__(TB) void k_volume_adam(float* __restrict__ P, const float* __restrict__ Gr, float* __restrict__ M,
                                                    float* __restrict__ Vv, long long n, AdamArgs a, unsigned* __restrict__ skipped) {
    unsigned skip = 0;
    const long long first = (long long)blockIdx.x * TB + threadIdx.x, stride = (long long)gridDim.x * TB;
    const long long n4 = VEC ? n >> 2 : 0;
    for (long long i = first; i < n4; i += stride) {
        float4 p = reinterpret_cast<float4*>(P)[i], m = reinterpret_cast<float4*>(M)[i], v = reinterpret_cast<float4*>(Vv)[i];
        const float4 g = reinterpret_cast<const float4*>(Gr)[i];
        const bool s0 = adam_one(p.x, g.x, m.x, v.x, a), s1 = adam_one(p.y, g.y, m.y, v.y, a);
        const bool s2 = adam_one(p.z, g.z, m.z, v.z, a), s3 = adam_one(p.w, g.w, m.w, v.w, a);
        skip += (unsigned)s0 + (unsigned)s1 + (unsigned)s2 + (unsigned)s3;
        reinterpret_cast<float4*>(P)[i] = p;
        reinterpret_cast<float4*>(M)[i] = m;
        reinterpret_cast<float4*>(Vv)[i] = v;
    }
    for (long long i = (n4 << 2) + first; i < n; i += stride) {   // (VEC: at most three voxels, in the first workgroup)
        float p = P[i], m = M[i], v = Vv[i];
        skip += (unsigned)adam_one(p, Gr[i], m, v, a);
        P[i] = p;
        M[i] = m;
        Vv[i] = v;
    }
    if (skipped) {   // integer adds, one per wavefront at most: exact in any order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) skip += __shfl_xor(skip, o);
        if ((threadIdx.x & 63) == 0 && skip) atomicAdd(skipped, skip);
    }
}

long long tv_blocks(int D0, int D1, int D2) {
    return (long long)((D0 + TX - 1) / TX) * ((D1 + TY - 1) / TY) * ((D2 + TZ - 1) / TZ);
}

}  // namespace

extern "C" {

size_t xvr_drr_tv_smooth_workspace_bytes(int D0, int D1, int D2) {
    if (D0 <= 0 || D1 <= 0 || D2 <= 0) return 0;
    return (size_t)tv_blocks(D0, D1, D2) * sizeof(double);
}

int xvr_drr_tv_smooth(const float* volume, int D0, int D1, int D2, double w0, double w1, double w2, double eps, double lambda, float* grad_accum,
                      float* value, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!volume) return rfail(XVR_DRR_E_ARG, "null pointer argument: volume");
    if (!grad_accum && !value) return rfail(XVR_DRR_E_ARG, "null pointer argument: neither grad_accum nor value is given");
    if (D0 < 2 || D1 < 2 || D2 < 2) return rfail(XVR_DRR_E_ARG, "bad size: every axis of the volume must be at least 2");
    if (!(eps > 0.0) || !((float)eps > 0.f)) return rfail(XVR_DRR_E_ARG, "eps must be positive (as a float too)");
    const long long nblk = tv_blocks(D0, D1, D2);
    if (nblk >= (1LL << 31)) return rfail(XVR_DRR_E_UNSUPPORTED, "total variation: 2^31 tiles or more");
    if (value && (!workspace || workspace_bytes < (size_t)nblk * sizeof(double)))
        return rfail(XVR_DRR_E_ARG, "workspace missing or smaller than xvr_drr_tv_smooth_workspace_bytes()");
    if (value && (reinterpret_cast<uintptr_t>(workspace) & 7u)) return rfail(XVR_DRR_E_ARG, "workspace must be 8-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    double* partial = value ? static_cast<double*>(workspace) : nullptr;
    const int nby = (D1 + TY - 1) / TY, nbz = (D2 + TZ - 1) / TZ;
    const TvDoubles dd = {w0, w1, w2, eps};
    const bool vec = D2 % 4 == 0 && ((reinterpret_cast<uintptr_t>(volume) | reinterpret_cast<uintptr_t>(grad_accum)) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(k_tv_smooth<true>, dim3((unsigned)nblk), dim3(TB), 0, stream, volume, D0, D1, D2, (float)w0, (float)w1, (float)w2,
                                (float)eps, (float)lambda, dd, grad_accum, partial, nby, nbz);
    else hipLaunchKernelGGL(k_tv_smooth<false>, dim3((unsigned)nblk), dim3(TB), 0, stream, volume, D0, D1, D2, (float)w0, (float)w1, (float)w2,
                            (float)eps, (float)lambda, dd, grad_accum, partial, nby, nbz);
    if (value) hipLaunchKernelGGL(k_tv_sum, dim3(1), dim3(TB), 0, stream, partial, nblk, lambda, value);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? XVR_DRR_OK : rfail(XVR_DRR_E_LAUNCH, hipGetErrorString(e));
}

int xvr_drr_volume_adam_step(float* volume, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1,
                             double beta2, double eps, double bc1, double bc2, float lo, float hi, int maximize, unsigned* skipped,
                             void* stream_) {
    if (!volume || !grad || !exp_avg || !exp_avg_sq) return rfail(XVR_DRR_E_ARG, "null pointer argument");
    if (n <= 0) return rfail(XVR_DRR_E_ARG, "bad size: n must be positive");
    if (!(eps > 0.0)) return rfail(XVR_DRR_E_ARG, "eps must be positive");
    if (!(lo <= hi)) return rfail(XVR_DRR_E_ARG, "lo > hi (or a NaN bound)");
    if (!(bc1 > 0.0) || !(bc2 > 0.0)) return rfail(XVR_DRR_E_ARG, "bias corrections bc1, bc2 must be positive (1 - beta^t, t >= 1)");
    if (reinterpret_cast<uintptr_t>(skipped) & 3u) return rfail(XVR_DRR_E_ARG, "skipped must be 4-byte aligned");
    AdamArgs a;
    a.b1 = (float)beta1;   // (hyper-parameters arrive as doubles: 1 - beta2 taken from a float beta2 is off by 1e-5 of itself)
    a.one_minus_b1 = (float)(1.0 - beta1);
    a.b2 = (float)beta2;
    a.one_minus_b2 = (float)(1.0 - beta2);
    a.step = (float)(lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.eps = (float)eps;
    a.lo = lo;
    a.hi = hi;
    a.sign = maximize ? -1.f : 1.f;
    const bool vec = ((reinterpret_cast<uintptr_t>(volume) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
                       reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15u) == 0;
    // grid-stride over what is resident at once (CUs x occupancy)
    static const long long resident = [] {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_volume_adam<true>), TB, 0) != hipSuccess || per_cu < 1) per_cu = 8;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        return (long long)per_cu * cus;
    }();
    const long long items = vec ? (n >> 2) + 3 : n;
    long long blocks = (items + TB - 1) / TB;
    if (blocks > resident) blocks = resident;
    if (vec) hipLaunchKernelGGL(k_volume_adam<true>, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream_, volume, grad, exp_avg, exp_avg_sq, n, a, skipped);
    else hipLaunchKernelGGL(k_volume_adam<false>, dim3((unsigned)blocks), dim3(TB), 0, (hipStream_t)stream_, volume, grad, exp_avg, exp_avg_sq, n, a, skipped);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? XVR_DRR_OK : rfail(XVR_DRR_E_LAUNCH, hipGetErrorString(e));
}

}  // extern "C"
