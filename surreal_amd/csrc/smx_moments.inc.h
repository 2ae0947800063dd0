// Statistics reductions shared by smx_ppo.hip (their own launches), smx_scan.hip (GAE + normalisation) and the
// end-of-learn roles (smx_learn_epilogue.inc.h).  Included at file scope.
#pragma once

// mergeable moments (count, mean, M2) of two disjoint sets (Chan et al.)
struct Mom { double n, mean, m2; };
static __device__ __forceinline__ Mom mom_merge(const Mom& a, const Mom& b) {
    if (b.n <= 0.0) return a;
    if (a.n <= 0.0) return b;
    Mom r;
    r.n = a.n + b.n;
    const double d = b.mean - a.mean;
    r.m2 = a.m2 + b.m2 + d * d * a.n * b.n / r.n;
    r.mean = a.mean + d * b.n / r.n;
    return r;
}
static __device__ __forceinline__ double shfl_d(double v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src, 64); hi = __shfl(hi, src, 64);
    return __hiloint2double(hi, lo);
}

// one wave: lane l folds the partial rows l, l + 64, ... of ONE epoch in order, then the 64 lanes are
// merged pairwise in a fixed tree (lane l with l + 32, 16, ...: the same order on every run)
static __device__ __forceinline__ void value_finalize_wave(const float* __restrict__ P, int nblk,
                                                           float* __restrict__ stats_e, int lane) {
    Mom d = {0.0, 0.0, 0.0}, g = {0.0, 0.0, 0.0};
    double sq = 0.0;
    for (int b = lane; b < nblk; b += 64) {
        const float4 lo = *(const float4*)(P + 8 * b);
        const float4 hi = *(const float4*)(P + 8 * b + 4);
        const Mom db = {(double)lo.x, (double)lo.y, (double)lo.z}, gb = {(double)lo.x, (double)lo.w, (double)hi.x};
        d = mom_merge(d, db);
        g = mom_merge(g, gb);
        if (lo.x > 0.f) sq += (double)hi.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Mom od, og;
        od.n = shfl_d(d.n, lane + off); od.mean = shfl_d(d.mean, lane + off); od.m2 = shfl_d(d.m2, lane + off);
        og.n = od.n; og.mean = shfl_d(g.mean, lane + off); og.m2 = shfl_d(g.m2, lane + off);
        const double osq = shfl_d(sq, lane + off);
        if (lane < off) {
            d = mom_merge(d, od);
            g = mom_merge(g, og);
            sq += osq;
        }
    }
    if (lane == 0) {
        const double n = d.n;
        stats_e[SMX_VS_LOSS] = (float)(sq / n);          // ppo.py:326
        // 1 - var(returns - values) / var(returns), unbiased variances (ppo.py:325)
        stats_e[SMX_VS_EXPVAR] = 1.0f - (float)(d.m2 / (n - 1.0)) / (float)(g.m2 / (n - 1.0));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// One workgroup's reductions, written for VT "virtual" threads and run by NTH real ones (VT a multiple of NTH, both of
// 64): real thread t plays the virtual threads t, t + NTH, ... one after the other, so virtual wave w + NTH / 64 is real
// wave w with the same lanes.  Every per-thread chain (stride VT), every wave butterfly and every fixed-order sum over
// the VT / 64 waves has the operands and the order it has on VT real threads: the result's bits depend on VT alone.
// With NTH == VT the pass loops have one trip.
// ---------------------------------------------------------------------------------------------------------------

// a running statistic that another workgroup of the SAME launch writes or reads travels as device-scope relaxed stores
// and loads (COH; see partial_store, smx_ppo_loss.inc.h); across a launch boundary plain accesses do
template <bool COH>
static __device__ __forceinline__ float stat_load(const float* p) {
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return __builtin_nontemporal_load(p);
}
template <bool COH>
static __device__ __forceinline__ void stat_store(float* p, float v) {
    if constexpr (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// batch moments {n, mean, M2} of x[0, n) in fp64 (two passes); red: VT / 64 doubles of LDS, bc: one more.  On return
// out[] is there for every thread of the workgroup.
template <int VT, int NTH>
static __device__ __forceinline__ void block_moments(const float* __restrict__ x, long n, float* __restrict__ out,
                                                     double* red, double* bc) {
    constexpr int PS = VT / NTH;
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const int vt = tid + NTH * ps;
        double s = 0.0;
        for (long i = vt; i < n; i += VT) s += (double)__builtin_nontemporal_load(x + i);
        s = smx_wave_sum_d(s);
        if (lane == 0) red[vt >> 6] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < VT / 64; ++i) t += red[i];
        *bc = t / (double)n;
    }
    __syncthreads();
    const double mean = *bc;
    double q2[PS];
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        double q = 0.0;
        for (long i = tid + NTH * ps; i < n; i += VT) {
            const double d = (double)__builtin_nontemporal_load(x + i) - mean;
            q += d * d;
        }
        q2[ps] = smx_wave_sum_d(q);
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < PS; ++ps)
        if (lane == 0) red[(tid + NTH * ps) >> 6] = q2[ps];
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < VT / 64; ++i) t += red[i];
        out[0] = (float)n;
        out[1] = (float)mean;
        out[2] = (float)t;
    }
    __syncthreads();
}

// out[0] = mean(log_var); out[1..3] = mean over the D features of running_sum/count,
// running_sumsq/count and sqrt(running_sumsq/count - (running_sum/count)^2)  (no clamp: z_filter.py:90-98);
// red: VT / 64 x 4 doubles of LDS
template <int VT, int NTH, bool COH>
static __device__ __forceinline__ void final_stats_block(const float* __restrict__ log_var, int A,
                                                         const float* __restrict__ rsum,
                                                         const float* __restrict__ rsumsq,
                                                         const float* __restrict__ count, int D,
                                                         float* __restrict__ out, double (*red)[4]) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();  // protect `red` from a previous use
#pragma unroll
    for (int ps = 0; ps < VT / NTH; ++ps) {
        const int vt = tid + NTH * ps;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int a = vt; a < A; a += VT) s0 += (double)log_var[a];
        if (rsum) {
            const float cnt = stat_load<COH>(count);
            for (int d = vt; d < D; d += VT) {
                const float m = stat_load<COH>(rsum + d) / cnt, q = stat_load<COH>(rsumsq + d) / cnt;
                s1 += (double)m;
                s2 += (double)q;
                s3 += (double)sqrtf(q - m * m);
            }
        }
        s0 = smx_wave_sum_d(s0); s1 = smx_wave_sum_d(s1); s2 = smx_wave_sum_d(s2); s3 = smx_wave_sum_d(s3);
        if (lane == 0) { const int w = vt >> 6; red[w][0] = s0; red[w][1] = s1; red[w][2] = s2; red[w][3] = s3; }
    }
    __syncthreads();
    if (tid < 4) {
        double t = 0.0;
        for (int i = 0; i < VT / 64; ++i) t += red[i][tid];
        out[tid] = (float)(t / (double)(tid == 0 ? A : (D > 0 ? D : 1)));
    }
}
