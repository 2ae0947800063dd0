// LayerNorm over the F features of a workgroup's RB rows of a hidden LDS tile, behind the barrier that ends the layer
// (the caller barriers after it) -- shared by the one-launch DDPG rollout (smx_rollout.hip) and the DDPG row schedule
// (smx_ddpg_rows.hip).  Included inside the including file's anonymous namespace, after smx_common.h.
//
// One wavefront owns a row, the rows dealt over the NWV waves; lane j takes the columns j + 64 c, c ascending, and the
// expressions are layernorm_fwd_kernel's (smx_ddpg.hip), its zero terms for the columns past F left out: given the same
// row the result, the mean and the reciprocal standard deviation have the bits smx_layernorm_forward_f32 produces,
// whatever RB and whichever wave.  Only columns < F are written: the padding of `out` stays what it was.  A lane's columns
// are consecutive words across the wave: no bank is hit twice.  `out` may be `pre` (in place).  MAXC columns per lane:
// F <= 64 MAXC.
//
// emit.value(r, j, y) sees every element written, emit.stats(r, mean, rstd) the row's statistics (every lane holds them).
struct LnNoEmit {
    __device__ __forceinline__ void value(int, int, float) const {}
    __device__ __forceinline__ void stats(int, float, float) const {}
};

template <int RB, int NWV, int MAXC, class Emit>
__device__ __forceinline__ void ln_rows(const float* pre, int ldp, float* out, int ldo, int F, const float* gamma,
                                        const float* beta, float eps, int wv, int lane, const Emit& emit) {
#pragma unroll 1
    for (int r = wv; r < RB; r += NWV) {
        const float* xr = pre + r * ldp;
        float* yr = out + r * ldo;
        float v[MAXC];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (64 * c >= F) break;                  // (wave-uniform)
            const int j = lane + 64 * c;
            v[c] = (j < F) ? xr[j] : 0.f;
            s += v[c];
        }
        const float m = smx_wave_sum(s) / (float)F;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (64 * c >= F) break;
            const int j = lane + 64 * c;
            const float d = (j < F) ? v[c] - m : 0.f;
            q += d * d;
        }
        const float rs = 1.0f / sqrtf(smx_wave_sum(q) / (float)F + eps);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (64 * c >= F) break;
            const int j = lane + 64 * c;
            if (j < F) {
                const float y = ((v[c] - m) * rs) * gamma[j] + beta[j];
                yr[j] = y;
                emit.value(r, j, y);
            }
        }
        emit.stats(r, m, rs);
    }
}
