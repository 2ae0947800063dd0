// The synthetic environment's dynamics and the z-filter's apply: the one definition every kernel that steps the
// environment or filters its observations uses (smx_replay.hip's per-step kernels, smx_rollout.hip's persistent
// rollouts and DDPG step).  Included inside an anonymous namespace.  The expressions keep their evaluation order: the
// build does not contract, and the goldens pin these roundings.

// element k's constant drift
__device__ __forceinline__ float synth_drift(int k) { return 0.01f * (float)(((37 * k) % 17) - 8); }

// element k's next state from its state s, its action column's (clipped) action ac and its drift
__device__ __forceinline__ float synth_next(float s, float ac, float drift) {
    const float sn = (0.9f * s + 0.5f * ac) + drift;
    return fminf(fmaxf(sn, -10.0f), 10.0f);
}

// the step's reward from q = sum_j a_j^2 (fp64, j ascending) and element 0 of the next state
__device__ __forceinline__ float synth_reward(double q, float sn0) { return (float)(-0.1 * q + 0.05 * (double)sn0); }

// the synthetic camera (SyntheticEnv._frame): a frame's shift from its step count t and the first state component s0
// (in double, as the host's 100 * abs(float(s0))), and byte (c, y, x) of that frame.  Every kernel that renders a frame
// (smx_replay.hip's synth_frame_kernel, smx_rollout.hip's DDPG pixel step) evaluates these two.
__device__ __forceinline__ int synth_frame_shift(int t, float s0) { return 3 * t + (int)(100.0 * (double)fabsf(s0)); }
__device__ __forceinline__ unsigned char synth_frame_px(int c, int y, int x, int shift) {
    return (unsigned char)((37 * c + 5 * y + 11 * x + shift) % 256);
}

// the z-filter's mean m and std sd of element k from the running sums (z_filter.py:74-76)
__device__ __forceinline__ void zfilter_stats(const float* zsum, const float* zsumsq, const float* zcount, float zeps,
                                              int k, float& m, float& sd) {
    const float c = zcount[0];
    m = zsum[k] / c;
    const float var = zsumsq[k] / c - m * m;
    sd = sqrtf(var);
    if (sd == sd) sd = fmaxf(sd, zeps);
}

// the filtered value, clamped to +-5 (z_filter.py:77)
__device__ __forceinline__ float zclamp(float x, float m, float sd) {
    float v = (x - m) / sd;
    if (v == v) v = fminf(fmaxf(v, -5.0f), 5.0f);
    return v;
}
