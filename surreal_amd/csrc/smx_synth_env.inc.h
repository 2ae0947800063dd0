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

// ---- the `reach` task (SMX_TASK_REACH; surreal_amd/env/tasks.py holds the definition): A point masses, the state row
// [p (A) | v (A) | g (A)].  The same rule: fp32, no contraction, each product rounded before the sum.
constexpr int REACH_MAX_A = 21;                      // D = 3 A <= 63: a row's elements sit in one wavefront
constexpr int ARM_MAX_A = 30;                        // (SMX_TASK_ARM, below) D = 2 A + 2 <= 62: likewise

// what the task entry points take (smx_synth_task_supported)
inline bool synth_task_ok(int task, int D, int A) {
    if (task == SMX_TASK_DRIFT) return D > 0 && A > 0;
    if (task == SMX_TASK_ARM) return A > 0 && A <= ARM_MAX_A && D == 2 * A + 2;
    return task == SMX_TASK_REACH && A > 0 && A <= REACH_MAX_A && D == 3 * A;
}

// mass j's next velocity from its velocity v and its (clipped) action ac; disturbed (a stream with a scale s != 0;
// uniform over the launch): the step's draw sw = s * w[j] (disturbance_uniform of smx_philox.inc.h; the product rounded)
// joins the sum before the clamp -- and is NOT added otherwise: an undisturbed step keeps its bytes, a -0 included
__device__ __forceinline__ float reach_next_v(float v, float ac, bool disturbed = false, float sw = 0.f) {
    float vn = (0.9f * v) + (0.2f * ac);
    if (disturbed) vn = vn + sw;
    return fminf(fmaxf(vn, -1.0f), 1.0f);
}

// its next position from its position p and its NEXT velocity vn
__device__ __forceinline__ float reach_next_p(float p, float vn) {
    const float pn = p + (0.1f * vn);
    return fminf(fmaxf(pn, -10.0f), 10.0f);
}

// the step's reward from sd = sum_j d_j^2, d_j = p'_j - g_j in fp32, and sa = sum_j a_j^2 (both fp64, j ascending)
__device__ __forceinline__ float reach_reward(double sd, double sa) { return (float)(-(sd + 0.01 * sa)); }

// ---- the `arm` task (SMX_TASK_ARM; surreal_amd/env/tasks.py holds the definition): a planar arm of A links of length w =
// 2^-ceil(log2 A), the state row [theta (A) | omega (A) | g (2)] -- each link's absolute orientation, its angular velocity,
// the fingertip's goal.  The same rule: fp32, no contraction, each product rounded before the sum.
// link j's next angular velocity from its angular velocity om and its (clipped) action ac; disturbed, sw: as reach_next_v's
__device__ __forceinline__ float arm_next_omega(float om, float ac, bool disturbed = false, float sw = 0.f) {
    float on = (0.9f * om) + (0.4f * ac);
    if (disturbed) on = on + sw;
    return fminf(fmaxf(on, -1.0f), 1.0f);
}

// its next orientation from its orientation th and its NEXT angular velocity on: joint limits at +-(float)pi, no wrap
__device__ __forceinline__ float arm_next_theta(float th, float on) {
    const float tn = th + (0.2f * on);
    return fminf(fmaxf(tn, -3.1415927f), 3.1415927f);
}

// the task's sine and cosine of th in [-pi, pi]: the Taylor polynomials in th^2, c_k = (float)((-1)^k / (2k+1)!), k = 0..8,
// and (float)((-1)^k / (2k)!), k = 0..9, by Horner from the highest, acc = (acc * x2) + c_k with every operation rounded.
// The polynomials are the definition (within 1e-6 of the functions): no library call, the host's bits.
__device__ __forceinline__ void arm_sincos(float th, float& sn, float& cs) {
    constexpr float S[9] = {0x1p+0f, -0x1.555556p-3f, 0x1.111112p-7f, -0x1.a01a02p-13f, 0x1.71de3ap-19f, -0x1.ae6456p-26f,
                            0x1.612462p-33f, -0x1.ae7f3ep-41f, 0x1.952c78p-49f};
    constexpr float C[10] = {0x1p+0f, -0x1p-1f, 0x1.555556p-5f, -0x1.6c16c2p-10f, 0x1.a01a02p-16f, -0x1.27e4fcp-22f,
                             0x1.1eed8ep-29f, -0x1.93974ap-37f, 0x1.ae7f3ep-45f, -0x1.682786p-53f};
    const float x2 = th * th;
    float ps = S[8], pc = C[9];
#pragma unroll
    for (int k = 7; k >= 0; --k) ps = (ps * x2) + S[k];
#pragma unroll
    for (int k = 8; k >= 0; --k) pc = (pc * x2) + C[k];
    sn = th * ps;
    cs = pc;
}

// the length of each of the J links: 2^-ceil(log2 J), exact in every product
__device__ __forceinline__ double arm_link(int J) {
    double w = 1.0;
    for (int m = 1; m < J; m <<= 1) w *= 0.5;
    return w;
}

// the step's reward from sx = sum_j c_j, sy = sum_j s_j of the NEXT orientations and sa = sum_j a_j^2 (fp64, j ascending),
// the link length w and the goal (g0, g1)
__device__ __forceinline__ float arm_reward(double sx, double sy, double sa, double w, float g0, float g1) {
    const double dx = sx * w - (double)g0;
    const double dy = sy * w - (double)g1;
    return (float)(-((dx * dx + dy * dy) + 0.01 * sa));
}

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

// ---- the episode monitor (struct smx_episode_monitor, include/surreal_amd.h) ----------------------------------------
// The one rule every kernel that evaluates synth_reward applies when a monitor is attached (M.ep_reward != null), by
// the ONE lane that formed actor a's reward: the step's fp32 reward joins the open episode's fp64 sum in step order;
// on done the pair goes to slot (finished episodes) % capacity of the actor's ring and the open pair clears.  open_reward /
// open_steps: the open pair wherever the caller holds it between steps (LDS in the persistent kernels, else HBM through
// episode_account).  Plain stores by the owning lane only: no atomics, so a sum depends on the order of its steps alone.
__device__ __forceinline__ void episode_step(const smx_episode_monitor& M, long a, double& open_reward, int& open_steps,
                                             float reward, bool done) {
    const double sum = open_reward + (double)reward;
    const int steps = open_steps + 1;
    if (done) {
        const long long e = M.ep_count[a];
        const size_t slot = (size_t)a * M.capacity + (size_t)(e % M.capacity);
        M.done_reward[slot] = sum;
        M.done_steps[slot] = steps;
        M.ep_count[a] = e + 1;
    }
    open_reward = done ? 0.0 : sum;
    open_steps = done ? 0 : steps;
}

// one step of an actor whose open pair lives in HBM between launches (the per-step kernels)
__device__ __forceinline__ void episode_account(const smx_episode_monitor& M, long a, float reward, bool done) {
    double open_reward = M.ep_reward[a];
    int open_steps = M.ep_steps[a];
    episode_step(M, a, open_reward, open_steps, reward, done);
    M.ep_reward[a] = open_reward;
    M.ep_steps[a] = open_steps;
}

// what the entry points ask of a monitor: none, or all five pointers (SMX_E_NULL) and a ring of at least one slot
inline bool episode_pointers_ok(const smx_episode_monitor& M) {
    return !M.ep_reward || (M.ep_steps && M.ep_count && M.done_reward && M.done_steps);
}
inline bool episode_shape_ok(const smx_episode_monitor& M) { return !M.ep_reward || M.capacity > 0; }
