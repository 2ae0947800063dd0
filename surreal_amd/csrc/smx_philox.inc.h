// Philox4x32-10 (Salmon et al. 2011) and the rollouts' exploration-noise stream built on it: the one definition the
// replay sampler (smx_replay.hip) and every launch that samples an action (smx_replay.hip's per-step kernels,
// smx_rollout.hip's persistent rollouts and step kernels, the fill kernel) evaluate.  Included inside an anonymous
// namespace, after include/surreal_amd.h (struct smx_noise_stream).

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// the ten rounds on counter c with key (k0, k1), in place
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// ---- the noise stream (struct smx_noise_stream, include/surreal_amd.h) ----------------------------------------------
// The standard normal of (seed, global actor id g < 2^32, draw step s, action component j): a pure function of the four.
//   x[0..3] = philox4x32_10(counter = (g, low32(s), high32(s), j >> 2), key = (low32(seed), high32(seed)))
//   pair p = (j & 3) >> 1 takes the words x[2p], x[2p + 1]:
//   u0 = ((float)(x[2p] >> 8) + 0.5f) * 0x1p-24f          (24 bits, exact in fp32; in (0, 1), never 0 or 1)
//   u1 = ((float)(x[2p + 1] >> 8) + 0.5f) * 0x1p-24f
//   r  = sqrtf(-2.0f * logf(u0));   (sn, cs) = sincospif(2.0f * u1)          (angle 2 pi u1; 2 u1 is exact)
//   normal = (j & 1) ? r * sn : r * cs
// so the four words of one block give components 4q .. 4q + 3 by two Box-Muller pairs, and |normal| <=
// sqrt(-2 ln 2^-25) ~ 5.887.  The accurate library functions, no fast intrinsics; the build does not contract: every
// caller gets the same bits.  Each (actor, component) lane runs its own ten rounds (a step's ~200 VALU instructions
// against the 32 k cycles of its layers).
// the word -> normal conversion above on a finished Philox block x: component j & 3 of its four normals
__device__ __forceinline__ float philox_normal(const uint32_t (&x)[4], int j) {
    const bool hi = (j & 2) != 0;
    const uint32_t x0 = hi ? x[2] : x[0], x1 = hi ? x[3] : x[1];
    const float u0 = ((float)(x0 >> 8) + 0.5f) * 0x1p-24f;
    const float u1 = ((float)(x1 >> 8) + 0.5f) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u0));
    float sn, cs;
    sincospif(2.0f * u1, &sn, &cs);
    return (j & 1) ? r * sn : r * cs;
}

__device__ __forceinline__ float noise_normal(uint64_t seed, uint32_t g, uint64_t s, int j) {
    uint32_t c[4] = {g, (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)j >> 2};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return philox_normal(c, j);
}

// the draw of local actor a at the call's k-th step, component j
__device__ __forceinline__ float noise_draw(const smx_noise_stream& N, long a, int k, int j) {
    return noise_normal(N.seed, (uint32_t)(N.actor_base + a), (uint64_t)(N.step + k), j);
}

// THE RULE of a sampling launch (include/surreal_amd.h): eps wins; else the stream when enabled; else no noise
__host__ __device__ inline bool noise_on(const float* eps, const smx_noise_stream& N) {
    return eps != nullptr || N.enabled != 0;
}
// a noisy launch's draw for (local actor a, the call's k-th step, component j): element i of eps, else the stream's
__device__ __forceinline__ float noise_pick(const float* eps, size_t i, const smx_noise_stream& N, long a, int k, int j) {
    return eps ? eps[i] : noise_draw(N, a, k, j);
}
// what the entry points ask of a stream over n actors: every global actor id in [0, 2^32) (SMX_E_SHAPE)
inline bool noise_shape_ok(const smx_noise_stream& N, long long n) {
    return !N.enabled || (N.actor_base >= 0 && N.actor_base + n <= (1LL << 32));
}

// ---- parameter-space noise (struct smx_param_noise, include/surreal_amd.h) -------------------------------------------
// The standard normal of (seed, global agent id g < 2^32, generation q < 2^32, element i of the actor's flat parameters
// W1 | b1 | W2 | b2 | W3 | b3, each row-major: the order DDPGModel keeps them in): component i & 3 of the block at counter
// (g, q, i >> 2, PARAM_NOISE_TAG) under the same key, through philox_normal.  The exploration stream's fourth counter
// word is j >> 2 < 16 (at most 64 action components), so the two never share a block, whatever the seed.
constexpr uint32_t PARAM_NOISE_TAG = 0x504E0001u;
__device__ __forceinline__ float param_noise_normal(uint64_t seed, uint32_t g, uint32_t q, uint32_t i) {
    uint32_t c[4] = {g, q, i >> 2, PARAM_NOISE_TAG};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return philox_normal(c, (int)(i & 3u));
}

// ---- the reset stream (struct smx_reset_stream, include/surreal_amd.h; surreal_amd/env/tasks.py holds the definition) --
// Element k < 3 J of the `reach` row [p | v | g] that (seed, global actor id g < 2^32, episode e) begins with: a pure
// function of the four.
//   x[0..3] = philox4x32_10(counter = (g, low32(e), high32(e), RESET_TAG | (k >> 2)), key = (low32(seed), high32(seed)))
//   u = (float)(x[k & 3] >> 8) * 0x1p-23f - 1.0f        (24 bits, scaled, minus one: every step exact in fp32; [-1, 1))
//   a position (k < J) or a goal (k >= 2 J) is u, a velocity is +0
// The exploration stream's fourth counter word is j >> 2 < 16 and the parameter noise's PARAM_NOISE_TAG, so the three
// never share a block, whatever the seed.  No transcendental function and no rounding: the host's integer form
// (tasks.reach_reset_state) gives the same bits.
constexpr uint32_t RESET_TAG = 0x52530000u;
__device__ __forceinline__ float reset_uniform(uint64_t seed, uint32_t g, uint64_t e, int k) {
    uint32_t c[4] = {g, (uint32_t)e, (uint32_t)(e >> 32), RESET_TAG | ((uint32_t)k >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t lo = (k & 1) ? c[1] : c[0], hi = (k & 1) ? c[3] : c[2];
    const uint32_t w = (k & 2) ? hi : lo;
    return (float)(w >> 8) * 0x1p-23f - 1.0f;
}

// element k of the row local actor a begins the call's i-th new episode with (R.episode: the index of the call's first)
__device__ __forceinline__ float reach_reset_value(const smx_reset_stream& R, long a, int i, int k, int J) {
    if (k >= J && k < 2 * J) return 0.0f;
    return reset_uniform(R.seed, (uint32_t)(R.actor_base + a), (uint64_t)(R.episode + i), k);
}

// the same of the `arm` row [theta (J) | omega (J) | g (2)] (tasks.arm_reset_state): the same blocks and tag, word k & 3 of
// block k >> 2 for element k; an orientation is u (in [-1, 1): well inside the joint limits), an angular
// velocity +0, a goal coordinate 0.25f * u (exact)
__device__ __forceinline__ float arm_reset_value(const smx_reset_stream& R, long a, int i, int k, int J) {
    if (k >= J && k < 2 * J) return 0.0f;
    const float u = reset_uniform(R.seed, (uint32_t)(R.actor_base + a), (uint64_t)(R.episode + i), k);
    return k < J ? u : 0.25f * u;
}

// element k of a TASK row of D elements (a task with a reset distribution)
template <int TASK>
__device__ __forceinline__ float task_reset_value(const smx_reset_stream& R, long a, int i, int k, int D) {
    if constexpr (TASK == SMX_TASK_ARM) return arm_reset_value(R, a, i, k, (D - 2) / 2);
    else return reach_reset_value(R, a, i, k, D / 3);
}

// what the entry points ask of a stream over n actors: every global actor id in [0, 2^32), an episode index >= 0
// (SMX_E_SHAPE)
inline bool reset_shape_ok(const smx_reset_stream& R, long long n) {
    return !R.enabled || (R.actor_base >= 0 && R.actor_base + n <= (1LL << 32) && R.episode >= 0);
}

// ---- the per-step disturbance of a task (struct smx_reset_stream's `reserved` word: the bits of the fp32 scale s, 0 <= s
// <= 1, zero bits: none; surreal_amd/env/tasks.py holds the definition) -------------------------------------------------------
// The draw of (seed, global actor id g, the episode under way e < 2^32, the step t within it, joint / mass j): a pure
// function of the five, through the reset stream's exact conversion.
//   x[0..3] = philox4x32_10(counter = (g, low32(e), t, DISTURB_TAG | (j >> 2)), key = (low32(seed), high32(seed)))
//   w[j]    = (float)(x[j & 3] >> 8) * 0x1p-23f - 1.0f                                                  (in [-1, 1))
// and the task adds s * w[j] (rounded) to the sum that becomes v'[j] / omega'[j], before the clamp (reach_next_v,
// arm_next_omega of smx_synth_env.inc.h).  The tag keeps these blocks apart from the reset blocks (RESET_TAG), the
// exploration stream's (fourth word < 16) and the parameter noise's (PARAM_NOISE_TAG), whatever the seed.
constexpr uint32_t DISTURB_TAG = 0x44530000u;
__device__ __forceinline__ float disturbance_uniform(uint64_t seed, uint32_t g, uint32_t e, uint32_t t, int j) {
    uint32_t c[4] = {g, e, t, DISTURB_TAG | ((uint32_t)j >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t lo = (j & 1) ? c[1] : c[0], hi = (j & 1) ? c[3] : c[2];
    const uint32_t w = (j & 2) ? hi : lo;
    return (float)(w >> 8) * 0x1p-23f - 1.0f;
}

// the stream's scale (read only when enabled; 0: no disturbance, and the tasks add nothing)
__host__ __device__ inline float reset_disturbance(const smx_reset_stream& R) {
    return R.enabled ? __builtin_bit_cast(float, R.reserved) : 0.0f;
}

// what the entry points ask of a disturbed stream whose launch has the episodes first .. first + more under way: a scale in [0, 1]
// (a NaN fails) and every such index in [0, 2^32) (SMX_E_SHAPE).  A recording launch from clock t over `steps` steps has
// episode - 1 .. episode - 1 + (t + steps - 1) / episode_len under way, an evaluation episode .. episode + episodes - 1.
inline bool disturbance_shape_ok(const smx_reset_stream& R, long long first, long long more) {
    if (!R.enabled || R.reserved == 0) return true;
    const float s = reset_disturbance(R);
    return s >= 0.0f && s <= 1.0f && first >= 0 && first < (1LL << 32) && first + more < (1LL << 32);
}
inline bool disturbance_rollout_ok(const smx_reset_stream& R, long long t, long long steps, long long episode_len) {
    if (!R.enabled || R.reserved == 0) return true;                 // (nothing is asked, and nothing divided, without a scale)
    if (episode_len < 1 || t < 0 || steps < 1) return false;
    return disturbance_shape_ok(R, R.episode - 1, (t + steps - 1) / episode_len);
}
