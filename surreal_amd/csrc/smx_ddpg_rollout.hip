// DDPG's acting loop on the device, recorded straight into the uniform replay's ring (surreal/agent/base.py:244-271
// the per-step loop of a rollout worker; surreal/agent/ddpg_agent.py:155-184 act: actor -> clip -> + exploration noise
// -> clip; surreal/agent/action_noise.py the Gaussian and Ornstein-Uhlenbeck processes; the n-step transitions of
// surreal/env/exp_sender_wrapper.py:72-112 ExpSenderWrapperSSARNStepBootstrap, which run on the host there).
//
// Two entry points share the per-step semantics (include/surreal_amd.h, struct smx_ddpg_rollout):
//   smx_synth_ddpg_rollout_f32  a workgroup OWNS 4, 8 or 16 actors and walks them through all steps in one launch, as
//                               smx_rollout.hip does for PPO: the actor's three layers on the 4-row v_mfma_f32_4x4x1 loop
//                               of smx_rows4_mma.inc.h (the smx_epoch_pack_f32 copy streamed from L2), then the tanh
//                               head, the noise, the environment step and the n-step record.  The state stays in
//                               registers for the whole rollout.
//   smx_synth_ddpg_step_f32     one step for all actors given the actor's output mu [n, A] from any forward (LayerNorm
//                               actors, unsupported shapes; with smx_epoch_forward_f32 the persistent kernel's
//                               two-launch reference).
//
// The open transitions of an actor (observation, action, reward of its last n_step steps) live in a ring of n_step
// slots in HBM, slot tau % n_step for episode step tau: every value is written and later read by the SAME lane, so no
// barrier orders them, and they carry from one call to the next.  Transition j = tau - n_step + 1 closes at step tau;
// the k-th closing step of a call writes actor a to ring row (cursor + k n + a) mod capacity.
#include "smx_common.h"
#include <string.h>

namespace {
#include "smx_epoch_pack.inc.h"
#include "smx_epoch_mma.inc.h"
#include "smx_rows4_mma.inc.h"

constexpr int DLDO = 36;          // row stride of the mu tile in LDS (<= 32 actions)
constexpr int DMAX_A = 32;
constexpr int DNWV = 8;           // wavefronts per workgroup (two per SIMD)
constexpr int DNTH = 64 * DNWV;
constexpr int DKV = 8;            // observation elements a lane owns per row (D <= 64 DKV)
constexpr int D_MAX_LDS = 150 * 1024;
constexpr int D_EXCLUSIVE_LDS = 84 * 1024;   // one workgroup per CU: each streams the packed weights by itself

struct DArgs {
    const float *P1, *P2, *P3, *b1, *b2, *b3;
    int D, H1, H2, A, n, steps, t0, episode_len, N, noise;
    const float* eps;
    const double* sigmas;
    double theta, dt, root_dt;
    const double* gpow;
    double* ou;
    float* state;
    const float* init_state;
    float *cobs, *cact, *crew;
    float *obs, *obs_next, *act, *rew, *done;
    long long cursor, capacity;
    int ldx, ldh1, ldh2, off_h1, off_h2, off_out, off_act, off_kmod;
};

__device__ __forceinline__ float clip1(float a) {
    if (a == a) a = fminf(fmaxf(a, -1.0f), 1.0f);          // (numpy's clip keeps a NaN)
    return a;
}

// ddpg_agent.py:176-184 on one (actor, action) pair: clip, the exploration noise in fp64 rounded once into the fp32
// action (action += noise() on a float32 array), clip.  x: the pair's OU state, zeroed at the episode start (pre_episode,
// ddpg_agent.py:205-208).  The expressions keep action_noise.py's evaluation order.
__device__ __forceinline__ float explore(float mu, int noise, float e, double sig, double theta, double dt, double root_dt,
                                         int tau, double& x) {
    float a = clip1(mu);
    if (noise == SMX_DDPG_NOISE_GAUSSIAN) {
        a = (float)((double)a + (0.0 + sig * (double)e));
    } else if (noise == SMX_DDPG_NOISE_OU) {
        if (tau == 0) x = 0.0;
        x = (x + (theta * (0.0 - x)) * dt) + (sig * root_dt) * (double)e;
        a = (float)((double)a + x);
    }
    return clip1(a);
}

// the closing transition's reward: r_j + g[e] r_{j+1} + ..., left to right in fp64 (the host wrapper's `+=` sequence),
// exponents as ExpSenderWrapperSSARNStepBootstrap._discount_exponent (the reference's ramp-up quirk included)
__device__ __forceinline__ float nstep_reward(const float* crew_a, const double* gpow, int N, int tau) {
    const int j = tau - N + 1;
    double R = (double)crew_a[j % N];
    for (int u = j + 1; u <= tau; ++u) {
        const int e = (u >= N - 1) ? (u - j) : (N - 1 - j);
        R = R + gpow[e] * (double)crew_a[u % N];
    }
    return (float)R;
}

__device__ __forceinline__ long long ring_row(const DArgs& G, int kemit, long a) {
    return (G.cursor + (long long)kemit * G.n + a) % G.capacity;
}

// RG row groups of four actors per workgroup; NT feature tiles a wave carries per pass.  The layer sums of an actor do
// not depend on RG or NT (k ascending within each kq class, then the classes meet): every block size gives the same bits.
template <int RG, int NT>
__global__ __launch_bounds__(DNTH) void ddpg_rollout_kernel(DArgs G) {
    constexpr int RB = 4 * RG;                       // actors per workgroup
    constexpr int WPR = RB < DNWV ? DNWV / RB : 1;   // wavefronts per actor row in the environment phase
    constexpr int RPW = RB > DNWV ? RB / DNWV : 1;   // actor rows per wavefront
    constexpr int KPL = DKV / WPR;                   // observation elements a lane owns per row
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fm = lane & 15, kq = lane >> 4;
    const long row0 = (long)blockIdx.x * RB;
    int nrows = G.n - (int)row0;
    if (nrows > RB) nrows = RB;
    const int D = G.D, A = G.A, N = G.N;
    float* xs = sm;
    float* h1s = sm + G.off_h1;
    float* h2s = sm + G.off_h2;
    float* outs = sm + G.off_out;
    float* s_act = sm + G.off_act;                   // [RB][DMAX_A] the actions of this step (unused columns stay 0)
    int* kmod = (int*)(sm + G.off_kmod);             // [D] k % A
    const int ldx = G.ldx, ldh1 = G.ldh1, ldh2 = G.ldh2;

    // ---- once: clear the tiles (their padding columns and rows must read as zeros), k % A to LDS, the state of the
    // environment phase's elements to registers: wave wv owns rows RPW (wv / WPR) .., a lane the elements
    // k = lane + 64 (part + WPR i)
    for (int i = tid; i < G.off_kmod; i += DNTH) sm[i] = 0.f;
    for (int k = tid; k < D; k += DNTH) kmod[k] = k % A;
    const int erow0 = RPW * (wv / WPR), part = wv % WPR;
    float st[RPW][KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int k = lane + 64 * (part + WPR * i);
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;
            st[rr][i] = (k < D && r < nrows) ? G.state[(row0 + r) * D + k] : 0.f;
        }
    }
    SMX_LDS_BARRIER();
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int r = erow0 + rr;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int k = lane + 64 * (part + WPR * i);
            if (k < D && r < nrows) xs[r * ldx + k] = st[rr][i];
        }
    }
    int am[KPL];
    float dr[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int k = lane + 64 * (part + WPR * i);
        am[i] = k < D ? kmod[k] : 0;
        dr[i] = 0.01f * (float)(((37 * k) % 17) - 8);
    }
    // the head's (actor, action) pair of this lane: its sigma and OU state for the whole rollout
    const int hr = tid / A, hj = tid - hr * A;       // RB x A <= 512 pairs
    const bool head = hr < nrows;
    const long ha = row0 + hr;
    double sig = 0.0, x = 0.0;
    if (head) {
        if (G.noise != SMX_DDPG_NOISE_NONE) sig = G.sigmas[ha];
        if (G.noise == SMX_DDPG_NOISE_OU) x = G.ou[ha * A + hj];
    }
    SMX_LDS_BARRIER();

    int tau = G.t0, kemit = 0;
#pragma unroll 1
    for (int step = 0; step < G.steps; ++step) {
        float ev = 0.f;                              // this step's draw, requested before the layers
        if (G.eps && head) ev = G.eps[((size_t)step * G.n + ha) * A + hj];
        // ---- the actor's three layers (ReLU, ReLU, tanh) --------------------------------------------------------
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            const float* Wp = l == 0 ? G.P1 : (l == 1 ? G.P2 : G.P3);
            const float* bias = l == 0 ? G.b1 : (l == 1 ? G.b2 : G.b3);
            const int H = l == 0 ? G.H1 : (l == 1 ? G.H2 : A);
            const int K = l == 0 ? D : (l == 1 ? G.H1 : G.H2);
            const float* in_lds = l == 0 ? xs : (l == 1 ? h1s : h2s);
            const int ldi = l == 0 ? ldx : (l == 1 ? ldh1 : ldh2);
            float* out_lds = l == 0 ? h1s : (l == 1 ? h2s : outs);
            const int ldo = l == 0 ? ldh1 : (l == 1 ? ldh2 : DLDO);
            const int tiles = (H + 15) >> 4;
            const int C2 = pack_chunks(K);
            const rsrc_t rw = make_rsrc(Wp, (unsigned)tiles * (unsigned)C2 * 2048u);
            const rsrc_t rbias = make_rsrc(bias, (unsigned)H * 4u);
#pragma unroll 1
            for (int tb = 0; tb < tiles; tb += DNWV * NT) {
                const int t0 = tb + wv;
                if (t0 >= tiles) continue;                            // (wave-uniform)
                float bs[NT];
#pragma unroll
                for (int g = 0; g < NT; ++g) {
                    const int f = 16 * (t0 + DNWV * g) + fm;
                    bs[g] = ld4(rbias, (f < H) ? (unsigned)f * 4u : OOB);
                }
                f32x4 acc[NT][RG];
#pragma unroll
                for (int g = 0; g < NT; ++g)
#pragma unroll
                    for (int r = 0; r < RG; ++r) acc[g][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
                fwd_tiles4<NT, RG, true>(acc, rw, tiles, C2, in_lds, ldi, t0, DNWV, lane);
#pragma unroll
                for (int g = 0; g < NT; ++g) {
                    const int f = 16 * (t0 + DNWV * g) + fm;
                    if (t0 + DNWV * g < tiles) {                      // (wave-uniform)
#pragma unroll
                        for (int r = 0; r < RG; ++r) {
                            float z = meet_rows(acc[g][r]);
                            z += bs[g];
                            z = (l == 2) ? tanhf(z) : ((z < 0.f) ? 0.f : z);
                            out_lds[(4 * r + kq) * ldo + f] = (f < H) ? z : 0.f;
                        }
                    }
                }
            }
            SMX_LDS_BARRIER();
        }
        const bool emit = tau >= N - 1;
        const int slot = tau % N, jslot = (tau + 1) % N;   // (transition j = tau - N + 1 sits in slot j % N)
        const bool done = (tau + 1 >= G.episode_len);
        // ---- exploration: one (actor, action) pair per lane ------------------------------------------------------
        if (head) {
            const float a = explore(outs[hr * DLDO + hj], G.noise, ev, sig, G.theta, G.dt, G.root_dt, tau, x);
            s_act[hr * DMAX_A + hj] = a;
            float* ca = G.cact + (size_t)ha * N * A + hj;
            ca[(size_t)slot * A] = a;
            if (emit) G.act[ring_row(G, kemit, ha) * A + hj] = ca[(size_t)jslot * A];
        }
        SMX_LDS_BARRIER();
        // ---- environment step (smx_synth_env_step_f32's expressions), n-step record, next x tile -------------------
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;                      // wave-uniform
            if (r < nrows) {
                const long a = row0 + r;
                const long long row = emit ? ring_row(G, kemit, a) : 0;
                float* co = G.cobs + (size_t)a * N * D;
                float sn0 = 0.f;
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    const int k = lane + 64 * (part + WPR * i);
                    if (k < D) {
                        const float ac = s_act[r * DMAX_A + am[i]];
                        const float s = st[rr][i];
                        float sn = (0.9f * s + 0.5f * ac) + dr[i];
                        sn = fminf(fmaxf(sn, -10.0f), 10.0f);
                        co[(size_t)slot * D + k] = s;
                        if (emit) {
                            G.obs[row * D + k] = co[(size_t)jslot * D + k];
                            G.obs_next[row * D + k] = sn;
                        }
                        if (i == 0) sn0 = sn;
                        const float next = done ? G.init_state[a * D + k] : sn;
                        st[rr][i] = next;
                        xs[r * ldx + k] = next;
                    }
                }
                if (lane == 0 && part == 0) {               // (k == 0 lives in lane 0, i == 0 of the row's first wave)
                    double q = 0.0;
                    for (int j = 0; j < A; ++j) {
                        const double v = (double)s_act[r * DMAX_A + j];
                        q += v * v;
                    }
                    float* cr = G.crew + (size_t)a * N;
                    cr[slot] = (float)(-0.1 * q + 0.05 * (double)sn0);
                    if (emit) {
                        G.rew[row] = nstep_reward(cr, G.gpow, N, tau);
                        G.done[row] = done ? 1.0f : 0.0f;
                    }
                }
            }
        }
        if (emit) ++kemit;
        tau = done ? 0 : tau + 1;
        SMX_LDS_BARRIER();
    }
    // ---- the states the actors and their noise processes are left in ------------------------------------------------
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int r = erow0 + rr;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int k = lane + 64 * (part + WPR * i);
            if (k < D && r < nrows) G.state[(row0 + r) * D + k] = st[rr][i];
        }
    }
    if (head && G.noise == SMX_DDPG_NOISE_OU) G.ou[ha * A + hj] = x;
}

// one step for four actors per workgroup, one wavefront each, given mu [n, A] (ld_mu)
constexpr int SA_MAX = 64;
__global__ __launch_bounds__(256) void ddpg_step_kernel(DArgs G, const float* mu, long long ld_mu) {
    __shared__ float s_act[4][SA_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long a = (long)blockIdx.x * 4 + w;
    const int D = G.D, A = G.A, N = G.N, tau = G.t0;
    const bool live = a < G.n;
    const bool emit = tau >= N - 1;
    const int slot = tau % N, jslot = (tau + 1) % N;   // (transition j = tau - N + 1 sits in slot j % N)
    const bool done = (tau + 1 >= G.episode_len);
    const long long row = (live && emit) ? ring_row(G, 0, a) : 0;
    if (live && lane < A) {
        double x = 0.0, sig = 0.0;
        if (G.noise != SMX_DDPG_NOISE_NONE) sig = G.sigmas[a];
        if (G.noise == SMX_DDPG_NOISE_OU) x = G.ou[a * A + lane];
        const float e = G.eps ? G.eps[a * A + lane] : 0.f;
        const float v = explore(mu[a * ld_mu + lane], G.noise, e, sig, G.theta, G.dt, G.root_dt, tau, x);
        if (G.noise == SMX_DDPG_NOISE_OU) G.ou[a * A + lane] = x;
        s_act[w][lane] = v;
        float* ca = G.cact + (size_t)a * N * A + lane;
        ca[(size_t)slot * A] = v;
        if (emit) G.act[row * A + lane] = ca[(size_t)jslot * A];
    }
    __syncthreads();
    if (!live) return;
    float* co = G.cobs + (size_t)a * N * D;
    float sn0 = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float ac = s_act[w][k % A];
        const float s = G.state[a * D + k];
        float sn = (0.9f * s + 0.5f * ac) + 0.01f * (float)(((37 * k) % 17) - 8);
        sn = fminf(fmaxf(sn, -10.0f), 10.0f);
        co[(size_t)slot * D + k] = s;
        if (emit) {
            G.obs[row * D + k] = co[(size_t)jslot * D + k];
            G.obs_next[row * D + k] = sn;
        }
        if (k == 0) sn0 = sn;
        G.state[a * D + k] = done ? G.init_state[a * D + k] : sn;
    }
    if (lane == 0) {
        double q = 0.0;
        for (int j = 0; j < A; ++j) {
            const double v = (double)s_act[w][j];
            q += v * v;
        }
        float* cr = G.crew + (size_t)a * N;
        cr[slot] = (float)(-0.1 * q + 0.05 * (double)sn0);
        if (emit) {
            G.rew[row] = nstep_reward(cr, G.gpow, N, tau);
            G.done[row] = done ? 1.0f : 0.0f;
        }
    }
}

inline int rr64(int v) { return (v + 63) & ~63; }

// row strides = 16 mod 64 words (smx_rollout.hip's carve for the 4-row loop); a tile holds pack_chunks(K) * 32 + 8
// columns at least
int carve(DArgs& G, int RB) {
    G.ldx = rr64(G.D + 40) + 16; G.ldh1 = rr64(G.H1 + 40) + 16; G.ldh2 = rr64(G.H2 + 40) + 16;
    G.off_h1 = RB * G.ldx;
    G.off_h2 = G.off_h1 + RB * G.ldh1;
    G.off_out = G.off_h2 + RB * G.ldh2;
    G.off_act = G.off_out + RB * DLDO;
    G.off_kmod = G.off_act + RB * DMAX_A;
    return (G.off_kmod + G.D) * (int)sizeof(float);
}

// the fields both entry points take from the argument block
int common_args(const struct smx_ddpg_rollout* a, DArgs& G) {
    SMX_REQUIRE(a && a->state && a->init_state && a->gpow && a->carry_obs && a->carry_act && a->carry_rew, SMX_E_NULL);
    SMX_REQUIRE(a->obs && a->obs_next && a->actions && a->rewards && a->dones, SMX_E_NULL);
    SMX_REQUIRE(a->n > 0 && a->D > 0 && a->A > 0 && a->n_step > 0 && a->episode_len > 0 && a->t >= 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->capacity > 0 && a->cursor >= 0 && a->cursor < a->capacity, SMX_E_SHAPE);
    SMX_REQUIRE(a->noise_type >= SMX_DDPG_NOISE_NONE && a->noise_type <= SMX_DDPG_NOISE_OU, SMX_E_SHAPE);
    SMX_REQUIRE(a->noise_type == SMX_DDPG_NOISE_NONE || (a->eps && a->sigmas), SMX_E_NULL);
    SMX_REQUIRE(a->noise_type != SMX_DDPG_NOISE_OU || a->ou, SMX_E_NULL);
    memset(&G, 0, sizeof(G));
    G.D = a->D; G.A = a->A; G.n = a->n; G.steps = a->steps; G.t0 = a->t; G.episode_len = a->episode_len;
    G.N = a->n_step; G.noise = a->noise_type;
    G.eps = a->noise_type == SMX_DDPG_NOISE_NONE ? nullptr : a->eps;
    G.sigmas = a->sigmas; G.theta = a->theta; G.dt = a->dt; G.root_dt = a->root_dt;
    G.gpow = a->gpow; G.ou = a->ou;
    G.state = a->state; G.init_state = a->init_state;
    G.cobs = a->carry_obs; G.cact = a->carry_act; G.crew = a->carry_rew;
    G.obs = a->obs; G.obs_next = a->obs_next; G.act = a->actions; G.rew = a->rewards; G.done = a->dones;
    G.cursor = a->cursor; G.capacity = a->capacity;
    return SMX_OK;
}

// closing steps among `steps` steps from clock t
long long emitting_steps(int t, int steps, int episode_len, int N) {
    long long m = 0;
    for (int s = 0; s < steps; ++s) {
        if (t >= N - 1) ++m;
        t = (t + 1 >= episode_len) ? 0 : t + 1;
    }
    return m;
}

}  // namespace

extern "C" int32_t smx_synth_ddpg_rollout_supported(int32_t D, int32_t H1, int32_t H2, int32_t A) {
    if (!(D > 0 && H1 > 0 && H2 > 0 && A > 0 && A <= DMAX_A && H1 % 4 == 0 && H2 % 4 == 0)) return 0;
    if (!(H1 <= 640 && H2 <= 640 && D <= 64 * DKV)) return 0;
    DArgs G;
    memset(&G, 0, sizeof(G));
    G.D = D; G.H1 = H1; G.H2 = H2; G.A = A;
    return carve(G, 16) <= D_MAX_LDS;
}

extern "C" int smx_synth_ddpg_rollout_f32(const struct smx_ddpg_rollout* a, smx_stream_t stream) {
    SMX_REQUIRE(a && a->net && a->packed, SMX_E_NULL);
    const smx_mlp3_t& net = *a->net;
    SMX_REQUIRE(smx_synth_ddpg_rollout_supported(net.D, net.H1, net.H2, net.OUT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(net.D == a->D && net.OUT == a->A && a->steps > 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->actors_per_workgroup == 0 || a->actors_per_workgroup == 4 || a->actors_per_workgroup == 8 ||
                a->actors_per_workgroup == 16, SMX_E_SHAPE);
    SMX_REQUIRE(((uintptr_t)a->packed & 15) == 0 && ((uintptr_t)net.b1 & 3) == 0, SMX_E_ALIGN);
    DArgs G;
    const int rc = common_args(a, G);
    if (rc != SMX_OK) return rc;
    // two workgroups must never write the same ring row: all n m rows of the call are distinct
    SMX_REQUIRE((long long)a->n * emitting_steps(a->t, a->steps, a->episode_len, a->n_step) <= a->capacity, SMX_E_SHAPE);
    G.P1 = a->packed;
    G.P2 = a->packed + 4 * pack_off(net.D, net.H1, net.H2, net.OUT, 1);
    G.P3 = a->packed + 4 * pack_off(net.D, net.H1, net.H2, net.OUT, 2);
    G.b1 = net.b1; G.b2 = net.b2; G.b3 = net.b3; G.H1 = net.H1; G.H2 = net.H2;
    // 4 or 8 actors per workgroup while that grid fits the chip once, else 16
    int rb = a->actors_per_workgroup;
    if (rb == 0) {
        rb = 16;
        for (int c = 4; c <= 8; c *= 2)
            if ((a->n + c - 1) / c <= smx_cu_count()) { rb = c; break; }
    }
    int lds = carve(G, rb);
    if (lds < D_EXCLUSIVE_LDS) lds = D_EXCLUSIVE_LDS;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)ddpg_rollout_kernel<1, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, D_MAX_LDS);
        (void)hipFuncSetAttribute((const void*)ddpg_rollout_kernel<2, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, D_MAX_LDS);
        (void)hipFuncSetAttribute((const void*)ddpg_rollout_kernel<4, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, D_MAX_LDS);
        attr_set = true;
    }
    const int blocks = (a->n + rb - 1) / rb;
    if (rb == 4) hipLaunchKernelGGL((ddpg_rollout_kernel<1, 3>), dim3(blocks), dim3(DNTH), lds, smx_s(stream), G);
    else if (rb == 8) hipLaunchKernelGGL((ddpg_rollout_kernel<2, 3>), dim3(blocks), dim3(DNTH), lds, smx_s(stream), G);
    else hipLaunchKernelGGL((ddpg_rollout_kernel<4, 2>), dim3(blocks), dim3(DNTH), lds, smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_ddpg_step_f32(const struct smx_ddpg_rollout* a, const float* mu, int64_t ld_mu,
                                       smx_stream_t stream) {
    SMX_REQUIRE(mu, SMX_E_NULL);
    DArgs G;
    const int rc = common_args(a, G);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(a->A <= SA_MAX && ld_mu >= a->A, SMX_E_SHAPE);
    SMX_REQUIRE((long long)a->n <= a->capacity, SMX_E_SHAPE);
    G.steps = 1;
    hipLaunchKernelGGL(ddpg_step_kernel, dim3((a->n + 3) / 4), dim3(256), 0, smx_s(stream), G, mu, (long long)ld_mu);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}
