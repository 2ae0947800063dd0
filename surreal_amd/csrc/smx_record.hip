// Recording the steps of host-stepped environments into the replays' device rings, one launch per step for all actors,
// every actor on an episode clock of its own (include/surreal_amd.h: smx_record_ppo_window_step_f32,
// smx_record_ddpg_nstep_step_f32; the rules are those of surreal_amd/env/exp_sender_wrapper.py).
//
// Both kernels move bytes.  What a launch reads and what it writes never meet across threads:
//   * element k of an actor's cur_obs row is read (the observation acted on) and then overwritten (the next one) by the
//     ONE thread that owns k, which also puts it into the carry ring and -- at a closing step -- into the table row as
//     the window's LAST step (the transition's only step when n_step == 1): the step's inputs, never the ring slot this
//     launch writes;
//   * the N - 1 older steps of a closing window come from ring slots other than tau % N, which this launch only reads:
//     they are spread over the actor's X workgroups (grid.y), item by item, in any order.
// A field whose row width is a multiple of 4 floats and whose buffers sit on 16 bytes moves as 4-float vectors, else as
// floats (the `vec` bits, decided per field on the host).
#include "smx_common.h"
#include <string.h>

namespace {

#include "smx_synth_env.inc.h"                          // episode_account and the monitor's argument rules
#include "smx_nstep.inc.h"                              // nstep_reward

constexpr int REC_THREADS = 256;                        // the window kernel's workgroup
constexpr int REC_DDPG_THREADS = 128;                   // a transition is a few KB: one small workgroup per actor
constexpr int VEC_OBS = 1, VEC_ACT = 2, VEC_PD = 4;

struct RecW {
    int n, D, A, Hl, N, adv, S, rows, X, vec;
    const int *t, *rank;
    float* cur;
    const float *act, *pd, *hb, *cb, *onext, *rew, *done, *oreset;
    float *cobs, *cact, *crew, *cpd, *ccell;
    float *obs, *obs_next, *actions, *rewards, *dones, *pds, *cells;
    long long cursor, capacity;
    smx_episode_monitor mon;
};

struct RecD {
    int n, D, A, N, rows, vec;
    const int *t, *rank;
    float* cur;
    const float *act, *onext, *rew, *done, *oreset;
    const double* gpow;
    float *cobs, *cact, *crew;
    float *obs, *obs_next, *actions, *rewards, *dones;
    long long cursor, capacity;
    smx_episode_monitor mon;
};

// One actor's observation at this step, w elements of type V a row: the ring slot and (out / out_next non-null: a
// closing step) the table's last step and obs_next, then cur <- the next acting observation.  `older` non-null (DDPG,
// n_step > 1): out takes the ring's slot of the transition's first step instead of this step's observation.
template <typename V, int NT>
__device__ __forceinline__ void step_obs(V* cur, const V* next, const V* reset, V* ring, V* out, V* out_next,
                                         const V* older, int w, int tid) {
    for (int k = tid; k < w; k += NT) {
        const V v = cur[k];
        const V nv = next[k];
        ring[k] = v;
        if (out) {
            out[k] = older ? older[k] : v;
            out_next[k] = nv;
        }
        cur[k] = reset ? reset[k] : nv;
    }
}

// a step input row `in` (actions, pds) into its ring slot and, at a closing step, into the table (`older` as above)
template <typename V, int NT>
__device__ __forceinline__ void step_row(const V* in, V* ring, V* out, const V* older, int w, int tid) {
    for (int k = tid; k < w; k += NT) {
        const V v = in[k];
        ring[k] = v;
        if (out) out[k] = older ? older[k] : v;
    }
}

// the U older steps of a closing window, w elements of type V a step: dst[u] = ring[(j0 + u) % N], items first,
// first + stride, ... of the U w
template <typename V>
__device__ __forceinline__ void copy_older(V* dst, const V* ring, int w, int U, int N, int j0, int first, int stride) {
    const int total = U * w;
    for (int i = first; i < total; i += stride) {
        const int u = i / w, k = i - u * w;
        int s = j0 + u;
        if (s >= N) s -= N;
        dst[(size_t)u * w + k] = ring[(size_t)s * w + k];
    }
}

template <typename V>
__device__ __forceinline__ V* as(float* p) { return reinterpret_cast<V*>(p); }
template <typename V>
__device__ __forceinline__ const V* as(const float* p) { return reinterpret_cast<const V*>(p); }

// a field's step and older parts at either width
#define REC_BY_WIDTH(bit, call)                \
    do {                                       \
        if (G.vec & (bit)) { using V = f32x4; constexpr int E = 4; call; } \
        else { using V = float; constexpr int E = 1; call; }                \
    } while (0)

__global__ __launch_bounds__(REC_THREADS) void record_ppo_window_kernel(RecW G) {
    const long a = blockIdx.x;
    const int x = blockIdx.y, tid = threadIdx.x;
    const int tau = G.t[a];
    if (tau < 0) return;                                 // (refused on the host where it can see the clocks)
    const int N = G.N, D = G.D, A = G.A, adv = G.adv;
    const int j = tau + 1 - N;                           // the window that ends with this step, if one starts there
    const int rank = G.rank[a];
    const bool wclose = rank >= 0 && rank < G.rows && j >= 0 && j % adv == 0;
    if (x > 0 && !(wclose && N > 1)) return;             // the extra workgroups only move a closing window's older steps
    const size_t row = wclose ? (size_t)((G.cursor + rank) % G.capacity) : 0;
    const int wslot = tau % N;
    const size_t ring0 = (size_t)a * N, last = row * N + (N - 1);

    if (x == 0) {
        const bool done = G.done[a] != 0.0f;
        const float* reset = (done && G.oreset) ? G.oreset + a * D : nullptr;
        REC_BY_WIDTH(VEC_OBS, (step_obs<V, REC_THREADS>(
            as<V>(G.cur + a * D), as<V>(G.onext + a * D), as<V>(reset), as<V>(G.cobs + (ring0 + wslot) * D),
            wclose ? as<V>(G.obs + last * D) : nullptr, wclose ? as<V>(G.obs_next + row * D) : nullptr,
            (const V*)nullptr, D / E, tid)));
        REC_BY_WIDTH(VEC_ACT, (step_row<V, REC_THREADS>(
            as<V>(G.act + a * A), as<V>(G.cact + (ring0 + wslot) * A), wclose ? as<V>(G.actions + last * A) : nullptr,
            (const V*)nullptr, A / E, tid)));
        REC_BY_WIDTH(VEC_PD, (step_row<V, REC_THREADS>(
            as<V>(G.pd + a * 2 * A), as<V>(G.cpd + (ring0 + wslot) * 2 * A),
            wclose ? as<V>(G.pds + last * 2 * A) : nullptr, (const V*)nullptr, 2 * A / E, tid)));
        if (tid == 0) {
            const float rew = G.rew[a];
            G.crew[ring0 + wslot] = rew;
            if (wclose) G.rewards[last] = rew;
            if (G.mon.ep_reward) episode_account(G.mon, a, rew, done);
        }
        if (wclose)
            for (int u = tid; u < N; u += REC_THREADS) G.dones[row * N + u] = (done && u == N - 1) ? 1.0f : 0.0f;
        if (G.ccell) {
            // [2, Hl] as one run of 2 Hl floats: h then c
            const int Hl = G.Hl, S = G.S;
            float* cc = G.ccell + (size_t)a * S * 2 * Hl;
            const bool put = G.hb && tau % adv == 0;
            for (int c = tid; c < 2 * Hl; c += REC_THREADS) {
                float v = 0.0f;
                if (put) {
                    v = c < Hl ? G.hb[a * Hl + c] : G.cb[a * Hl + c - Hl];
                    cc[(size_t)((tau / adv) % S) * 2 * Hl + c] = v;
                }
                if (wclose && G.cells) {
                    if (!(put && j == tau)) v = cc[(size_t)((j / adv) % S) * 2 * Hl + c];    // (j == tau: n_step 1)
                    G.cells[row * 2 * Hl + c] = v;
                }
            }
        }
    }
    if (!(wclose && N > 1)) return;
    // ---- the window's N - 1 older steps, out of the rings in episode order --------------------------------------------
    const int first = x * REC_THREADS + tid, stride = G.X * REC_THREADS, j0 = j % N, U = N - 1;
    REC_BY_WIDTH(VEC_OBS, (copy_older<V>(as<V>(G.obs + row * N * D), as<V>(G.cobs + ring0 * D), D / E, U, N, j0, first,
                                         stride)));
    REC_BY_WIDTH(VEC_PD, (copy_older<V>(as<V>(G.pds + row * N * 2 * A), as<V>(G.cpd + ring0 * 2 * A), 2 * A / E, U, N, j0,
                                        first, stride)));
    REC_BY_WIDTH(VEC_ACT, (copy_older<V>(as<V>(G.actions + row * N * A), as<V>(G.cact + ring0 * A), A / E, U, N, j0, first,
                                         stride)));
    copy_older<float>(G.rewards + row * N, G.crew + ring0, 1, U, N, j0, first, stride);
}

__global__ __launch_bounds__(REC_DDPG_THREADS) void record_ddpg_nstep_kernel(RecD G) {
    const long a = blockIdx.x;
    const int tid = threadIdx.x;
    const int tau = G.t[a];
    if (tau < 0) return;
    const int N = G.N, D = G.D, A = G.A;
    const int rank = G.rank[a];
    const bool emits = rank >= 0 && rank < G.rows && tau >= N - 1;
    const size_t row = emits ? (size_t)((G.cursor + rank) % G.capacity) : 0;
    const int wslot = tau % N, jslot = (tau + 1) % N;    // transition j = tau - N + 1 sits in slot j % N
    const bool ring_first = N > 1;                       // (n_step 1: the transition's first step is this one)
    const size_t ring0 = (size_t)a * N;
    const bool done = G.done[a] != 0.0f;
    const float* reset = (done && G.oreset) ? G.oreset + a * D : nullptr;
    REC_BY_WIDTH(VEC_OBS, (step_obs<V, REC_DDPG_THREADS>(
        as<V>(G.cur + a * D), as<V>(G.onext + a * D), as<V>(reset), as<V>(G.cobs + (ring0 + wslot) * D),
        emits ? as<V>(G.obs + row * D) : nullptr, emits ? as<V>(G.obs_next + row * D) : nullptr,
        ring_first ? as<V>((const float*)G.cobs + (ring0 + jslot) * D) : nullptr, D / E, tid)));
    REC_BY_WIDTH(VEC_ACT, (step_row<V, REC_DDPG_THREADS>(
        as<V>(G.act + a * A), as<V>(G.cact + (ring0 + wslot) * A), emits ? as<V>(G.actions + row * A) : nullptr,
        ring_first ? as<V>((const float*)G.cact + (ring0 + jslot) * A) : nullptr, A / E, tid)));
    if (tid == 0) {
        const float rew = G.rew[a];
        float* cr = G.crew + ring0;
        cr[wslot] = rew;
        if (emits) {
            G.rewards[row] = nstep_reward(cr, G.gpow, N, tau);
            G.dones[row] = done ? 1.0f : 0.0f;
        }
        if (G.mon.ep_reward) episode_account(G.mon, a, rew, done);
    }
}

#undef REC_BY_WIDTH

// ---- host side -------------------------------------------------------------------------------------------------------

bool on16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the clocks and ranks as the host holds them (either may be null: not looked at): clocks >= 0, ranks in [-1, n) and as
// many closing actors as the caller reserved rows for
bool clocks_ok(const int32_t* t_host, const int32_t* rank_host, int n, int rows) {
    int closing = 0;
    for (int a = 0; a < n; ++a) {
        if (t_host && t_host[a] < 0) return false;
        if (rank_host) {
            if (rank_host[a] < -1 || rank_host[a] >= n) return false;
            closing += rank_host[a] >= 0;
        }
    }
    return !rank_host || closing == rows;
}

template <typename Block>
bool step_pointers(const Block& a) {
    return a.t && a.rank && a.cur_obs && a.step_actions && a.step_obs_next && a.step_rewards && a.step_dones &&
           a.carry_obs && a.carry_act && a.carry_rew && a.obs && a.obs_next && a.actions && a.rewards && a.dones;
}
// positive sizes, a cursor inside the ring, a row for every actor (all of them may close in one step)
template <typename Block>
bool step_shape_ok(const Block& a) {
    return a.n > 0 && a.D > 0 && a.A > 0 && a.n_step > 0 && a.capacity > 0 && a.cursor >= 0 && a.cursor < a.capacity &&
           a.n <= a.capacity && a.rows >= 0 && a.rows <= a.n;
}

// the workgroups per actor that move a closing window's older steps: 8 KB each, and no more than 16 workgroups per CU
// over the launch's closing actors
int window_copy_workgroups(const smx_record_ppo_window_step& a) {
    if (a.rows == 0 || a.n_step == 1) return 1;
    const long long bytes = (long long)(a.n_step - 1) * (a.D + 3 * a.A + 1) * 4;
    long long X = (bytes + 8191) / 8192;
    const long long room = 16LL * smx_cu_count() / a.rows;
    if (X > room) X = room;
    if (X > 64) X = 64;
    return X < 1 ? 1 : (int)X;
}

}  // namespace

extern "C" int smx_record_ppo_window_step_f32(const struct smx_record_ppo_window_step* a, smx_stream_t stream) {
    SMX_REQUIRE(a && step_pointers(*a) && a->step_pds && a->carry_pd && a->pds, SMX_E_NULL);
    SMX_REQUIRE((a->h_before == nullptr) == (a->c_before == nullptr) && episode_pointers_ok(a->mon), SMX_E_NULL);
    // an LSTM policy's cells: the ring whenever a state comes in or a window's cells go out
    SMX_REQUIRE((!a->h_before && !a->cells) || a->carry_cells, SMX_E_NULL);
    SMX_REQUIRE(step_shape_ok(*a) && a->hidden >= 0 && a->advance > 0 && a->advance <= a->n_step, SMX_E_SHAPE);
    SMX_REQUIRE(!a->carry_cells || a->hidden > 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->copy_workgroups >= 0 && a->copy_workgroups <= 1024 && episode_shape_ok(a->mon), SMX_E_SHAPE);
    SMX_REQUIRE(clocks_ok(a->t_host, a->rank_host, a->n, a->rows), SMX_E_SHAPE);
    RecW G;
    memset(&G, 0, sizeof(G));
    G.n = a->n; G.D = a->D; G.A = a->A; G.Hl = a->hidden; G.N = a->n_step; G.adv = a->advance;
    G.S = (a->n_step + a->advance - 1) / a->advance;
    G.rows = a->rows;
    G.X = a->copy_workgroups ? a->copy_workgroups : window_copy_workgroups(*a);
    G.t = a->t; G.rank = a->rank;
    G.cur = a->cur_obs; G.act = a->step_actions; G.pd = a->step_pds; G.hb = a->h_before; G.cb = a->c_before;
    G.onext = a->step_obs_next; G.rew = a->step_rewards; G.done = a->step_dones; G.oreset = a->step_obs_reset;
    G.cobs = a->carry_obs; G.cact = a->carry_act; G.crew = a->carry_rew; G.cpd = a->carry_pd; G.ccell = a->carry_cells;
    G.obs = a->obs; G.obs_next = a->obs_next; G.actions = a->actions; G.rewards = a->rewards; G.dones = a->dones;
    G.pds = a->pds; G.cells = a->cells;
    G.cursor = a->cursor; G.capacity = a->capacity;
    G.mon = a->mon;
    if (a->D % 4 == 0 && on16(a->cur_obs) && on16(a->step_obs_next) && on16(a->step_obs_reset) && on16(a->carry_obs) &&
        on16(a->obs) && on16(a->obs_next))
        G.vec |= VEC_OBS;
    if (a->A % 4 == 0 && on16(a->step_actions) && on16(a->carry_act) && on16(a->actions)) G.vec |= VEC_ACT;
    if (a->A % 2 == 0 && on16(a->step_pds) && on16(a->carry_pd) && on16(a->pds)) G.vec |= VEC_PD;
    hipLaunchKernelGGL(record_ppo_window_kernel, dim3(a->n, G.X), dim3(REC_THREADS), 0, smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_record_ddpg_nstep_step_f32(const struct smx_record_ddpg_nstep_step* a, smx_stream_t stream) {
    SMX_REQUIRE(a && step_pointers(*a) && a->gpow && episode_pointers_ok(a->mon), SMX_E_NULL);
    SMX_REQUIRE(step_shape_ok(*a) && episode_shape_ok(a->mon), SMX_E_SHAPE);
    SMX_REQUIRE(clocks_ok(a->t_host, a->rank_host, a->n, a->rows), SMX_E_SHAPE);
    RecD G;
    memset(&G, 0, sizeof(G));
    G.n = a->n; G.D = a->D; G.A = a->A; G.N = a->n_step; G.rows = a->rows;
    G.t = a->t; G.rank = a->rank;
    G.cur = a->cur_obs; G.act = a->step_actions; G.onext = a->step_obs_next; G.rew = a->step_rewards;
    G.done = a->step_dones; G.oreset = a->step_obs_reset; G.gpow = a->gpow;
    G.cobs = a->carry_obs; G.cact = a->carry_act; G.crew = a->carry_rew;
    G.obs = a->obs; G.obs_next = a->obs_next; G.actions = a->actions; G.rewards = a->rewards; G.dones = a->dones;
    G.cursor = a->cursor; G.capacity = a->capacity;
    G.mon = a->mon;
    if (a->D % 4 == 0 && on16(a->cur_obs) && on16(a->step_obs_next) && on16(a->step_obs_reset) && on16(a->carry_obs) &&
        on16(a->obs) && on16(a->obs_next))
        G.vec |= VEC_OBS;
    if (a->A % 4 == 0 && on16(a->step_actions) && on16(a->carry_act) && on16(a->actions)) G.vec |= VEC_ACT;
    hipLaunchKernelGGL(record_ddpg_nstep_kernel, dim3(a->n), dim3(REC_DDPG_THREADS), 0, smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}
