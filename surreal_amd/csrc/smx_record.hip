// Recording the steps of host-stepped environments into the replays' device rings, one launch per step for all actors,
// every actor on an episode clock of its own (include/surreal_amd.h: smx_record_ppo_window_step_f32,
// smx_record_ddpg_nstep_step_f32; the rules are those of surreal_amd/env/exp_sender_wrapper.py), and the same two steps
// for actors with a camera (smx_record_ppo_pixel_window_step, smx_record_ddpg_pixel_nstep_step: further down, with the
// frames' own statement of the invariant below).
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

// one actor's step of the moving windows: workgroup x of the X that share the actor (x == 0: the step itself)
__device__ __forceinline__ void ppo_window_step(const RecW& G, long a, int x, int X, int tid) {
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
    const int first = x * REC_THREADS + tid, stride = X * REC_THREADS, j0 = j % N, U = N - 1;
    REC_BY_WIDTH(VEC_OBS, (copy_older<V>(as<V>(G.obs + row * N * D), as<V>(G.cobs + ring0 * D), D / E, U, N, j0, first,
                                         stride)));
    REC_BY_WIDTH(VEC_PD, (copy_older<V>(as<V>(G.pds + row * N * 2 * A), as<V>(G.cpd + ring0 * 2 * A), 2 * A / E, U, N, j0,
                                        first, stride)));
    REC_BY_WIDTH(VEC_ACT, (copy_older<V>(as<V>(G.actions + row * N * A), as<V>(G.cact + ring0 * A), A / E, U, N, j0, first,
                                         stride)));
    copy_older<float>(G.rewards + row * N, G.crew + ring0, 1, U, N, j0, first, stride);
}

__global__ __launch_bounds__(REC_THREADS) void record_ppo_window_kernel(RecW G) {
    ppo_window_step(G, blockIdx.x, blockIdx.y, G.X, threadIdx.x);
}

// one actor's step of the n-step transitions, by a workgroup of NT threads
template <int NT>
__device__ __forceinline__ void ddpg_nstep_step(const RecD& G, long a, int tid) {
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
    REC_BY_WIDTH(VEC_OBS, (step_obs<V, NT>(
        as<V>(G.cur + a * D), as<V>(G.onext + a * D), as<V>(reset), as<V>(G.cobs + (ring0 + wslot) * D),
        emits ? as<V>(G.obs + row * D) : nullptr, emits ? as<V>(G.obs_next + row * D) : nullptr,
        ring_first ? as<V>((const float*)G.cobs + (ring0 + jslot) * D) : nullptr, D / E, tid)));
    REC_BY_WIDTH(VEC_ACT, (step_row<V, NT>(
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

__global__ __launch_bounds__(REC_DDPG_THREADS) void record_ddpg_nstep_kernel(RecD G) {
    ddpg_nstep_step<REC_DDPG_THREADS>(G, blockIdx.x, threadIdx.x);
}

#undef REC_BY_WIDTH

// ---- the same steps for actors with a camera -----------------------------------------------------------------------------
// The frame rule of the synthetic camera steps (smx_rollout.hip, above struct PArgs) with the clock PER ACTOR: tau = t[a],
// p = hist_pos (one counter for all actors: every actor receives one frame per step), Hd = hist_len >= N + S.  The frame
// of step u of actor a's current episode sits in slot (p - tau + u) mod Hd; slot (p + 1) mod Hd takes the reset frame
// where done, else the next frame (the terminal frame never enters the history); stacked(u) = frames
// max(u - S + 1 + i, 0), i < S.  What a launch reads and what it writes never meet across threads here either:
//   * the frames read from the history are those of episode steps max(tau - N - S + 2, 0) .. tau, in slots
//     (p - tau + u) mod Hd with tau - u <= N + S - 2 < Hd - 1; the one slot written, (p + 1) mod Hd, is that of step
//     tau + 1 - Hd <= tau - N - S + 1;
//   * the step's own frames (next, reset) come from the inputs, which no workgroup writes;
//   * obs_pixel and the table rows are only written, every destination unit by one thread.
// Grid (n, 1 + X).  Workgroup (a, 0) does the low-dimensional step exactly as the kernels above do (as their one
// workgroup), then reads step_frame_next[a] once and stores it wherever it goes: the history and the acting
// observation's last frame (not on done), pixel_next's last frame at a closing step.  Workgroups (a, 1 .. X) split the
// actor's other destination frames in units of U bytes (smx_frame_unit.inc.h).
#include "smx_frame_unit.inc.h"

constexpr int REC_PIXEL_THREADS = 256;

struct RecP {
    int S, Hd, pos, X;
    long long F;                               // C H W bytes per frame
    const unsigned char *fnext, *freset;
    unsigned char *hist, *pix, *pix_next, *obs_pix;
};

// workgroup 0's tail: step_frame_next[a] -> the history slot of step tau + 1 and the acting observation's last frame
// (unless the actor restarts), pixel_next's last frame of `row` at a closing step
template <int U>
__device__ __forceinline__ void store_next_frame(const RecP& P, long a, bool restart, bool closing, size_t row, int tid) {
    const long long F = P.F, SF = (long long)P.S * F, nu = F / U;
    const size_t last = (size_t)(P.S - 1) * F;
    const unsigned char* src = P.fnext + (size_t)a * F;
    unsigned char* d0 = restart ? nullptr : P.hist + ((size_t)a * P.Hd + (size_t)((P.pos + 1) % P.Hd)) * F;
    unsigned char* d1 = closing ? P.pix_next + row * SF + last : nullptr;
    unsigned char* d2 = restart ? nullptr : P.obs_pix + (size_t)a * SF + last;
    if (!d0 && !d1) return;                          // (d2 goes with d0)
    alignas(16) unsigned char b[U];
    for (long long v = tid; v < nu; v += REC_PIXEL_THREADS) {
        load_unit<U>(src + v * U, b);
        if (d0) store_unit<U>(d0 + v * U, b);
        if (d1) store_unit<U>(d1 + v * U, b);
        if (d2) store_unit<U>(d2 + v * U, b);
    }
}

// the copy workgroups (y = 1 .. X): item q < nq is one destination frame
//   restart:  q < 1 + S: step_frame_reset[a] -> the history slot (q = 0), acting observation frame q - 1
//   else:     q < S - 1: acting observation frame q <- history, step tau + 2 - S + q
//   then at a closing step the kernel's npix items -- pixel(i, dst, u): destination and source step of item i -- and
//   S - 1 items: pixel_next frame i of `row` <- step tau + 2 - S + i                              (steps < 0: step 0)
template <int U, typename Pixel>
__device__ __forceinline__ void copy_step_frames(const RecP& P, long a, int tau, bool restart, bool closing, size_t row,
                                                 int npix, int y, int tid, Pixel pixel) {
    const int S = P.S, Hd = P.Hd;
    const long long F = P.F, SF = (long long)S * F, nu = F / U;
    const int nfirst = restart ? 1 + S : S - 1;
    const int nq = nfirst + (closing ? npix + S - 1 : 0);
    unsigned char* hist_a = P.hist + (size_t)a * Hd * F;
    const long long total = (long long)nq * nu, stride = (long long)P.X * REC_PIXEL_THREADS;
    alignas(16) unsigned char b[U];
    for (long long g = (long long)(y - 1) * REC_PIXEL_THREADS + tid; g < total; g += stride) {
        const int q = (int)(g / nu);
        const long long e = (g - (long long)q * nu) * U;
        unsigned char* dst;
        int u = 0;                                   // the source step (unless first: the reset frame)
        const bool first = restart && q < nfirst;
        if (q < nfirst) {
            if (restart) dst = q == 0 ? hist_a + (size_t)((P.pos + 1) % Hd) * F : P.obs_pix + (size_t)a * SF + (size_t)(q - 1) * F;
            else { dst = P.obs_pix + (size_t)a * SF + (size_t)q * F; u = tau + 2 - S + q; }
        } else if (q < nfirst + npix) {
            pixel(q - nfirst, dst, u);
        } else {
            const int i = q - nfirst - npix;
            dst = P.pix_next + row * SF + (size_t)i * F;
            u = tau + 2 - S + i;
        }
        if (first) {
            load_unit<U>(P.freset + (size_t)a * F + e, b);
        } else {
            u = u < 0 ? 0 : u;
            const int hs = (((P.pos - tau + u) % Hd) + Hd) % Hd;
            load_unit<U>(hist_a + (size_t)hs * F + e, b);
        }
        store_unit<U>(dst + e, b);
    }
}

template <int U>
__global__ __launch_bounds__(REC_PIXEL_THREADS) void record_ppo_pixel_window_kernel(RecW G, RecP P) {
    const long a = blockIdx.x;
    const int y = blockIdx.y, tid = threadIdx.x;
    const int tau = G.t[a];
    if (tau < 0) return;
    const int N = G.N, S = P.S;
    const int j = tau + 1 - N;
    const int rank = G.rank[a];
    const bool wclose = rank >= 0 && rank < G.rows && j >= 0 && j % G.adv == 0;      // (ppo_window_step's rule)
    const size_t row = wclose ? (size_t)((G.cursor + rank) % G.capacity) : 0;
    const bool restart = G.done[a] != 0.0f && P.freset;
    if (y == 0) {
        ppo_window_step(G, a, 0, 1, tid);
        store_next_frame<U>(P, a, restart, wclose, row, tid);
        return;
    }
    // the closing window's N S items: pixel frame i of window step w <- step j + w - S + 1 + i
    const long long F = P.F;
    copy_step_frames<U>(P, a, tau, restart, wclose, row, N * S, y, tid, [&](int q, unsigned char*& dst, int& u) {
        const int w = q / S, i = q - w * S;
        dst = P.pix + (row * N + w) * (size_t)S * F + (size_t)i * F;
        u = j + w - S + 1 + i;
    });
}

template <int U>
__global__ __launch_bounds__(REC_PIXEL_THREADS) void record_ddpg_pixel_nstep_kernel(RecD G, RecP P) {
    const long a = blockIdx.x;
    const int y = blockIdx.y, tid = threadIdx.x;
    const int tau = G.t[a];
    if (tau < 0) return;
    const int N = G.N, S = P.S;
    const int rank = G.rank[a];
    const bool emits = rank >= 0 && rank < G.rows && tau >= N - 1;                   // (ddpg_nstep_step's rule)
    const size_t row = emits ? (size_t)((G.cursor + rank) % G.capacity) : 0;
    const bool restart = G.done[a] != 0.0f && P.freset;
    if (y == 0) {
        ddpg_nstep_step<REC_PIXEL_THREADS>(G, a, tid);
        store_next_frame<U>(P, a, restart, emits, row, tid);
        return;
    }
    // the emitted transition j's S items: pixel frame i <- step j - S + 1 + i
    const int j = tau - N + 1;
    const long long F = P.F;
    copy_step_frames<U>(P, a, tau, restart, emits, row, S, y, tid, [&](int i, unsigned char*& dst, int& u) {
        dst = P.pix + row * (size_t)S * F + (size_t)i * F;
        u = j - S + 1 + i;
    });
}

// ---- DDPG with a camera, frame-pool layout (include/surreal_amd.h, above smx_synth_ddpg_pixel_pool_step) ------------------
// Every frame once in a per-actor pool of Pl slots, counter i in slot i mod Pl; a terminal step brings two frames (the
// terminal one, the reset one), so the counters are the actors' own: f = cin[a], first = cin[n + a] before the step,
// cout[...] after it -- two buffers, because the copy workgroups read what workgroup (a, 0) moves on.  Workgroup (a, 0):
// the low-dimensional step, the row's counters at a closing step, step_frame_next[a] -> the pool at f + 1 and (unless the
// actor restarts) the acting observation's last frame.  Workgroups (a, 1 .. X): the observation's older frames out of the
// pool (counters max(f + 2 - S + q, first)), or on a restart step_frame_reset[a] -> the pool at f + 2 and S times into the
// observation.  Read: f + 2 - S .. f; written: f + 1, f + 2 -- S + 1 consecutive counters, distinct slots as Pl >= S + 2.
struct RecPool {
    int S, X;
    long long F, Pl;
    const unsigned char *fnext, *freset;
    unsigned char *pool, *obs_pix;
    const int64_t* cin;
    int64_t *cout, *frame_next, *frame_first;
    int* frame_actor;
};

template <int U>
__global__ __launch_bounds__(REC_PIXEL_THREADS) void record_ddpg_pixel_pool_nstep_kernel(RecD G, RecPool P) {
    const long a = blockIdx.x;
    const int y = blockIdx.y, tid = threadIdx.x;
    const int tau = G.t[a];
    if (tau < 0) return;
    const int N = G.N, S = P.S;
    const int rank = G.rank[a];
    const bool emits = rank >= 0 && rank < G.rows && tau >= N - 1;                   // (ddpg_nstep_step's rule)
    const size_t row = emits ? (size_t)((G.cursor + rank) % G.capacity) : 0;
    const bool restart = G.done[a] != 0.0f && P.freset;
    const long long f = P.cin[a], first = P.cin[G.n + a];
    const long long F = P.F, nu = F / U;
    unsigned char* pool_a = P.pool + (size_t)a * P.Pl * F;
    unsigned char* obs_a = P.obs_pix + (size_t)a * S * F;
    auto slot = [&](long long c) { return pool_a + (size_t)(((c % P.Pl) + P.Pl) % P.Pl) * F; };
    alignas(16) unsigned char b[U];
    if (y == 0) {
        ddpg_nstep_step<REC_PIXEL_THREADS>(G, a, tid);
        if (tid == 0) {
            if (emits) {
                P.frame_next[row] = f + 1;
                P.frame_first[row] = first;
                P.frame_actor[row] = (int)a;
            }
            P.cout[a] = f + (restart ? 2 : 1);
            P.cout[G.n + a] = restart ? f + 2 : first;
        }
        const unsigned char* src = P.fnext + (size_t)a * F;
        unsigned char* d0 = slot(f + 1);
        unsigned char* d1 = restart ? nullptr : obs_a + (size_t)(S - 1) * F;
        for (long long v = tid; v < nu; v += REC_PIXEL_THREADS) {
            load_unit<U>(src + v * U, b);
            store_unit<U>(d0 + v * U, b);
            if (d1) store_unit<U>(d1 + v * U, b);
        }
        return;
    }
    const int nq = restart ? 1 + S : S - 1;
    const long long total = (long long)nq * nu, stride = (long long)P.X * REC_PIXEL_THREADS;
    for (long long g = (long long)(y - 1) * REC_PIXEL_THREADS + tid; g < total; g += stride) {
        const int q = (int)(g / nu);
        const long long e = (g - (long long)q * nu) * U;
        unsigned char* dst;
        if (restart) {
            dst = q == 0 ? slot(f + 2) : obs_a + (size_t)(q - 1) * F;
            load_unit<U>(P.freset + (size_t)a * F + e, b);
        } else {
            dst = obs_a + (size_t)q * F;
            const long long c = f + 2 - S + q;
            load_unit<U>(slot(c < first ? first : c) + e, b);
        }
        store_unit<U>(dst + e, b);
    }
}

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

// ---- what the low-dimensional and the camera entry points of a step share: the checks (the SMX_E_* code, SMX_OK) and
// the kernel's argument block, from either argument struct ----
template <typename Block>
int window_step_check(const Block* a) {
    SMX_REQUIRE(a && step_pointers(*a) && a->step_pds && a->carry_pd && a->pds, SMX_E_NULL);
    SMX_REQUIRE((a->h_before == nullptr) == (a->c_before == nullptr) && episode_pointers_ok(a->mon), SMX_E_NULL);
    // an LSTM policy's cells: the ring whenever a state comes in or a window's cells go out
    SMX_REQUIRE((!a->h_before && !a->cells) || a->carry_cells, SMX_E_NULL);
    SMX_REQUIRE(step_shape_ok(*a) && a->hidden >= 0 && a->advance > 0 && a->advance <= a->n_step, SMX_E_SHAPE);
    SMX_REQUIRE(!a->carry_cells || a->hidden > 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->copy_workgroups >= 0 && a->copy_workgroups <= 1024 && episode_shape_ok(a->mon), SMX_E_SHAPE);
    SMX_REQUIRE(clocks_ok(a->t_host, a->rank_host, a->n, a->rows), SMX_E_SHAPE);
    return SMX_OK;
}

template <typename Block>
bool obs_on16(const Block* a) {
    return a->D % 4 == 0 && on16(a->cur_obs) && on16(a->step_obs_next) && on16(a->step_obs_reset) && on16(a->carry_obs) &&
           on16(a->obs) && on16(a->obs_next);
}

template <typename Block>
RecW window_step_fields(const Block* a) {
    RecW G;
    memset(&G, 0, sizeof(G));
    G.n = a->n; G.D = a->D; G.A = a->A; G.Hl = a->hidden; G.N = a->n_step; G.adv = a->advance;
    G.S = (a->n_step + a->advance - 1) / a->advance;
    G.rows = a->rows;
    G.X = 1;
    G.t = a->t; G.rank = a->rank;
    G.cur = a->cur_obs; G.act = a->step_actions; G.pd = a->step_pds; G.hb = a->h_before; G.cb = a->c_before;
    G.onext = a->step_obs_next; G.rew = a->step_rewards; G.done = a->step_dones; G.oreset = a->step_obs_reset;
    G.cobs = a->carry_obs; G.cact = a->carry_act; G.crew = a->carry_rew; G.cpd = a->carry_pd; G.ccell = a->carry_cells;
    G.obs = a->obs; G.obs_next = a->obs_next; G.actions = a->actions; G.rewards = a->rewards; G.dones = a->dones;
    G.pds = a->pds; G.cells = a->cells;
    G.cursor = a->cursor; G.capacity = a->capacity;
    G.mon = a->mon;
    if (obs_on16(a)) G.vec |= VEC_OBS;
    if (a->A % 4 == 0 && on16(a->step_actions) && on16(a->carry_act) && on16(a->actions)) G.vec |= VEC_ACT;
    if (a->A % 2 == 0 && on16(a->step_pds) && on16(a->carry_pd) && on16(a->pds)) G.vec |= VEC_PD;
    return G;
}

template <typename Block>
int nstep_step_check(const Block* a) {
    SMX_REQUIRE(a && step_pointers(*a) && a->gpow && episode_pointers_ok(a->mon), SMX_E_NULL);
    SMX_REQUIRE(step_shape_ok(*a) && episode_shape_ok(a->mon), SMX_E_SHAPE);
    SMX_REQUIRE(clocks_ok(a->t_host, a->rank_host, a->n, a->rows), SMX_E_SHAPE);
    return SMX_OK;
}

template <typename Block>
RecD nstep_step_fields(const Block* a) {
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
    if (obs_on16(a)) G.vec |= VEC_OBS;
    if (a->A % 4 == 0 && on16(a->step_actions) && on16(a->carry_act) && on16(a->actions)) G.vec |= VEC_ACT;
    return G;
}

// the camera of either camera argument struct: the frame buffers and the input frame, the frame, and a history long
// enough that no launch reads the slot it writes (proof above struct RecP)
template <typename Block>
int camera_check(const Block* a) {
    SMX_REQUIRE(a->hist && a->pixel && a->pixel_next && a->obs_pixel && a->step_frame_next, SMX_E_NULL);
    SMX_REQUIRE(a->C > 0 && a->H > 0 && a->W > 0 && a->frame_stacks > 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->hist_len >= a->n_step + a->frame_stacks && a->hist_pos >= 0 && a->hist_pos < a->hist_len, SMX_E_SHAPE);
    SMX_REQUIRE(a->copy_workgroups >= 0 && a->copy_workgroups <= 1024, SMX_E_SHAPE);
    return SMX_OK;
}

// ... with X copy workgroups per actor: copy_workgroups, or ~32 KB each of the destination frames of the actor that
// moves most -- one that restarts and, with rows > 0, closes: 1 + S frames and `closing` more -- and no more than 16
// workgroups per CU over the launch's closing actors
template <typename Block>
RecP camera_fields(const Block* a, long long closing) {
    RecP P;
    memset(&P, 0, sizeof(P));
    P.S = a->frame_stacks; P.Hd = a->hist_len; P.pos = a->hist_pos;
    P.F = (long long)a->C * a->H * a->W;
    P.fnext = a->step_frame_next; P.freset = a->step_frame_reset;
    P.hist = a->hist; P.pix = a->pixel; P.pix_next = a->pixel_next; P.obs_pix = a->obs_pixel;
    long long X = a->copy_workgroups;
    if (X == 0) {
        const long long frames = 1 + P.S + (a->rows > 0 ? closing : 0);
        X = (frames * P.F + 32767) / 32768;
        if (a->rows > 0) {
            const long long room = 16LL * smx_cu_count() / a->rows;
            if (X > room) X = room;
        }
        if (X > 64) X = 64;
    }
    P.X = X < 1 ? 1 : (int)X;
    return P;
}

// a camera record kernel on the grid (n, 1 + X): K16 moves 16 bytes a lane where the frame size and every frame buffer
// allow it, else K1 single bytes
template <auto K16, auto K1, typename Args>
int launch_camera(const Args& G, const RecP& P, int n, smx_stream_t stream) {
    const bool vec = P.F % 16 == 0 && on16(P.fnext) && on16(P.freset) && on16(P.hist) && on16(P.pix) && on16(P.pix_next) &&
                     on16(P.obs_pix);
    hipLaunchKernelGGL(vec ? K16 : K1, dim3(n, 1 + P.X), dim3(REC_PIXEL_THREADS), 0, smx_s(stream), G, P);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

}  // namespace

extern "C" int smx_record_ppo_window_step_f32(const struct smx_record_ppo_window_step* a, smx_stream_t stream) {
    const int rc = window_step_check(a);
    if (rc != SMX_OK) return rc;
    RecW G = window_step_fields(a);
    G.X = a->copy_workgroups ? a->copy_workgroups : window_copy_workgroups(*a);
    hipLaunchKernelGGL(record_ppo_window_kernel, dim3(a->n, G.X), dim3(REC_THREADS), 0, smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_record_ddpg_nstep_step_f32(const struct smx_record_ddpg_nstep_step* a, smx_stream_t stream) {
    const int rc = nstep_step_check(a);
    if (rc != SMX_OK) return rc;
    const RecD G = nstep_step_fields(a);
    hipLaunchKernelGGL(record_ddpg_nstep_kernel, dim3(a->n), dim3(REC_DDPG_THREADS), 0, smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_record_ppo_pixel_window_step(const struct smx_record_ppo_pixel_window_step* a, smx_stream_t stream) {
    int rc = window_step_check(a);
    if (rc == SMX_OK) rc = camera_check(a);
    if (rc != SMX_OK) return rc;
    const RecW G = window_step_fields(a);
    // a closing step: the window's N S stacked frames and pixel_next's S - 1 older ones
    const RecP P = camera_fields(a, (long long)(a->n_step + 1) * a->frame_stacks - 1);
    return launch_camera<record_ppo_pixel_window_kernel<16>, record_ppo_pixel_window_kernel<1>>(G, P, a->n, stream);
}

extern "C" int smx_record_ddpg_pixel_pool_nstep_step(const struct smx_record_ddpg_pixel_pool_nstep_step* a,
                                                     smx_stream_t stream) {
    const int rc = nstep_step_check(a);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(a->pool && a->obs_pixel && a->step_frame_next && a->counters_in && a->counters_out && a->frame_next &&
                a->frame_first && a->frame_actor, SMX_E_NULL);
    SMX_REQUIRE(a->C > 0 && a->H > 0 && a->W > 0 && a->frame_stacks > 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->pool_len >= (int64_t)a->n_step + a->frame_stacks + 1 && a->counters_in != a->counters_out, SMX_E_SHAPE);
    SMX_REQUIRE(a->copy_workgroups >= 0 && a->copy_workgroups <= 1024, SMX_E_SHAPE);
    SMX_REQUIRE((((uintptr_t)a->counters_in | (uintptr_t)a->counters_out | (uintptr_t)a->frame_next |
                  (uintptr_t)a->frame_first) & 7) == 0 && ((uintptr_t)a->frame_actor & 3) == 0, SMX_E_ALIGN);
    const RecD G = nstep_step_fields(a);
    RecPool P;
    memset(&P, 0, sizeof(P));
    P.S = a->frame_stacks; P.F = (long long)a->C * a->H * a->W; P.Pl = a->pool_len;
    P.fnext = a->step_frame_next; P.freset = a->step_frame_reset; P.pool = a->pool; P.obs_pix = a->obs_pixel;
    P.cin = a->counters_in; P.cout = a->counters_out;
    P.frame_next = a->frame_next; P.frame_first = a->frame_first; P.frame_actor = a->frame_actor;
    // (the copy workgroups: ~32 KB each of the 1 + S frames of an actor that restarts)
    long long X = a->copy_workgroups ? a->copy_workgroups : ((1LL + P.S) * P.F + 32767) / 32768;
    P.X = (int)(X < 1 ? 1 : (X > 64 && !a->copy_workgroups ? 64 : X));
    const bool vec = P.F % 16 == 0 && on16(P.fnext) && on16(P.freset) && on16(P.pool) && on16(P.obs_pix);
    hipLaunchKernelGGL(vec ? record_ddpg_pixel_pool_nstep_kernel<16> : record_ddpg_pixel_pool_nstep_kernel<1>,
                       dim3(a->n, 1 + P.X), dim3(REC_PIXEL_THREADS), 0, smx_s(stream), G, P);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_record_ddpg_pixel_nstep_step(const struct smx_record_ddpg_pixel_nstep_step* a, smx_stream_t stream) {
    int rc = nstep_step_check(a);
    if (rc == SMX_OK) rc = camera_check(a);
    if (rc != SMX_OK) return rc;
    const RecD G = nstep_step_fields(a);
    const RecP P = camera_fields(a, 2LL * a->frame_stacks - 1);
    return launch_camera<record_ddpg_pixel_nstep_kernel<16>, record_ddpg_pixel_nstep_kernel<1>>(G, P, a->n, stream);
}

