// Device-resident rollouts in ONE launch, for PPO and for DDPG.  Actors are independent of each other, time steps are
// not: so a workgroup OWNS 4, 8 or 16 actors and walks them through all steps by itself -- no per-step launch, no
// grid-wide synchronisation.  The environment's state of its actors stays in registers for the whole rollout.  Per step:
//   x tile (the observations of its actors, LDS)  ->  the three actor layers on FP32 MFMA with the fragment-order packed
//   weights streamed from L2  ->  the head (per kernel)  ->  the synthetic environment's step for the block's actors  ->
//   the recording (per kernel)  ->  the next observation straight into the x tile.
//
//   smx_synth_rollout_f32       PPO (surreal/agent/base.py:244-271 the per-step loop of a rollout worker,
//                               surreal/agent/ppo_agent.py:106-154 act: z-filter -> policy MLP -> DiagGauss sample ->
//                               clip; the recording of surreal/env/exp_sender_wrapper.py:153-264 into rollout tables
//                               [actors, T + 1, .]).  4 and 8 actors per workgroup run rollout_kernel<RG> on the 4-row
//                               v_mfma_f32_4x4x1 loop of smx_rows4_mma.inc.h, 16 run rollout16_kernel on the 16x16x4 loop
//                               of smx_epoch_mma.inc.h.
//   smx_synth_lstm_rollout_f32  PPO with the one-layer LSTM stem in front of the policy MLP (ppo_net.py:317-354, the
//                               reference's default policy): lstm_rollout_kernel<RG>, the PPO kernel body with the gate
//                               and cell passes first in every step, on the 4-row loop at every block size.
//   smx_synth_ddpg_rollout_f32  DDPG (surreal/agent/ddpg_agent.py:155-184 act: actor -> clip -> + exploration noise ->
//                               clip; surreal/agent/action_noise.py; the n-step transitions of
//                               surreal/env/exp_sender_wrapper.py:72-112 ExpSenderWrapperSSARNStepBootstrap, which run on
//                               the host there) recorded straight into the uniform replay's ring: ddpg_rollout_kernel on
//                               the 4-row loop at every block size.
//                               With a struct smx_ddpg_actor_variant the same launch runs over a population of
//                               perturbed actors (packed_pop; parameter-space noise, smx_param_noise.hip):
//                               ddpg_rollout_kernel<RG, NT, true>, each workgroup's layers run from the copy of the agent
//                               its actors belong to, and one step of the call can measure the agents' action distance
//                               against the clean actor; and for an actor with a LayerNorm behind each hidden ReLU (ln):
//                               ddpg_rollout_kernel<RG, NT, POP, true>, ln_rows over the hidden tiles.
//   smx_synth_ddpg_step_f32     one DDPG step for all actors given the actor's output mu [n, A] from any forward
//                               (LayerNorm actors, unsupported shapes; with smx_epoch_forward_f32 the persistent kernel's
//                               two-launch reference).
//   smx_synth_ddpg_pixel_step   the same step for actors with a camera, plus the frames: the new frame rendered into a
//                               per-actor history, the closing transitions' stacked uint8 pixel / pixel_next into the ring,
//                               the next acting observation (ddpg_pixel_step_kernel; the CNN perception runs between steps).
//   smx_synth_ppo_pixel_window_step  one PPO step for actors with a camera given the policy mean: head, step, the moving
//                               windows' carry rings and frame history, the closing windows' fields and stacked uint8
//                               pixel / pixel_next into the FIFO's ring (ppo_pixel_window_step_kernel).
//
//   smx_synth_ppo_window_rollout_clocks_f32 / smx_synth_ddpg_rollout_clocks_f32  the windowed PPO and the DDPG launch with
//                               an episode clock PER ACTOR (struct smx_actor_clocks; the row table of smx_actor_clock.hip):
//                               the CLK instantiations of the same kernels (ClkArgs).
//
//   smx_synth_ppo_window_rollout_resets_f32 / smx_synth_ddpg_rollout_resets_f32  the same two with the episodes' first rows
//                               drawn in the launch (struct smx_reset_stream; reach_reset_value of smx_philox.inc.h).
//
//   smx_synth_ppo_window_rollout_task_f32 / smx_synth_ddpg_rollout_task_f32  the windowed PPO launch (plain MLP or LSTM stem)
//                               and the plain DDPG launch on another task's dynamics (SMX_TASK_REACH: EnvLanes::step_reach;
//                               ppo_window_task_kernel, lstm_window_task_kernel, ddpg_rollout_kernel<..., TASK>).
//
//   smx_synth_ddpg_rollout_variant_task_f32  the DDPG launch of any of the four actors (struct smx_ddpg_actor_variant) on a
//                               task, with or without the reset stream: ddpg_rollout_kernel<RG, NT, POP, LN, false, TASK>.
//
//   smx_synth_ppo_eval_f32 / smx_synth_ddpg_eval_f32  evaluation: whole episodes of the policy as independent (actor, episode)
//                               rows of one launch, nothing recorded, the fp64 returns stored once (ppo_eval_kernel,
//                               ddpg_eval_kernel: new kernels that share the pieces above, not the bodies).
//
//   smx_synth_ppo_eval_sets_f32 / smx_synth_ddpg_eval_sets_f32  the same for several parameter SNAPSHOTS on the same episodes
//                               in one launch (the SETS instantiations of the two evaluation kernels on a grid (blocks, sets):
//                               the same bodies, the set's shift applied once at entry); smx_eval_snapshot_floats /
//                               smx_eval_snapshot_store_f32: a snapshot's layout and its store (at the end of the file).
//
// Layout: the persistent kernels (PPO, then DDPG, then the evaluation), the step kernels (the two camera ones share their frame half:
// frame_ctx / render_next_frame / copy_frames), then the host side: carve() and launch(), the argument fills (net_fields,
// roll_fields, table_fields, lstm_fields, win_fields, pixel_fields), the rules the entry points share (*_ok, *_pointers),
// the entry points.
//
// The per-step launches the PPO rollout replaces were 3 dependent launches of ~9.5 us each (two hidden layers as GEMM
// launches, then head + step), 384 launches for T = 128.
//
// DDPG's open transitions of an actor (observation, action, reward of its last n_step steps) live in a ring of n_step
// slots in HBM, slot tau % n_step for episode step tau: every value is written and later read by the SAME lane, so no
// barrier orders them, and they carry from one call to the next.  Transition j = tau - n_step + 1 closes at step tau;
// the k-th closing step of a call writes actor a to ring row (cursor + k n + a) mod capacity.
//
// Episode monitor (struct smx_episode_monitor; mon.ep_reward null: none): the lane that forms an actor's reward also keeps
// its open episode's fp64 reward sum and length (episode_step, smx_synth_env.inc.h) -- in LDS behind the layout in the
// persistent kernels (HBM at entry, at a closing step, at exit), in HBM in the step kernels.
//
// Exploration noise (struct smx_noise_stream): a sampling head takes its lane's draw from eps when there is one, else --
// noise.enabled -- forms it itself where it requested the eps word before (noise_pick, smx_philox.inc.h: ten Philox
// rounds and one Box-Muller element per (actor, component) lane and step), else samples nothing.
#include "smx_common.h"
#include <string.h>
#include <type_traits>

namespace {
#include "smx_epoch_pack.inc.h"
#include "smx_epoch_mma.inc.h"
#include "smx_rows4_mma.inc.h"
#include "smx_synth_env.inc.h"
#include "smx_philox.inc.h"
#include "smx_lstm_act.inc.h"

// Phase timestamps exist only in a build with -DSMX_ROLLOUT_TIMING (scripts/bench_rollout.py); the product build has none.
#ifdef SMX_ROLLOUT_TIMING
#define RSTAMP(i) do { if (g_rtbuf_dev && threadIdx.x == 0 && step == G.steps / 2) g_rtbuf_dev[(size_t)blockIdx.x * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#define RWALL(i) do { if (g_rtbuf_dev && threadIdx.x == 0) g_rtbuf_dev[(size_t)blockIdx.x * 16 + (i)] = (long long)wall_clock64(); } while (0)
#define RCYC(i) do { if (g_rtbuf_dev && threadIdx.x == 0) g_rtbuf_dev[(size_t)blockIdx.x * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
__device__ long long* g_rtbuf_dev = nullptr;
#else
#define RSTAMP(i) do { } while (0)
#define RWALL(i) do { } while (0)
#define RCYC(i) do { } while (0)
#endif

constexpr int RLDO = 36;          // row stride of the output tile in LDS (<= 32 actions)
constexpr int RMAX_A = 32;
constexpr int RNWV = 8;           // two wavefronts per SIMD: the K loops have no barrier inside, so one wave's loads
constexpr int RNTH = 64 * RNWV;   // and epilogue hide under the other's MFMAs
constexpr int RKV = 8;            // observation elements a lane owns per row (D <= 64 RKV)
constexpr int ROLL_MAX_LDS = 150 * 1024;
constexpr int ROLL_EXCLUSIVE_LDS = 84 * 1024;   // one workgroup per CU: each streams the packed weights by itself

// What every persistent kernel takes: the actor, the actors' states and the LDS layout (carve()).
struct RollBase {
    const float *P1, *P2, *P3;                  // packed weights (smx_epoch_pack_f32)
    const float *b1, *b2, *b3;
    int D, H1, H2, A, n, steps, t0, episode_len;
    const float* eps;                           // this step's normal draws [steps, n, A] or null
    smx_noise_stream nstream;                   // eps null and nstream.enabled: the draws are formed here (noise_draw)
    float* state;                               // [n, D] in / out
    const float* init_state;
    int ldx, ldh1, ldh2, off_h1, off_h2, off_out, off_act, off_red3, off_z, off_kmod;
    smx_episode_monitor mon;                    // mon.ep_reward null: none
    int off_ep;                                 // the open episodes of the block's actors in LDS (carve_episodes())
};

struct RollArgs : RollBase {
    int out_act;
    const float *log_var, *noise_scale;
    const float *zsum, *zsumsq, *zcount;        // z-filter running sums or null
    float zeps;
    int R, slot0;                               // R = rows per actor in the rollout tables
    float *obs_roll, *act_roll, *rew_roll, *done_roll, *pd_roll, *obs_last;
};

// the LSTM stem in front of the PPO actor (lstm_rollout_kernel)
struct LArgs : RollArgs {
    const float *Pg, *bg;                       // the gate pass: [W_ih | 0 | W_hh] packed over K = Dp + H, b_ih + b_hh
    int H, Hl, Dp, off_g, ldg, off_c;           // H: units (padded to 4), Hl: logical units; Dp = D rounded up to 4
    const float *h0, *c0;                       // [n, Hl] or null (zeros)
    float *hN, *cN, *h_before, *c_before;       // [n, Hl]: after the last step, before it (h_before / c_before nullable)
    float* cell_roll;                           // [n, R, 2, Hl] the state before every step, or null
};

// the windowed PPO rollouts (ppo_window_kernel, lstm_window_kernel): the carry rings of the open windows and the FIFO's
// tables the closing windows go to
struct WinArgs {
    int N, adv, S;                              // n_step, window advance min(stride, n_step), cell slots ceil(N / adv)
    float *cobs, *cact, *crew, *cpd;            // [n, N, D | A | 1 | 2A]: step tau in slot tau % N
    float* ccell;                               // [n, S, 2, Hl]: the state before window start tau in slot (tau / adv) % S
    float *obs, *obs_next, *act, *rew, *done, *pd, *cells;   // [capacity, N D | D | N A | N | N | N 2A | 2 Hl]
    long long cursor, capacity;
};
struct RollArgsW : RollArgs { WinArgs W; };
struct LArgsW : LArgs { WinArgs W; };

struct DArgs : RollBase {
    int N, noise;
    const double* sigmas;
    double theta, dt, root_dt;
    const double* gpow;
    double* ou;
    float *cobs, *cact, *crew;
    float *obs, *obs_next, *act, *rew, *done;
    long long cursor, capacity;
};

// the population rollout (ddpg_rollout_kernel<RG, NT, true>): every agent -- apa consecutive actors -- has its own copy
struct PopArgs : DArgs {
    RollBase popnet;                            // what layers4 reads, the weights and biases those of AGENT 0's copy
    long long stride;                           // floats from one agent's copy to the next (pop_copy_floats at least)
    int apa, measure_step;                      // actors per agent; the step that measures the action distance or -1
    double* dist;                               // [agents]
};

// a LayerNorm behind each hidden ReLU (ddpg_rollout_kernel<RG, NT, POP, true>): g = ln1.W [H1] | ln1.b [H1] | ln2.W [H2]
// | ln2.b [H2] of the clean actor; pop: the same block of AGENT 0's copy (the population rollout)
struct LnTail {
    const float *g, *pop;
    float eps;
    int off;                                    // the block the workgroup's layers use, in LDS (carve_ln())
};
struct DLnArgs : DArgs { LnTail ln; };
struct PopLnArgs : PopArgs { LnTail ln; };
template <bool POP, bool LN>
using DdpgArgs = std::conditional_t<LN, std::conditional_t<POP, PopLnArgs, DLnArgs>, std::conditional_t<POP, PopArgs, DArgs>>;

// Episode clocks per actor (struct smx_actor_clocks; the CLK instantiations of the windowed PPO kernels and of the DDPG
// kernel, which take one of these behind their arguments).  The block's clocks live in LDS, three ints per actor row at
// `off` (carve_clocks()): the actor's clock, its episode length, and this step's row_off word, which the row's head
// lane requested before the layers.  Every reader sits behind a barrier of the step; one lane per actor advances the
// clock behind the step's last barrier.  They are stored nowhere at exit: the host knows them.
struct ClkArgs {
    const int32_t *t, *L, *row_off;
    long long rows;
    int off;
};
struct NoClk {};
// a CLK kernel's arguments: those of its shared-clock twin, then the clocks
template <typename Base>
struct WithClk : Base { ClkArgs clk; };
template <typename Base>
__device__ __forceinline__ ClkArgs clk_of(const WithClk<Base>& G) { return G.clk; }
__device__ __forceinline__ NoClk clk_of(const RollBase&) { return NoClk{}; }

// a task kernel's arguments: those of its SMX_TASK_DRIFT twin, then the reset stream (struct smx_reset_stream; rst.enabled
// 0: the actors restart from init_state).  What EnvLanes keeps of it (ResetLanes): where the stream lies in the argument
// segment and the call's episode ends so far -- on the shared clock a wave-uniform count -- for SMX_TASK_REACH / _ARM, nothing for
// a task without a reset distribution.  (Held by value, the stream's seven scalars stayed live across the layers of every
// step: 17 to 48 more SGPR spills a kernel, 2 to 3 more VGPRs, and 0.2 % on a DDPG call that draws nothing.)
template <typename Base>
struct WithRst : Base { smx_reset_stream rst; };
template <int TASK>
struct ResetLanes {};
template <>
struct ResetLanes<SMX_TASK_REACH> {
    const smx_reset_stream* rst;                // in the kernel's argument segment (rst_arg): read at an episode end, and
    int ends;                                   // by a disturbed step for the draw's counter and key words
    int tstep;                                  // the step within the episode under way (the disturbance's counter word)
    int evalE;                                  // an evaluation launch's episodes per actor (row = a E + i), else 0
    float dsc;                                  // the stream's scale, read once (one scalar; 0: the steps are undisturbed)
    __device__ __forceinline__ float scale() const { return dsc; }
    // w[j] of row a's step: a recording launch's row is local actor a in episode rst.episode - 1 + ends, an evaluation's
    // row a = a' E + i is actor a' in episode rst.episode + i (rows < 2^31: an int division, only where the scale is on)
    __device__ __forceinline__ float draw(long a, int j) const {
        uint32_t g = (uint32_t)rst->actor_base, e = (uint32_t)rst->episode;
        if (evalE) {
            const int q = (int)a / evalE;
            g += (uint32_t)q;
            e += (uint32_t)((int)a - q * evalE);
        } else {
            g += (uint32_t)a;
            e += (uint32_t)(ends - 1);
        }
        return disturbance_uniform(rst->seed, g, e, (uint32_t)tstep, j);
    }
    // the clock behind a step
    __device__ __forceinline__ void tick(bool done) {
        tstep = done ? 0 : tstep + 1;
        if (done) ++ends;
    }
    __device__ __forceinline__ void begin(const smx_reset_stream* S, int t0, int E = 0) {
        rst = S; ends = 0; tstep = t0; evalE = E;
        dsc = reset_disturbance(*S);
    }
};
template <>
struct ResetLanes<SMX_TASK_ARM> : ResetLanes<SMX_TASK_REACH> {};
// where a task kernel's arguments KArgs = WithRst<...> hold the stream (scalar loads; no registers held between episode ends)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"       // (WithRst derives from its Base: not standard-layout, one layout here)
template <typename KArgs>
__device__ __forceinline__ const smx_reset_stream* rst_arg() {
    return (const smx_reset_stream*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(KArgs, rst));
}
#pragma clang diagnostic pop

// the ring row of a closing record from its row_off word, which the caller found in [0, rows) (rows <= capacity: one
// wrap at most)
__device__ __forceinline__ long long clk_row(long long cursor, long long capacity, int off) {
    const long long r = cursor + off;
    return r >= capacity ? r - capacity : r;
}

// actor row r's clock and episode length into the block's LDS words.  The ring slots are tau % N: a clock outside
// [0, L) or a length < 1 (the host checks both where it makes the table) is taken as clock 0 / length 1, so that no
// slot index is ever negative
__device__ __forceinline__ void clk_load(const ClkArgs& C, int* clk, int r, long row0) {
    int t = C.t[row0 + r], L = C.L[row0 + r];
    if (L < 1) L = 1;
    if (t < 0 || t >= L) t = 0;
    clk[3 * r] = t;
    clk[3 * r + 1] = L;
    clk[3 * r + 2] = -1;
}

// ---- once per launch: clear the tiles (their padding columns and rows must read as zeros, the action tile's unused
// columns too); k % A (an integer division per element and step otherwise) and, with the z-filter's running sums, its
// mean | std go to the LDS tables at off_kmod and off_z
__device__ __forceinline__ void clear_tiles(const RollBase& G, float* sm, int tid, const float* zsum, const float* zsumsq,
                                            const float* zcount, float zeps) {
    for (int i = tid; i < G.off_z; i += RNTH) sm[i] = 0.f;
    float* zm = sm + G.off_z;
    int* kmod = (int*)(sm + G.off_kmod);
    for (int k = tid; k < G.D; k += RNTH) {
        kmod[k] = k % G.A;
        if (zsum) zfilter_stats(zsum, zsumsq, zcount, zeps, k, zm[k], zm[G.D + k]);
    }
}

// The environment phase of an RB-actor block.  Wave wv steps the actor rows erow0 .. erow0 + RPW - 1 (RB >= 8) or the
// part `part` of row erow0 (RB = 4: WPR waves share a row); a lane owns the elements k = lane + 64 (part + WPR i) of
// them and keeps their raw state in registers for the whole rollout (RB = 16: two rows a wave, k = lane + 64 i).
// COLS: the elements' action column and drift in registers too (else read from kmod and formed every step, where the
// registers are short).
// TASK: the dynamics (SMX_TASK_*; step(), step_reach() and step_arm()).
struct OwnStart {};
template <int RB, bool COLS = true, int TASK = SMX_TASK_DRIFT>
struct EnvLanes : ResetLanes<TASK> {
    static constexpr int TASK_ID = TASK;
    static constexpr int WPR = RB < RNWV ? RNWV / RB : 1;   // wavefronts per actor row
    static constexpr int RPW = RB > RNWV ? RB / RNWV : 1;   // actor rows per wavefront
    static constexpr int KPL = RKV / WPR;                   // observation elements a lane owns per row
    const int D, ldx;                           // (copies, not a reference to the kernel's arguments: fewer registers)
    float* const state;
    const float* const init_state;
    float* xs;                                  // the x tile
    const float* zm;                            // the z-filter's [D] mean | [D] std in LDS, or null: raw observations
    const int* kmod;
    const smx_episode_monitor mon;              // (touched at entry, at closing steps and at exit only)
    double* ep_reward;                          // [RB] the open episodes' sums, then [RB] int their steps, in LDS: each
    int* ep_steps;                              // pair is read and written by the lane that forms its actor's reward
    long row0;
    int nrows, lane, erow0, part;
    float st[RPW][KPL];
    int am[KPL];                                // the elements' action column k % A (COLS)
    float dr[KPL];                              // their drift (COLS)

    // the states of the block's actors to registers
    __device__ __forceinline__ EnvLanes(const RollBase& G, float* sm, const float* zm_, int wv, int lane_)
        : D(G.D), ldx(G.ldx), state(G.state), init_state(G.init_state), xs(sm), zm(zm_), kmod((const int*)(sm + G.off_kmod)),
          mon(G.mon), ep_reward((double*)(sm + G.off_ep)), ep_steps((int*)(sm + G.off_ep + 2 * RB)),
          row0((long)blockIdx.x * RB), lane(lane_), erow0(RPW * (wv / WPR)), part(wv % WPR) {
        nrows = G.n - (int)row0;
        if (nrows > RB) nrows = RB;
        if (mon.ep_reward && owner()) {
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int r = erow0 + rr;
                if (r < nrows) {
                    ep_reward[r] = mon.ep_reward[row0 + r];
                    ep_steps[r] = mon.ep_steps[row0 + r];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int k = kel(i);
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int r = erow0 + rr;
                st[rr][i] = (k < D && r < nrows) ? state[(row0 + r) * D + k] : 0.f;
            }
        }
    }
    // the evaluation launches (OwnStart): the block's rows begin where the caller puts them (eval_start) -- `state` is
    // neither read nor written, there is no monitor; rows: the rows of the launch
    __device__ __forceinline__ EnvLanes(const RollBase& G, float* sm, const float* zm_, int wv, int lane_, OwnStart)
        : D(G.D), ldx(G.ldx), state(nullptr), init_state(G.init_state), xs(sm), zm(zm_), kmod((const int*)(sm + G.off_kmod)),
          mon(smx_episode_monitor{}), ep_reward(nullptr), ep_steps(nullptr),
          row0((long)blockIdx.x * RB), lane(lane_), erow0(RPW * (wv / WPR)), part(wv % WPR) {
        nrows = G.n - (int)row0;
        if (nrows > RB) nrows = RB;
#pragma unroll
        for (int i = 0; i < KPL; ++i)
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) st[rr][i] = 0.f;
    }
    __device__ __forceinline__ int kel(int i) const { return lane + 64 * (part + WPR * i); }
    // the lane that forms the rewards of the wave's actor rows (k == 0 lives in lane 0, i == 0 of a row's first wave)
    __device__ __forceinline__ bool owner() const { return lane == 0 && part == 0; }
    __device__ __forceinline__ void put_x(int r, int k, float v) {
        xs[r * ldx + k] = zm ? zclamp(v, zm[k], zm[D + k]) : v;
    }
    // behind the barrier that ends clear_tiles: the first x tile and the per-element constants
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int k = kel(i);
                if (k < D && r < nrows) put_x(r, k, st[rr][i]);
            }
        }
        if (COLS) {
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int k = kel(i);
                am[i] = k < D ? kmod[k] : 0;
                dr[i] = synth_drift(k);
            }
        }
    }
    // One environment step of the block's actors from the clipped actions in s_act [RB][RMAX_A] (unused columns 0),
    // the next state (the reset state when `done`) into the registers and the x tile.  The recording is the caller's:
    // p = open(a) once per actor row, rec(a, p, k, s, sn) per element (state s, next state sn), close(a, p, reward).
    // ROWDONE (per-actor episode clocks): the row's own p.done in place of `done`.
    template <bool ROWDONE = false, typename Open, typename Rec, typename Close>
    __device__ __forceinline__ void step(const float* s_act, bool done, Open open, Rec rec, Close close) {
        if constexpr (TASK == SMX_TASK_REACH) {
            step_reach<ROWDONE>(s_act, done, open, rec, close);
            return;
        }
        if constexpr (TASK == SMX_TASK_ARM) {
            step_arm<ROWDONE>(s_act, done, open, rec, close);
            return;
        }
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;                   // wave-uniform
            if (r < nrows) {
                const long a = row0 + r;
                const auto p = open(a);
                if constexpr (ROWDONE) done = p.done;
                float sn0 = 0.f;
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    const int k = kel(i);
                    if (k < D) {
                        const float s = st[rr][i];
                        const float sn = COLS ? synth_next(s, s_act[r * RMAX_A + am[i]], dr[i])
                                              : synth_next(s, s_act[r * RMAX_A + kmod[k]], synth_drift(k));
                        rec(a, p, k, s, sn);
                        if (i == 0) sn0 = sn;
                        const float next = done ? init_state[a * D + k] : sn;
                        st[rr][i] = next;
                        put_x(r, k, next);
                    }
                }
                if (owner()) {
                    // sum_j a_j^2 in fp64, j ascending (the order of smx_synth_env_step_f32).  All RMAX_A reads are
                    // issued up front (unused columns of the tile are zero and add +0.0): one LDS round trip, not A
                    float av[RMAX_A];
#pragma unroll
                    for (int j = 0; j < RMAX_A; ++j) av[j] = s_act[r * RMAX_A + j];
                    double q = 0.0;
#pragma unroll
                    for (int j = 0; j < RMAX_A; ++j) q += (double)av[j] * (double)av[j];
                    const float rew = synth_reward(q, sn0);
                    close(a, p, rew);
                    if (mon.ep_reward) episode_step(mon, a, ep_reward[r], ep_steps[r], rew, done);
                }
            }
        }
    }
    // The same step of SMX_TASK_REACH (reach_* of smx_synth_env.inc.h; D = 3 A <= 63, checked by the entry points).  A
    // row's elements are coupled, and all of them sit in the 64 lanes of the row's first wave (kel(0), part == 0) at
    // every block size: lane j < A holds p[j], lane A + j holds v[j], lane 2 A + j holds g[j].  So wave shuffles carry
    // what an element needs from another -- v'[j] and g[j] to lane j -- and the d[j] and a[j] to the fp64 sums, j
    // ascending (every lane of the wave forms them, the owner uses them): no LDS, no barrier.  The shuffles run in
    // wave-uniform control flow; a source lane past the row (k >= D) is read by lanes whose value is not used.
    // The reset row at an episode end: with a stream (rst.enabled, uniform over the kernel) every live lane draws its
    // element of episode rst.episode + ends itself (reach_reset_value: ten Philox rounds, no memory read), else it loads
    // init_state's.
    // The per-step disturbance (a stream with a scale != 0; ResetLanes::dsc, uniform over the launch): lane A + j, which
    // forms v'[j], draws s * w[j] of step tstep of the episode under way (ResetLanes::draw: ten more rounds, no memory
    // read) ahead of the step's dependent chain; with dsc == 0 nothing is drawn and nothing is added.  tick(done) behind
    // the step moves the clock of the draws on: tstep + 1, or 0 and one more episode end (what `++ends` did alone).
    template <bool ROWDONE, typename Open, typename Rec, typename Close>
    __device__ __forceinline__ void step_reach(const float* s_act, bool done, Open open, Rec rec, Close close) {
        if (part != 0) return;                          // (wave-uniform: these waves own k >= 64 > D)
        const int k = lane;                             // kel(0)
        const int J = D / 3;
        const int kind = k >= 2 * J ? 2 : (k >= J ? 1 : 0);
        const int j = k - kind * J;
        const bool live = k < D;
        const float dsc = this->scale();                // (wave-uniform) the disturbance's scale, 0: none
        // lane A + j: s * w[j] of the wave's rows (ten Philox rounds, no memory), drawn ahead of the step's dependent chain
        // so that an undisturbed step keeps that chain in one piece
        float sw[RPW];
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) sw[rr] = 0.f;
        if (dsc != 0.0f) {
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) sw[rr] = dsc * this->draw(row0 + erow0 + rr, j);
        }
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;                   // wave-uniform
            if (r < nrows) {
                const long a = row0 + r;
                const auto p = open(a);
                if constexpr (ROWDONE) done = p.done;
                const float s = st[rr][0];
                const float ac = live ? s_act[r * RMAX_A + j] : 0.f;
                const float vc = reach_next_v(s, ac, dsc != 0.0f, sw[rr]);  // lane A + j: v'[j]
                const float vn = __shfl(vc, k + J);                 // lane j: v'[j]
                const float pc = reach_next_p(s, vn);               // lane j: p'[j]
                const float gj = __shfl(s, k + 2 * J);              // lane j: g[j]
                const float d = kind == 0 ? pc - gj : 0.f;
                const float sn = kind == 0 ? pc : (kind == 1 ? vc : s);
                if (live) {
                    rec(a, p, k, s, sn);
                    float next = sn;
                    if (done)
                        next = this->rst->enabled ? reach_reset_value(*this->rst, a, this->ends, k, J) : init_state[a * D + k];
                    st[rr][0] = next;
                    put_x(r, k, next);
                }
                double sd = 0.0, sa = 0.0;
                for (int jj = 0; jj < J; ++jj) {
                    const double dj = (double)__shfl(d, jj);
                    sd += dj * dj;
                }
                for (int jj = 0; jj < J; ++jj) {
                    const double aj = (double)__shfl(ac, jj);
                    sa += aj * aj;
                }
                if (owner()) {
                    const float rew = reach_reward(sd, sa);
                    close(a, p, rew);
                    if (mon.ep_reward) episode_step(mon, a, ep_reward[r], ep_steps[r], rew, done);
                }
            }
        }
        this->tick(done);                               // (ROWDONE: never with a task)
    }
    // The same step of SMX_TASK_ARM (arm_* of smx_synth_env.inc.h; D = 2 A + 2 <= 62, checked by the entry points), laid
    // out as step_reach's: lane j < A holds theta[j], lane A + j holds omega[j], lanes 2 A and 2 A + 1 hold the goal.  One
    // shuffle carries omega'[j] to lane j, which forms theta'[j] and its sine and cosine; every lane of the wave forms the
    // three fp64 sums -- cosines, sines, squared actions -- over jj ascending and reads the goal by two more shuffles, the
    // owner uses them: no LDS, no barrier, the shuffles in wave-uniform control flow.  The reset row as in step_reach
    // (arm_reset_value).
    template <bool ROWDONE, typename Open, typename Rec, typename Close>
    __device__ __forceinline__ void step_arm(const float* s_act, bool done, Open open, Rec rec, Close close) {
        if (part != 0) return;                          // (wave-uniform: these waves own k >= 64 > D)
        const int k = lane;                             // kel(0)
        const int J = (D - 2) / 2;
        const int kind = k >= 2 * J ? 2 : (k >= J ? 1 : 0);
        const int j = k - kind * J;                     // (a goal lane: 0 or 1 -- a column of the tile, its action unused)
        const bool live = k < D;
        const double w = arm_link(J);
        const float dsc = this->scale();                // (wave-uniform) the disturbance's scale, 0: none
        float sw[RPW];                                  // lane A + j: s * w[j] of the wave's rows, as in step_reach
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) sw[rr] = 0.f;
        if (dsc != 0.0f) {
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) sw[rr] = dsc * this->draw(row0 + erow0 + rr, j);
        }
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;                   // wave-uniform
            if (r < nrows) {
                const long a = row0 + r;
                const auto p = open(a);
                if constexpr (ROWDONE) done = p.done;
                const float s = st[rr][0];
                const float ac = live ? s_act[r * RMAX_A + j] : 0.f;
                const float oc = arm_next_omega(s, ac, dsc != 0.0f, sw[rr]);    // lane A + j: omega'[j]
                const float on = __shfl(oc, k + J);                 // lane j: omega'[j]
                const float tc = arm_next_theta(s, on);             // lane j: theta'[j]
                float sj, cj;
                arm_sincos(tc, sj, cj);                             // lane j: its sine and cosine
                const float g0 = __shfl(s, 2 * J), g1 = __shfl(s, 2 * J + 1);
                const float sn = kind == 0 ? tc : (kind == 1 ? oc : s);
                if (live) {
                    rec(a, p, k, s, sn);
                    float next = sn;
                    if (done)
                        next = this->rst->enabled ? arm_reset_value(*this->rst, a, this->ends, k, J) : init_state[a * D + k];
                    st[rr][0] = next;
                    put_x(r, k, next);
                }
                double sx = 0.0, sy = 0.0, sa = 0.0;
                for (int jj = 0; jj < J; ++jj) sx += (double)__shfl(cj, jj);
                for (int jj = 0; jj < J; ++jj) sy += (double)__shfl(sj, jj);
                for (int jj = 0; jj < J; ++jj) {
                    const double aj = (double)__shfl(ac, jj);
                    sa += aj * aj;
                }
                if (owner()) {
                    const float rew = arm_reward(sx, sy, sa, w, g0, g1);
                    close(a, p, rew);
                    if (mon.ep_reward) episode_step(mon, a, ep_reward[r], ep_steps[r], rew, done);
                }
            }
        }
        this->tick(done);                               // (ROWDONE: never with a task)
    }
    // the states the actors are left in
    __device__ __forceinline__ void store() const {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = erow0 + rr;
#pragma unroll
            for (int i = 0; i < KPL; ++i) {
                const int k = kel(i);
                if (k < D && r < nrows) state[(row0 + r) * D + k] = st[rr][i];
            }
            if (mon.ep_reward && owner() && r < nrows) {
                mon.ep_reward[row0 + r] = ep_reward[r];
                mon.ep_steps[row0 + r] = ep_steps[r];
            }
        }
    }
};

// A layer in front of the actor's (GATE: the LSTM gate pass): packed weights W, bias, H outputs over K inputs read from
// the x tile, output tile at off_out (row stride ldo), no activation
struct PreLayer {
    const float* W;
    const float* bias;
    int H, K, off_out, ldo;
};

// The first nl actor layers of the block's 4 RG rows on the 4-row loop (smx_rows4_mma.inc.h), NT feature tiles a wave
// per pass: bias, then ReLU on the hidden layers and act_f(., out_act) on the output layer.  The layer sums of a row do
// not depend on RG or NT (k ascending within each kq class, then the classes meet).  after(l) follows layer l's barrier.
// Layer 0 reads K0 inputs from column in0 on of the x tile (a plain MLP: the observation, in0 = 0, K0 = D).  GATE: layer
// -1 = `pre` runs first, from column 0 of the x tile (after(-1) then follows its barrier).  shift: floats added to every
// weight and bias pointer (the population rollout: from agent 0's copy to the workgroup's agent's).
template <int RG, int NT, bool GATE = false, typename After>
__device__ __forceinline__ void layers4(const RollBase& G, float* sm, int nl, int out_act, int wv, int lane, After after,
                                        int in0, int K0, const PreLayer& pre = PreLayer{}, size_t shift = 0) {
    const int fm = lane & 15, kq = lane >> 4;
#pragma unroll 1
    for (int l = GATE ? -1 : 0; l < nl; ++l) {
        const bool pl = GATE && l < 0;
        const float* Wp = (pl ? pre.W : (l == 0 ? G.P1 : (l == 1 ? G.P2 : G.P3))) + shift;
        const float* bias = (pl ? pre.bias : (l == 0 ? G.b1 : (l == 1 ? G.b2 : G.b3))) + shift;
        const int H = pl ? pre.H : (l == 0 ? G.H1 : (l == 1 ? G.H2 : G.A));
        const int K = pl ? pre.K : (l == 0 ? K0 : (l == 1 ? G.H1 : G.H2));
        const float* in_lds = sm + (pl ? 0 : (l == 0 ? in0 : (l == 1 ? G.off_h1 : G.off_h2)));
        const int ldi = pl ? G.ldx : (l == 0 ? G.ldx : (l == 1 ? G.ldh1 : G.ldh2));
        float* out_lds = sm + (pl ? pre.off_out : (l == 0 ? G.off_h1 : (l == 1 ? G.off_h2 : G.off_out)));
        const int ldo = pl ? pre.ldo : (l == 0 ? G.ldh1 : (l == 1 ? G.ldh2 : RLDO));
        const int tiles = (H + 15) >> 4;
        const int C2 = pack_chunks(K);
        const rsrc_t rw = make_rsrc(Wp, (unsigned)tiles * (unsigned)C2 * 2048u);
        const rsrc_t rbias = make_rsrc(bias, (unsigned)H * 4u);
#pragma unroll 1
        for (int tb = 0; tb < tiles; tb += RNWV * NT) {
            const int t0 = tb + wv;
            if (t0 >= tiles) continue;                            // (wave-uniform)
            float bs[NT];
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const int f = 16 * (t0 + RNWV * g) + fm;
                bs[g] = ld4(rbias, (f < H) ? (unsigned)f * 4u : OOB);
            }
            f32x4 acc[NT][RG];
#pragma unroll
            for (int g = 0; g < NT; ++g)
#pragma unroll
                for (int r = 0; r < RG; ++r) acc[g][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
            fwd_tiles4<NT, RG, true>(acc, rw, tiles, C2, in_lds, ldi, t0, RNWV, lane);
            // the kq groups meet; lane (fm, kq) then keeps row kq of every group: bias, activation, one word to LDS
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const int f = 16 * (t0 + RNWV * g) + fm;
                if (t0 + RNWV * g < tiles) {                      // (wave-uniform)
#pragma unroll
                    for (int r = 0; r < RG; ++r) {
                        float z = meet_rows(acc[g][r]);
                        z += bs[g];
                        if (l == 2) z = act_f(z, out_act);
                        else if (!pl) z = (z < 0.f) ? 0.f : z;
                        out_lds[(4 * r + kq) * ldo + f] = (f < H) ? z : 0.f;
                    }
                }
            }
        }
        SMX_LDS_BARRIER();
        after(l);
    }
}

// ---- PPO -------------------------------------------------------------------------------------------------------------

// the FIFO row of actor a's window at the k-th closing step of the launch: (cursor + k n + a) % capacity, given
// base = (cursor + k n) % capacity (a < n <= capacity: one wrap at most)
__device__ __forceinline__ long long win_row(const WinArgs& W, long long base, long a) {
    const long long r = base + a;
    return r >= W.capacity ? r - W.capacity : r;
}

// A closing window's N steps from a carry ring to its FIFO row: ld(slot, c) reads column c of ring slot `slot`, st(u, c,
// v) stores it as step u of the window (streaming).  The window's first step sits in slot `first`; U steps' C columns are
// loaded before any of them is stored, so that U C loads are in flight (the ring was written steps ago: L2 or HBM).
template <int U, int C, typename Ld, typename St>
__device__ __forceinline__ void copy_window(int N, int first, Ld ld, St st) {
#pragma unroll 1
    for (int u0 = 0; u0 < N; u0 += U) {
        int s0 = first + u0;
        s0 = s0 >= N ? s0 - N : s0;
        float v[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = s0 + u >= N ? s0 + u - N : s0 + u;
#pragma unroll
            for (int c = 0; c < C; ++c) v[u][c] = (u0 + u < N) ? ld(s, c) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (u0 + u < N)
#pragma unroll
                for (int c = 0; c < C; ++c) st(u0 + u, c, v[u][c]);
    }
}

// ---- the policy step's pieces the recording and the evaluation kernels share ---------------------------------------------

__device__ __forceinline__ float clip1(float a) {
    if (a == a) a = fminf(fmaxf(a, -1.0f), 1.0f);          // (numpy's clip keeps a NaN)
    return a;
}

// The sampling head (smx_diaggauss_sample_f32's expressions) on one (actor, action) pair: the clipped action from the
// pair's mean, standard deviation and normal draw; noisy false: the policy acts on its mean.
__device__ __forceinline__ float gauss_act(float mu, float sd, float ev, bool noisy) {
    return clip1(noisy ? ev * sd + mu : mu);
}

// The LSTM cell pass behind the gate pass (smx_lstm.hip's gate functions and update order): thread q owns the (row, unit)
// pairs q + RNTH i.  hook(r, j, h_before, c_before) runs between reading the pair's old state and writing its new one
// (h_before: the tile's word, read where the hook uses it); a padded unit stays exactly zero whatever its weights.
template <int RB, typename Args, typename Hook>
__device__ __forceinline__ void lstm_cells(const Args& G, float* sm, int tid, Hook hook) {
    const float* gs = sm + G.off_g;
    const int H = G.H, ldx = G.ldx, ldg = G.ldg, Hl = G.Hl;
    float* cst = sm + G.off_c;
#pragma unroll 1
    for (int q = tid; q < RB * H; q += RNTH) {
        const int r = q / H, j = q - r * H;
        const float* g = gs + r * ldg + j;
        const float gi = fast_sigm(g[0]), gf = fast_sigm(g[H]), gg = fast_tanh(g[2 * H]), go = fast_sigm(g[3 * H]);
        const float c0 = cst[q];
        float c = gf * c0 + gi * gg;
        float h = go * fast_tanh(c);
        if (j >= Hl) c = h = 0.f;
        hook(r, j, (const float&)sm[r * ldx + G.Dp + j], c0);
        cst[q] = c;
        sm[r * ldx + G.Dp + j] = h;
    }
    SMX_LDS_BARRIER();
}

// RG row groups of four actors per workgroup (round 6; smx_rows4_mma.inc.h).  1024 actors: RG = 1 -> 256 workgroups, one per
// CU.  The host picks the smallest RG whose grid fits the chip once (more actors per workgroup = fewer passes over the
// packed weights per actor; fewer = more CUs at work).
// LSTM (lstm_rollout_kernel): every step first runs the stem on the same loop -- the gate pass, ONE 4-row layer over K =
// Dp + H reading the x tile's row [x | 0 | h] against [W_ih | 0 | W_hh], gates to LDS; then the cell pass: thread q owns
// the (row, unit) pairs q + RNTH i (at most RG of them for H <= 128) and keeps their cells in LDS slots no other thread
// touches (registers are short at 16 actors); it writes h' back into the tile's h columns, where the actor's first
// layer reads it.
// WIN (ppo_window_kernel, lstm_window_kernel; Args carries a WinArgs W): the same steps, recorded as moving windows
// instead of rollout tables.  Step tau of an actor goes to slot tau % N of its carry rings (the state before it, the
// action, the reward, the pd; an LSTM state before every window start tau % adv == 0 to slot (tau / adv) % S) -- each
// value written and later read by the SAME lane, as DDPG's open transitions, so no barrier orders them and they carry
// from one launch to the next.  At the step that closes window j = tau + 1 - N (j >= 0, j % adv == 0), the lanes that
// wrote its steps copy them into the FIFO row (cursor + k n + a) % capacity (k: the closing steps of the launch before
// this one), with obs_next the observation after the step (the terminal one before a reset) and the window's dones 0
// but the last (= done: a window never crosses an episode, the clock restarts at 0).
// CLK (WIN only; Clk = ClkArgs): an episode clock per actor.  What a step takes from the shared clock t -- wslot, wfirst,
// wstart, wclose, done -- every reader forms for ITS actor row from the row's clock in LDS (rowclk), and a closing
// window's FIFO row comes from the call's row_off table, (cursor + row_off[step, a]) % capacity, where the clock closes
// one and the word lies in [0, rows).
// TASK (WIN without CLK only): the environment's dynamics, EnvLanes' TASK; S: its reset stream (SMX_TASK_REACH; rst_arg).
template <int RG, int NT, bool LSTM, bool COLS, bool WIN = false, bool CLK = false, int TASK = SMX_TASK_DRIFT, typename Args,
          typename Clk = NoClk>
__device__ __forceinline__ void ppo_rollout(Args G, Clk C = Clk{}, const smx_reset_stream* S = nullptr) {
    static_assert(!CLK || WIN, "per-actor clocks: the windowed kernels");
    static_assert(TASK == SMX_TASK_DRIFT || (WIN && !CLK), "tasks: the windowed kernels on the shared clock");
    constexpr int RB = 4 * RG;                       // actors per workgroup
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fm = lane & 15, kq = lane >> 4;
    const int A = G.A, R = G.R, D = G.D;
    const float* h2s = sm + G.off_h2;
    const float* outs = sm + G.off_out;
    float* s_act = sm + G.off_act;              // [RB][RMAX_A] clipped actions
    const int ldh2 = G.ldh2;

    clear_tiles(G, sm, tid, G.zsum, G.zsumsq, G.zcount, G.zeps);
    EnvLanes<RB, COLS, TASK> E(G, sm, G.zsum ? sm + G.off_z : nullptr, wv, lane);
    if constexpr (TASK != SMX_TASK_DRIFT) E.begin(S, G.t0);
    SMX_LDS_BARRIER();
    E.start();
    SMX_LDS_BARRIER();
    const long row0 = E.row0;
    const int nrows = E.nrows;
    int* clk = nullptr;                          // (CLK) [RB][3]: clock, episode length, this step's row_off word
    if constexpr (CLK) {
        clk = (int*)(sm + C.off);
        if (tid < nrows) clk_load(C, clk, tid, row0);        // (first read behind the first layer's barrier)
    }
    if constexpr (LSTM) {
        float* cst = sm + G.off_c;
#pragma unroll 1
        for (int q = tid; q < RB * G.H; q += RNTH) {
            const int r = q / G.H, j = q - r * G.H;
            const bool rec = r < nrows && j < G.Hl;
            const long o = (row0 + r) * G.Hl + j;
            cst[q] = (rec && G.c0) ? G.c0[o] : 0.f;
            if (rec && G.h0) sm[r * G.ldx + G.Dp + j] = G.h0[o];
        }
        SMX_LDS_BARRIER();
    }

    // ---- the output layer (K = H2, <= 32 outputs) is a latency chain if two waves walk its chunks alone (measured: 5.0 k
    // cycles of a 36 k-cycle step for 2 tiles x 8 chunks).  Its K is split over the EIGHT waves instead: wave w owns chunk w
    // of both tiles, keeps those 4 KB of packed weights in registers for the whole rollout (no loads at all), and the
    // eight partial sums of a (row, action) pair meet in the sampling head, added in wave order.  Shapes with more than 8
    // chunks (H2 > 256) or more than 2 tiles take the generic loop.
    // (ppo_eval_kernel repeats the load, the chunk pass and the fold word for word: moved into functions, whether over a
    // struct or over these locals, they compiled to other SGPR-spill counts in several recording kernels)
    const int tiles3 = (A + 15) >> 4, C3 = pack_chunks(G.H2);
    const bool l3res = C3 <= RNWV && tiles3 <= 2;
    // (16-actor blocks: the register budget has no room for them -- re-read from L2 every step, the same words)
    constexpr bool W3REG = RG < 4;
    float4 w3a[2], w3b[2];
    auto load_w3 = [&]() {
        const rsrc_t rw3 = make_rsrc(G.P3, (unsigned)tiles3 * (unsigned)C3 * 2048u);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const unsigned o = (l3res && g < tiles3 && wv < C3)
                ? (((unsigned)g * (unsigned)C3 + (unsigned)wv) * 512u + (unsigned)lane * 4u) * 4u : OOB;
            w3a[g] = ld16(rw3, o);
            w3b[g] = ld16(rw3, o == OOB ? OOB : o + 1024u);
        }
    };
    if (W3REG) load_w3();
    float* red3 = sm + G.off_red3;
    // the sampling head's per-pair constants (the same expressions, formed once instead of every step)
    const int hr = tid / A, hj = tid - hr * A;            // RB x A <= 512 pairs
    const float b3v = G.b3[hj];
    float sd0 = expf(G.log_var[hj]);
    if (G.noise_scale && hr < nrows) sd0 = sd0 * G.noise_scale[row0 + hr];
    const bool noisy = noise_on(G.eps, G.nstream);
    int t = G.t0;
    long long wbase = 0;                         // (WIN) (cursor + k n) % capacity after k closing steps
    if constexpr (WIN) wbase = G.W.cursor;
    RWALL(12); RCYC(13);
#pragma unroll 1
    for (int step = 0; step < G.steps; ++step) {
        const int slot = G.slot0 + step;
        const bool last_step = step + 1 == G.steps;
        // (WIN) this step's ring slot, whether it starts a window / closes one, the closing window's first slot
        int wslot = 0, wfirst = 0;
        bool wstart = false, wclose = false;
        if constexpr (WIN) {
            const int wj = t + 1 - G.W.N;
            wslot = t % G.W.N;
            wfirst = (t + 1) % G.W.N;
            wstart = t % G.W.adv == 0;
            wclose = wj >= 0 && wj % G.W.adv == 0;
        }
        const bool done = (t + 1 >= G.episode_len);
        // what the step takes from the clock, for actor row r: the shared values, or (CLK) formed from the row's own
        struct RowClk { int t, wslot, wfirst; bool wstart, wclose, done; };
        auto rowclk = [&](int r) -> RowClk {
            if constexpr (CLK) {
                const int tr = clk[3 * r], wj = tr + 1 - G.W.N;
                return RowClk{tr, tr % G.W.N, (tr + 1) % G.W.N, tr % G.W.adv == 0, wj >= 0 && wj % G.W.adv == 0,
                              tr + 1 >= clk[3 * r + 1]};
            } else {
                (void)r;
                return RowClk{t, wslot, wfirst, wstart, wclose, done};
            }
        };
        // the FIFO row of actor a's closing window; (CLK) `off`: its row_off word, which must lie in [0, rows) -- else
        // `closes` turns false and nothing is written
        auto fifo_row = [&](long a, int off, bool& closes) -> long long {
            if constexpr (CLK) {
                (void)a;
                closes = closes && off >= 0 && off < C.rows;
                return closes ? clk_row(G.W.cursor, G.W.capacity, off) : 0;
            } else if constexpr (WIN) {
                (void)off;
                return closes ? win_row(G.W, wbase, a) : 0;
            } else {
                (void)a; (void)off; (void)closes;
                return 0;
            }
        };
        RSTAMP(0);
        // this step's normal draw of the lane's (row, action) pair, requested before the layers (consumed behind them)
        float ev = 0.f;
        if (noisy && hr < nrows) ev = noise_pick(G.eps, ((size_t)step * G.n + row0 + hr) * A + hj, G.nstream, row0 + hr, step, hj);
        int hoff = -1;                               // (CLK) the pair's row_off word, requested here for the same reason
        if constexpr (CLK) {
            if (hr < nrows) hoff = C.row_off[(size_t)step * G.n + row0 + hr];
        }
        // ---- the three layers (the output layer below when its weights are register-resident) -------------------
        if constexpr (LSTM) {
            const PreLayer gate{G.Pg, G.bg, 4 * G.H, G.Dp + G.H, G.off_g, G.ldg};
            layers4<RG, NT, true>(G, sm, l3res ? 2 : 3, G.out_act, wv, lane, [&](int l) {
                if (l >= 0) { RSTAMP(1 + l); return; }
                RSTAMP(6);
                // ---- the cell pass; the hook records the state BEFORE the step
                lstm_cells<RB>(G, sm, tid, [&](int r, int j, const float& hb, float c0) {
                    const int Hl = G.Hl;
                    if (r < nrows && j < Hl) {
                        const long a = row0 + r;
                        if (G.cell_roll) {
                            float* cp = G.cell_roll + ((a * R + slot) * 2) * Hl + j;
                            __builtin_nontemporal_store(hb, cp);
                            __builtin_nontemporal_store(c0, cp + Hl);
                        }
                        if (last_step && G.h_before) {
                            G.h_before[a * Hl + j] = hb;
                            G.c_before[a * Hl + j] = c0;
                        }
                        if constexpr (WIN) {
                            const WinArgs& W = G.W;
                            float* cc = W.ccell + (size_t)a * W.S * 2 * Hl + j;
                            const RowClk k = rowclk(r);
                            if (k.wstart) {
                                float* cw = cc + (size_t)((k.t / W.adv) % W.S) * 2 * Hl;
                                cw[0] = hb;
                                cw[Hl] = c0;
                            }
                            bool closes = k.wclose;
                            // ((CLK) the row_off word is read here, at closing steps only: the row's head lane
                            // publishes its copy only behind the layers)
                            int off = 0;
                            if constexpr (CLK) {
                                if (closes) off = C.row_off[(size_t)step * G.n + a];
                            }
                            const long long row = fifo_row(a, off, closes);
                            if (closes) {
                                const float* cr = cc + (size_t)(((k.t + 1 - W.N) / W.adv) % W.S) * 2 * Hl;
                                float* d = W.cells + row * 2 * Hl + j;
                                __builtin_nontemporal_store(cr[0], d);
                                __builtin_nontemporal_store(cr[Hl], d + Hl);
                            }
                        }
                    }
                });
                RSTAMP(7);
            }, G.Dp, G.H, gate);
        } else {
            layers4<RG, NT>(G, sm, l3res ? 2 : 3, G.out_act, wv, lane, [&](int l) { RSTAMP(1 + l); }, 0, G.D);
        }
        if (l3res) {
            if (!W3REG) load_w3();
            // wave w: chunk w of the output layer against h2 (zero weights past the last chunk: a zero partial sum)
            // (RC row groups at a time: the register budget of 16-actor blocks; a row group's sums do not depend on it)
            constexpr int RC = RG < 4 ? RG : 1;
#pragma unroll 1
            for (int rg0 = 0; rg0 < RG; rg0 += RC) {
            const float* bp = h2s + (lane & 3) * ldh2 + 8 * kq + 32 * (wv < C3 ? wv : 0) + 4 * rg0 * ldh2;
            f32x4 a3[2][RC];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int r = 0; r < RC; ++r) a3[g][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float4 x0[RC], x1[RC];
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                x0[r] = *(const float4*)(bp + 4 * r * ldh2);
                x1[r] = *(const float4*)(bp + 4 * r * ldh2 + 4);
            }
#define SMX_L3(X, W, E)                                                      \
            _Pragma("unroll") for (int g = 0; g < 2; ++g)                    \
                _Pragma("unroll") for (int r = 0; r < RC; ++r) a3[g][r] = MFMA4(X[r].E, W[g].E, a3[g][r]);
            SMX_L3(x0, w3a, x) SMX_L3(x0, w3a, y) SMX_L3(x0, w3a, z) SMX_L3(x0, w3a, w)
            SMX_L3(x1, w3b, x) SMX_L3(x1, w3b, y) SMX_L3(x1, w3b, z) SMX_L3(x1, w3b, w)
#undef SMX_L3
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int r = 0; r < RC; ++r) {
                    const float z = meet_rows(a3[g][r]);
                    red3[(wv * RB + 4 * (rg0 + r) + kq) * 32 + 16 * g + fm] = z;
                }
            }
            SMX_LDS_BARRIER();
            RSTAMP(3);
        }
        // ---- sampling head: one (actor, action) pair per lane ---------------------------------------------------
        if (hr < nrows) {
            const long a = row0 + hr;
            float mu;
            if (l3res) {
                float p8[RNWV];
#pragma unroll
                for (int w = 0; w < RNWV; ++w) p8[w] = red3[(w * RB + hr) * 32 + hj];
                float z = p8[0];
#pragma unroll
                for (int w = 1; w < RNWV; ++w) z += p8[w];
                mu = act_f(z + b3v, G.out_act);
            } else {
                mu = outs[hr * RLDO + hj];
            }
            const float sd = sd0;
            const float act = gauss_act(mu, sd, ev, noisy);
            s_act[hr * RMAX_A + hj] = act;
            if constexpr (!WIN) {
            // (the rollout tables are written once and read by a later launch: streaming stores, so that 3 MB of them per
            // step do not push the packed weights -- re-read by every workgroup every step -- out of the L2s)
            if (G.act_roll) __builtin_nontemporal_store(act, &G.act_roll[(a * R + slot) * A + hj]);
            if (G.pd_roll) {
                __builtin_nontemporal_store(mu, &G.pd_roll[(a * R + slot) * 2 * A + hj]);
                __builtin_nontemporal_store(sd, &G.pd_roll[(a * R + slot) * 2 * A + A + hj]);
            }
            } else {
                // the pair's action and pd into the ring (plain stores: read back within N steps), the window's N of
                // them into the FIFO row when one closes
                const WinArgs& W = G.W;
                const int N = W.N;
                float* ca = W.cact + (size_t)a * N * A + hj;
                float* cp = W.cpd + (size_t)a * N * 2 * A + hj;
                const RowClk k = rowclk(hr);
                ca[(size_t)k.wslot * A] = act;
                cp[(size_t)k.wslot * 2 * A] = mu;
                cp[(size_t)k.wslot * 2 * A + A] = sd;
                // ((CLK) the row's word for the environment lanes, which read it behind the barrier below)
                if constexpr (CLK) {
                    if (hj == 0) clk[3 * hr + 2] = hoff;
                }
                bool closes = k.wclose;
                const long long row = fifo_row(a, hoff, closes);
                if (closes) {
                    float* da = W.act + (row * N) * A + hj;
                    float* dp = W.pd + (row * N) * 2 * A + hj;
                    copy_window<8, 3>(N, k.wfirst,
                        [&](int s, int c) { return c == 0 ? ca[(size_t)s * A] : cp[(size_t)s * 2 * A + (c - 1) * A]; },
                        [&](int u, int c, float v) {
                            if (c == 0) __builtin_nontemporal_store(v, da + (size_t)u * A);
                            else __builtin_nontemporal_store(v, dp + (size_t)u * 2 * A + (c - 1) * A);
                        });
                }
            }
        }
        SMX_LDS_BARRIER();
        RSTAMP(4);
        // ---- environment step of the actors (smx_synth_env_step_f32's expressions), recording, next x tile ------
        if constexpr (!WIN) {
        E.step(s_act, done,
               [&](long a) { return G.obs_roll ? G.obs_roll + (a * R + slot) * D : nullptr; },
               [&](long a, float* orow, int k, float s, float sn) {
                   if (orow) {
                       __builtin_nontemporal_store(s, &orow[k]);
                       // the observation AFTER the step: row slot + 1 -- which the next step of this launch writes itself
                       // (the same value, or the reset state when the episode ended here), so only the launch's last
                       // step stores it
                       if (slot + 1 < R) { if (last_step) __builtin_nontemporal_store(sn, &orow[D + k]); }
                       else if (G.obs_last) G.obs_last[a * D + k] = sn;     // (the replay's obs_next field)
                   }
               },
               [&](long a, float*, float rew) {
                   if (G.rew_roll) __builtin_nontemporal_store(rew, &G.rew_roll[a * R + slot]);
                   if (G.done_roll) __builtin_nontemporal_store(done ? 1.0f : 0.0f, &G.done_roll[a * R + slot]);
               });
        } else {
            // the state before the step into the ring, obs_next (the next state before any reset) and the window's
            // rewards and dones into the FIFO row when one closes; its observations below
            const WinArgs& W = G.W;
            const int N = W.N;
            // (the row's slot, closing window and done travel in what open(a) returns: with CLK they are the row's own)
            struct Row { float* co; long long row; int wslot, wfirst; bool wclose, done; };
            auto open_row = [&](long a) {
                const int r = (int)(a - row0);
                const RowClk k = rowclk(r);
                bool closes = k.wclose;
                int off = 0;
                if constexpr (CLK) off = clk[3 * r + 2];
                const long long row = fifo_row(a, off, closes);
                return Row{W.cobs + ((size_t)a * N + k.wslot) * D, row, k.wslot, k.wfirst, closes, k.done};
            };
            E.template step<CLK>(s_act, done, open_row,
                   [&](long, const Row& p, int k, float s, float sn) {
                       p.co[k] = s;
                       if (p.wclose) __builtin_nontemporal_store(sn, &W.obs_next[p.row * D + k]);
                   },
                   [&](long a, const Row& p, float rew) {
                       float* cr = W.crew + (size_t)a * N;
                       cr[p.wslot] = rew;
                       if (p.wclose) {
                           float* dr = W.rew + p.row * N;
                           float* dd = W.done + p.row * N;
                           const bool last = p.done;
                           copy_window<8, 1>(N, p.wfirst, [&](int s, int) { return cr[s]; },
                                             [&](int u, int, float v) {
                                                 __builtin_nontemporal_store(v, dr + u);
                                                 __builtin_nontemporal_store((last && u == N - 1) ? 1.0f : 0.0f, dd + u);
                                             });
                       }
                   });
            if (CLK || wclose) {
                // the window's observations: every lane copies the elements it wrote, RPW rows of KPL each
                using EL = decltype(E);
#pragma unroll
                for (int rr = 0; rr < EL::RPW; ++rr) {
                    const int r = E.erow0 + rr;
                    if (r < nrows) {
                        const long a = row0 + r;
                        const Row p = open_row(a);
                        if (!p.wclose) continue;
                        const float* co = W.cobs + (size_t)a * N * D;
                        float* dst = W.obs + p.row * N * D;
                        copy_window<32 / EL::KPL, EL::KPL>(N, p.wfirst,
                            [&](int s, int i) { const int k = E.kel(i); return k < D ? co[(size_t)s * D + k] : 0.f; },
                            [&](int u, int i, float v) {
                                const int k = E.kel(i);
                                if (k < D) __builtin_nontemporal_store(v, &dst[(size_t)u * D + k]);
                            });
                    }
                }
            }
            if (!CLK && wclose) {
                wbase += G.n;
                wbase = wbase >= G.W.capacity ? wbase - G.W.capacity : wbase;
            }
        }
        t = done ? 0 : t + 1;
        SMX_LDS_BARRIER();
        if constexpr (CLK) {
            // every reader of the step's clocks is behind the barrier above; the next ones follow a layer's barrier
            if (tid < nrows) {
                const int tr = clk[3 * tid];
                clk[3 * tid] = (tr + 1 >= clk[3 * tid + 1]) ? 0 : tr + 1;
            }
        }
        RSTAMP(5);
    }
    RWALL(14); RCYC(15);
    E.store();
    if constexpr (LSTM) {
        const float* cst = sm + G.off_c;
#pragma unroll 1
        for (int q = tid; q < RB * G.H; q += RNTH) {
            const int r = q / G.H, j = q - r * G.H;
            if (r < nrows && j < G.Hl) {             // (h, c: the thread's own last writes to the tiles)
                G.hN[(row0 + r) * G.Hl + j] = sm[r * G.ldx + G.Dp + j];
                G.cN[(row0 + r) * G.Hl + j] = cst[q];
            }
        }
    }
}

template <int RG>
__global__ __launch_bounds__(RNTH) void rollout_kernel(RollArgs G) {
    ppo_rollout<RG, 3, false, true>(G);
}

// 4, 8 and 16 actors per workgroup, all on the 4-row loop; every block size gives the same bits.  16 (the register
// budget): two feature tiles a wave per pass, the environment lanes' per-element constants formed every step, the split
// output layer's weights re-read every step and its row groups taken one at a time
template <int RG>
__global__ __launch_bounds__(RNTH) void lstm_rollout_kernel(LArgs G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, true, RG < 4>(G);
}

// The windowed rollouts (smx_synth_ppo_window_rollout_f32): the two kernels above recording moving windows into the
// FIFO; the plain-MLP policy on the 4-row loop at 16 actors too (as the LSTM kernel), so 4, 8 and 16 give the same bits
template <int RG>
__global__ __launch_bounds__(RNTH) void ppo_window_kernel(RollArgsW G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, false, RG < 4, true>(G);
}

template <int RG>
__global__ __launch_bounds__(RNTH) void lstm_window_kernel(LArgsW G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, true, RG < 4, true>(G);
}

// The same two on another task's dynamics (smx_synth_ppo_window_rollout_task_f32)
template <int RG, int TASK>
__global__ __launch_bounds__(RNTH) void ppo_window_task_kernel(WithRst<RollArgsW> G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, false, RG < 4, true, false, TASK>((RollArgsW)G, NoClk{}, rst_arg<WithRst<RollArgsW>>());
}

template <int RG, int TASK>
__global__ __launch_bounds__(RNTH) void lstm_window_task_kernel(WithRst<LArgsW> G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, true, RG < 4, true, false, TASK>((LArgsW)G, NoClk{}, rst_arg<WithRst<LArgsW>>());
}

// The same two with an episode clock per actor (smx_synth_ppo_window_rollout_clocks_f32)
template <int RG>
__global__ __launch_bounds__(RNTH) void ppo_window_clk_kernel(WithClk<RollArgsW> G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, false, RG < 4, true, true>((RollArgsW)G, G.clk);
}

template <int RG>
__global__ __launch_bounds__(RNTH) void lstm_window_clk_kernel(WithClk<LArgsW> G) {
    ppo_rollout<RG, RG == 4 ? 2 : 3, true, RG < 4, true, true>((LArgsW)G, G.clk);
}

constexpr int RTG = 3;            // feature tiles a wave carries per pass (register budget of two waves per SIMD)

// More actors than 8 per CU (n > 2048 on 256 CUs): 16 actors per workgroup on v_mfma_f32_16x16x4_f32 (the row-block loop of
// smx_epoch_mma.inc.h, bit-identical means to smx_epoch_forward_f32) -- at 16 rows the matrix pipes bound the step and one
// 16x16x4 operand read feeds 16 rows where 4x4x1 needs four (measured, 4096 actors x 128 steps: 2.95 ms against 3.9 ms on
// four row groups of the 4-row loop).
__global__ __launch_bounds__(RNTH) void rollout16_kernel(RollArgs G) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fm = lane & 15, kq = lane >> 4;
    const int D = G.D, A = G.A, R = G.R;
    float* xs = sm;
    float* h1s = sm + G.off_h1;
    float* h2s = sm + G.off_h2;
    float* outs = sm + G.off_out;
    float* s_act = sm + G.off_act;              // [16][RMAX_A] clipped actions
    const int ldx = G.ldx, ldh1 = G.ldh1, ldh2 = G.ldh2;

    clear_tiles(G, sm, tid, G.zsum, G.zsumsq, G.zcount, G.zeps);
    EnvLanes<ER, false> E(G, sm, G.zsum ? sm + G.off_z : nullptr, wv, lane);
    SMX_LDS_BARRIER();
    E.start();
    SMX_LDS_BARRIER();
    const long row0 = E.row0;
    const int nrows = E.nrows;

    const bool noisy = noise_on(G.eps, G.nstream);
    int t = G.t0;
    RWALL(12); RCYC(13);
#pragma unroll 1
    for (int step = 0; step < G.steps; ++step) {
        const int slot = G.slot0 + step;
        RSTAMP(0);
        // this step's normal draw of the lane's (row, action) pair, requested before the layers (consumed behind them)
        const int hr = tid / A, hj = tid - hr * A;        // 16 x A <= 512 pairs
        float ev = 0.f;
        if (noisy && hr < nrows) ev = noise_pick(G.eps, ((size_t)step * G.n + row0 + hr) * A + hj, G.nstream, row0 + hr, step, hj);
        // ---- the three layers: the loop of epoch_fwd_kernel without its global stores ---------------------
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            const float* Wp = l == 0 ? G.P1 : (l == 1 ? G.P2 : G.P3);
            const float* bias = l == 0 ? G.b1 : (l == 1 ? G.b2 : G.b3);
            const int H = l == 0 ? G.H1 : (l == 1 ? G.H2 : A);
            const int K = l == 0 ? D : (l == 1 ? G.H1 : G.H2);
            const float* in_lds = l == 0 ? xs : (l == 1 ? h1s : h2s);
            const int ldi = l == 0 ? ldx : (l == 1 ? ldh1 : ldh2);
            float* out_lds = l == 0 ? h1s : (l == 1 ? h2s : outs);
            const int ldo = l == 0 ? ldh1 : (l == 1 ? ldh2 : RLDO);
            const int tiles = (H + 15) >> 4;
            const int C2 = pack_chunks(K);
            const rsrc_t rw = make_rsrc(Wp, (unsigned)tiles * (unsigned)C2 * 2048u);
            const rsrc_t rbias = make_rsrc(bias, (unsigned)H * 4u);
#pragma unroll 1
            for (int tb = 0; tb < tiles; tb += RNWV * RTG) {
                const int t0 = tb + wv;
                int nt = (tiles - t0 + RNWV - 1) / RNWV;
                nt = nt < 0 ? 0 : (nt > RTG ? RTG : nt);
                float bs[RTG][4];
#pragma unroll
                for (int g = 0; g < RTG; ++g) {
                    const int f0 = 16 * (t0 + RNWV * g) + 4 * kq;
#pragma unroll
                    for (int r = 0; r < 4; ++r) bs[g][r] = ld4(rbias, (g < nt) ? (unsigned)(f0 + r) * 4u : OOB);
                }
                f32x4 acc[TG];
#pragma unroll
                for (int g = 0; g < TG; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (nt > 2) fwd_tiles<3>(acc, rw, tiles, C2, in_lds, ldi, t0, RNWV, lane);
                else if (nt > 1) fwd_tiles<2>(acc, rw, tiles, C2, in_lds, ldi, t0, RNWV, lane);
                else if (nt > 0) fwd_tiles<1>(acc, rw, tiles, C2, in_lds, ldi, t0, RNWV, lane);
#pragma unroll
                for (int g = 0; g < RTG; ++g) {
                    if (g < nt) {
                        const int f0 = 16 * (t0 + RNWV * g) + 4 * kq;
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float z = acc[g][r] + bs[g][r];
                            if (l == 2) z = act_f(z, G.out_act);
                            else z = (z < 0.f) ? 0.f : z;
                            v[r] = (f0 + r < H) ? z : 0.f;
                        }
                        *(float4*)(out_lds + fm * ldo + f0) = make_float4(v[0], v[1], v[2], v[3]);
                    }
                }
            }
            SMX_LDS_BARRIER();
            RSTAMP(1 + l);
        }
        // ---- sampling head (smx_diaggauss_sample_f32's expressions): one (actor, action) pair per lane -------
        const bool done = (t + 1 >= G.episode_len);
        if (hr < nrows) {
            const long a = row0 + hr;
            const float mu = outs[hr * RLDO + hj];
            float sd = expf(G.log_var[hj]);
            if (G.noise_scale) sd = sd * G.noise_scale[a];
            const float act = gauss_act(mu, sd, ev, noisy);
            s_act[hr * RMAX_A + hj] = act;
            if (G.act_roll) G.act_roll[(a * R + slot) * A + hj] = act;
            if (G.pd_roll) {
                G.pd_roll[(a * R + slot) * 2 * A + hj] = mu;
                G.pd_roll[(a * R + slot) * 2 * A + A + hj] = sd;
            }
        }
        SMX_LDS_BARRIER();
        RSTAMP(4);
        // ---- environment step of the 16 actors (smx_synth_env_step_f32's expressions), recording, next x tile ---
        E.step(s_act, done,
               [&](long a) { return G.obs_roll ? G.obs_roll + (a * R + slot) * D : nullptr; },
               [&](long a, float* orow, int k, float s, float sn) {
                   if (orow) {
                       orow[k] = s;
                       if (slot + 1 < R) orow[D + k] = sn;
                       else if (G.obs_last) G.obs_last[a * D + k] = sn;     // (the replay's obs_next field)
                   }
               },
               [&](long a, float*, float rew) {
                   if (G.rew_roll) G.rew_roll[a * R + slot] = rew;
                   if (G.done_roll) G.done_roll[a * R + slot] = done ? 1.0f : 0.0f;
               });
        t = done ? 0 : t + 1;
        SMX_LDS_BARRIER();
        RSTAMP(5);
    }
    RWALL(14); RCYC(15);
    E.store();
}

// ---- DDPG ------------------------------------------------------------------------------------------------------------

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

#include "smx_nstep.inc.h"                           // nstep_reward: the closing transition's reward

__device__ __forceinline__ long long ring_row(const DArgs& G, int kemit, long a) {
    return (G.cursor + (long long)kemit * G.n + a) % G.capacity;
}

// LayerNorm over the F features of the block's RB rows of a hidden tile, in place (behind the barrier that ends the
// layer; the caller barriers after it): ln_rows of smx_ln_rows.inc.h, which the DDPG row schedule shares -- given the same
// row the result has the bits smx_layernorm_forward_f32 produces.  gb = gamma [F] | beta [F].
constexpr int RLN_MAXC = 10;                         // columns per lane: H1, H2 <= 640
#include "smx_ln_rows.inc.h"

// RG row groups of four actors per workgroup; NT feature tiles a wave carries per pass.  Every block size gives the same
// bits (layers4).
// POP (variant->packed_pop; 4 RG divides the actors per agent): the same body with the layers run from
// the agent's copy.  At step measure_step the workgroups that hold an agent's first actor (a workgroup-uniform branch:
// layers4 has barriers) first run the clean actor -- G's own -- on the same x tile and keep that actor's outputs, then
// store the L2 distance of the two outputs of that one actor.
// LN (variant->ln): the same body with ln_rows behind the
// barrier of each hidden layer and a barrier of its own behind it.  The gains and biases the workgroup's layers use --
// the clean actor's, or (POP) its agent's perturbed ones -- are copied to LDS once; the clean actor of a measuring step
// reads its own from memory.
// CLK (the arguments then end with the clocks): an episode clock per actor, as in ppo_rollout -- tau, emit, slot, jslot
// and done are the actor row's own, a closing transition's ring row comes from the call's row_off table.
// (a task kernel's end with the reset stream)
template <bool POP, bool LN, bool CLK, int TASK = SMX_TASK_DRIFT>
using DdpgKernelArgs = std::conditional_t<TASK != SMX_TASK_DRIFT, WithRst<DdpgArgs<POP, LN>>,
                                          std::conditional_t<CLK, WithClk<DdpgArgs<POP, LN>>, DdpgArgs<POP, LN>>>;
// TASK (any actor on the shared clock; smx_synth_ddpg_rollout_variant_task_f32): the environment's dynamics, EnvLanes'
// TASK.  (A template parameter of the kernel itself: with the body moved into a function that two kernels call, every
// existing instantiation compiled to other code -- its arguments no longer read as kernel arguments.)
template <int RG, int NT, bool POP = false, bool LN = false, bool CLK = false, int TASK = SMX_TASK_DRIFT>
__global__ __launch_bounds__(RNTH) void ddpg_rollout_kernel(DdpgKernelArgs<POP, LN, CLK, TASK> G) {
    static_assert(TASK == SMX_TASK_DRIFT || !CLK, "tasks: the shared clock");
    constexpr int RB = 4 * RG;                       // actors per workgroup
    const auto C = clk_of(G);
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = G.D, A = G.A, N = G.N;
    const float* outs = sm + G.off_out;
    float* s_act = sm + G.off_act;                   // [RB][RMAX_A] the actions of this step (unused columns stay 0)

    clear_tiles(G, sm, tid, nullptr, nullptr, nullptr, 0.f);
    EnvLanes<RB, true, TASK> E(G, sm, nullptr, wv, lane);
    if constexpr (TASK != SMX_TASK_DRIFT) E.begin(rst_arg<DdpgKernelArgs<POP, LN, CLK, TASK>>(), G.t0);
    SMX_LDS_BARRIER();
    E.start();
    // the head's (actor, action) pair of this lane: its sigma and OU state for the whole rollout
    const int hr = tid / A, hj = tid - hr * A;       // RB x A <= 512 pairs
    const bool head = hr < E.nrows;
    const long ha = E.row0 + hr;
    double sig = 0.0, x = 0.0;
    if (head) {
        if (G.noise != SMX_DDPG_NOISE_NONE) sig = G.sigmas[ha];
        if (G.noise == SMX_DDPG_NOISE_OU) x = G.ou[ha * A + hj];
    }
    int* clk = nullptr;                              // (CLK) [RB][3]: clock, episode length, this step's row_off word
    if constexpr (CLK) {
        clk = (int*)(sm + C.off);
        if (tid < E.nrows) clk_load(C, clk, tid, E.row0);
    }
    SMX_LDS_BARRIER();

    const bool noisy = noise_on(G.eps, G.nstream);     // (never with SMX_DDPG_NOISE_NONE: common_args)
    // (POP) floats from agent 0's copy, which G.popnet points into, to the copy of this workgroup's agent
    size_t shift = 0;
    if constexpr (POP) shift = (size_t)(E.row0 / G.apa) * G.stride;
    // (LN) the actor's three layers from `net`, a LayerNorm behind each hidden one; gb: ln1.W | ln1.b | ln2.W | ln2.b
    auto actor =[&](const RollBase& net, size_t sh, const float* gb) {
        if constexpr (LN) {
            layers4<RG, NT>(net, sm, 3, SMX_ACT_TANH, wv, lane, [&](int l) {
                if (l < 2) {
                    float* tile = sm + (l == 0 ? G.off_h1 : G.off_h2);
                    const int ld = l == 0 ? G.ldh1 : G.ldh2, F = l == 0 ? G.H1 : G.H2;
                    const float* g = gb + (l == 0 ? 0 : 2 * G.H1);
                    ln_rows<RB, RNWV, RLN_MAXC>(tile, ld, tile, ld, F, g, g + F, G.ln.eps, wv, lane, LnNoEmit{});
                    SMX_LDS_BARRIER();
                }
            }, 0, G.D, PreLayer{}, sh);
        }
    };
    const float* gb = nullptr;
    if constexpr (LN) {
        const float* src = G.ln.g;
        if constexpr (POP) src = G.ln.pop + shift;
#ifdef SMX_LN_PARAMS_L2
        gb = src;                                    // (A/B builds only: the gains and biases read from memory every step)
#else
        float* dst = sm + G.ln.off;
        for (int i = tid; i < 2 * (G.H1 + G.H2); i += RNTH) dst[i] = src[i];
        gb = dst;
        SMX_LDS_BARRIER();
#endif
    }
    int tau = G.t0, kemit = 0;
#pragma unroll 1
    for (int step = 0; step < G.steps; ++step) {
        float ev = 0.f;                              // this step's draw, requested before the layers
        if (noisy && head) ev = noise_pick(G.eps, ((size_t)step * G.n + ha) * A + hj, G.nstream, ha, step, hj);
        int hoff = -1;                               // (CLK) the pair's row_off word, requested here for the same reason
        if constexpr (CLK) {
            if (head) hoff = C.row_off[(size_t)step * G.n + ha];
        }
        bool measure = false;
        float clean = 0.f;
        if constexpr (POP) {
            measure = step == G.measure_step && E.row0 % G.apa == 0;
            if (measure) {
                if constexpr (LN) actor(G, 0, G.ln.g);
                else layers4<RG, NT>(G, sm, 3, SMX_ACT_TANH, wv, lane, [](int) {}, 0, G.D);
                // (row 0's outputs; the layers below write the output tile again only behind two more barriers)
                if (tid < A) clean = outs[tid];
            }
        }
        // ---- the actor's three layers (ReLU, ReLU, tanh) --------------------------------------------------------
        if constexpr (LN && POP) actor(G.popnet, shift, gb);
        else if constexpr (LN) actor(G, 0, gb);
        else if constexpr (POP) layers4<RG, NT>(G.popnet, sm, 3, SMX_ACT_TANH, wv, lane, [](int) {}, 0, G.D, PreLayer{}, shift);
        else layers4<RG, NT>(G, sm, 3, SMX_ACT_TANH, wv, lane, [](int) {}, 0, G.D);
        if constexpr (POP) {
            if (measure && wv == 0) {
                // ddpg_agent.py:173-175 on the agent's first actor: the fp32 differences squared and summed in fp64
                const float d = tid < A ? outs[tid] - clean : 0.f;
                double q = 0.0;
                for (int j = 0; j < A; ++j) {
                    const double dj = (double)__shfl(d, j);
                    q += dj * dj;
                }
                if (lane == 0) G.dist[E.row0 / G.apa] = sqrt(q);
            }
        }
        const bool emit = tau >= N - 1;
        const int slot = tau % N, jslot = (tau + 1) % N;   // (transition j = tau - N + 1 sits in slot j % N)
        const bool done = (tau + 1 >= G.episode_len);
        // what the step takes from the clock, for actor row r: the shared values, or (CLK) formed from the row's own; a
        // closing transition's ring row from `off`, the row_off word, which must lie in [0, rows) -- else nothing closes
        struct Row { long long row; float* co; int tau, slot, jslot; bool emit, done; };
        auto open_row = [&](long a, int off) {
            float* co = G.cobs + (size_t)a * N * D;
            if constexpr (CLK) {
                const int r = (int)(a - E.row0), tr = clk[3 * r];
                const bool closes = tr >= N - 1 && off >= 0 && off < C.rows;
                return Row{closes ? clk_row(G.cursor, G.capacity, off) : 0, co, tr, tr % N, (tr + 1) % N, closes,
                           tr + 1 >= clk[3 * r + 1]};
            } else {
                (void)off;
                return Row{emit ? ring_row(G, kemit, a) : 0, co, tau, slot, jslot, emit, done};
            }
        };
        // ---- exploration: one (actor, action) pair per lane ------------------------------------------------------
        if (head) {
            // (two bodies that differ only in where the clock's values come from: written on open_row alone, the
            // shared-clock 8-actor kernel spills 36 bytes of scratch that it does not need with its own expressions)
            float* ca = G.cact + (size_t)ha * N * A + hj;
            if constexpr (CLK) {
                const Row p = open_row(ha, hoff);
                const float a = explore(outs[hr * RLDO + hj], G.noise, ev, sig, G.theta, G.dt, G.root_dt, p.tau, x);
                s_act[hr * RMAX_A + hj] = a;
                ca[(size_t)p.slot * A] = a;
                if (p.emit) G.act[p.row * A + hj] = ca[(size_t)p.jslot * A];
                // (the row's word for the environment lanes, which read it behind the barrier below)
                if (hj == 0) clk[3 * hr + 2] = hoff;
            } else {
                const float a = explore(outs[hr * RLDO + hj], G.noise, ev, sig, G.theta, G.dt, G.root_dt, tau, x);
                s_act[hr * RMAX_A + hj] = a;
                ca[(size_t)slot * A] = a;
                if (emit) G.act[ring_row(G, kemit, ha) * A + hj] = ca[(size_t)jslot * A];
            }
        }
        SMX_LDS_BARRIER();
        // ---- environment step (smx_synth_env_step_f32's expressions), n-step record, next x tile -------------------
        E.template step<CLK>(s_act, done,
               [&](long a) { return open_row(a, CLK ? clk[3 * (a - E.row0) + 2] : 0); },
               [&](long, const Row& p, int k, float s, float sn) {
                   p.co[(size_t)p.slot * D + k] = s;
                   if (p.emit) {
                       G.obs[p.row * D + k] = p.co[(size_t)p.jslot * D + k];
                       G.obs_next[p.row * D + k] = sn;
                   }
               },
               [&](long a, const Row& p, float rew) {
                   float* cr = G.crew + (size_t)a * N;
                   cr[p.slot] = rew;
                   if (p.emit) {
                       G.rew[p.row] = nstep_reward(cr, G.gpow, N, p.tau);
                       G.done[p.row] = p.done ? 1.0f : 0.0f;
                   }
               });
        if (emit) ++kemit;
        tau = done ? 0 : tau + 1;
        SMX_LDS_BARRIER();
        if constexpr (CLK) {
            // every reader of the step's clocks is behind the barrier above; the next ones follow a layer's barrier
            if (tid < E.nrows) {
                const int tr = clk[3 * tid];
                clk[3 * tid] = (tr + 1 >= clk[3 * tid + 1]) ? 0 : tr + 1;
            }
        }
    }
    // ---- the states the actors and their noise processes are left in ------------------------------------------------
    E.store();
    if (head && G.noise == SMX_DDPG_NOISE_OU) G.ou[ha * A + hj] = x;
}

// ---- evaluation ------------------------------------------------------------------------------------------------------
// Whole episodes of the policy, nothing recorded (smx_synth_ppo_eval_f32 / smx_synth_ddpg_eval_f32).  Episode e of actor g
// is a pure function of (parameters, streams, g, e), so the (actor, episode) pairs are independent ROWS: row r = a E + i
// is episode first_episode + i of local actor a, and a launch over n actors x E episodes is n E rows on the 4-, 8- or
// 16-row blocks of the rollouts above (RollBase.n: the rows; the tail block as there), each walked through exactly
// episode_len steps.  A row begins where eval_start puts it -- the stream's draw, else init_state[a] -- and `state` is
// never touched.  The policy step is the recording kernels': clear_tiles, layers4 with their NT / COLS choices, the split
// output layer (written out as in ppo_rollout), gauss_act, lstm_cells, EnvLanes::step with done = false throughout (the
// reset behind the final step is unobservable), so a row's actions have the bits of the recording launches at every
// block size.  The owner lane of a row keeps its fp64 return in a register, 0.0 + (double)rew in step order
// (episode_step's sum), and stores it once at the end: no LDS monitor words, no HBM traffic per step, no atomics.
struct EvalTail {
    int E;                                      // episodes per actor
    smx_reset_stream rst;                       // rst.episode: first_episode (read by eval_start only)
    double* returns;                            // [n, E] = [rows]
};
struct PEvalArgs : RollBase {
    int out_act;
    const float *log_var;
    const float *zsum, *zsumsq, *zcount;        // z-filter running sums or null
    float zeps;
    const float *Pg, *bg;                       // (LSTM) the gate pass, as LArgs
    int H, Hl, Dp, off_g, ldg, off_c;
    EvalTail ev;
};
struct DEvalArgs : RollBase { EvalTail ev; };
// Several parameter sets in one launch (smx_synth_*_eval_sets_f32; the SETS instantiations): a set's twin arguments --
// every parameter pointer into set 0's snapshot, n the rows of ONE set, returns set 0's [n, E] -- then the floats from
// one snapshot to the next.  The grid is (blocks of one set, sets): workgroup (x, s) is block x of the single-set launch
// with every parameter pointer moved on by s * set_stride floats and the returns by s * n.
template <typename Base>
struct WithSets : Base { long long set_stride; };
template <bool SETS>
using PEvalKernelArgs = std::conditional_t<SETS, WithSets<PEvalArgs>, PEvalArgs>;
template <bool SETS>
using DEvalKernelArgs = std::conditional_t<SETS, WithSets<DEvalArgs>, DEvalArgs>;
// floats from set 0's parameters to this workgroup's set's (0 in a single-set kernel: folded away)
template <bool SETS, typename KArgs>
__device__ __forceinline__ size_t eval_set_shift(const KArgs& G) {
    if constexpr (SETS) return (size_t)blockIdx.y * (size_t)G.set_stride;
    else return 0;
}

// where an evaluation kernel's arguments hold the stream (rst_arg's scalar loads: a step reads its disturbance there)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
template <typename KArgs>
__device__ __forceinline__ const smx_reset_stream* eval_rst_arg() {
    return (const smx_reset_stream*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(KArgs, ev) +
                                     __builtin_offsetof(EvalTail, rst));
}
#pragma clang diagnostic pop

// the first rows of the block's episodes into the environment lanes' registers (before E.start())
template <typename Lanes>
__device__ __forceinline__ void eval_start(Lanes& E, const EvalTail& V, bool stream) {
#pragma unroll
    for (int rr = 0; rr < Lanes::RPW; ++rr) {
        const int r = E.erow0 + rr;
        if (r >= E.nrows) continue;                     // (wave-uniform)
        const long row = E.row0 + r;
        const long a = row / V.E;
        const int i = (int)(row - a * V.E);
#pragma unroll
        for (int q = 0; q < Lanes::KPL; ++q) {
            const int k = E.kel(q);
            if (k < E.D) E.st[rr][q] = stream ? task_reset_value<Lanes::TASK_ID>(V.rst, a, i, k, E.D) : E.init_state[a * E.D + k];
        }
    }
}

// what the owner lane of the wave's (at most two) rows holds: their returns
struct EvalReturns {
    double r0 = 0.0, r1 = 0.0;
    template <typename Lanes>
    __device__ __forceinline__ void add(const Lanes& E, long row, float rew) {
        if ((int)(row - E.row0) == E.erow0) r0 = r0 + (double)rew;
        else r1 = r1 + (double)rew;
    }
    template <typename Lanes>
    __device__ __forceinline__ void store(const Lanes& E, double* returns) const {
        static_assert(Lanes::RPW <= 2, "two rows a wave at most");
        if (!E.owner()) return;
        if (E.erow0 < E.nrows) returns[E.row0 + E.erow0] = r0;
        if (Lanes::RPW > 1 && E.erow0 + 1 < E.nrows) returns[E.row0 + E.erow0 + 1] = r1;
    }
};
struct EvalNoRow {};

// PPO: ppo_window_kernel's / lstm_window_kernel's step (NT, COLS as there; gauss_act, lstm_cells) without a
// record.  LSTM rows start from zero h, c (PPOAgent.reset, ppo_agent.py:169-178).  A sampling launch (nstream.enabled:
// eval_stochastic) draws row (a, i)'s step t at normal(seed, actor_base + a, first_step + i L + t, j): what a serial run
// of the actor's E episodes on that stream draws.
template <int RG, int NT, bool LSTM, bool COLS, int TASK, bool SETS = false>
__global__ __launch_bounds__(RNTH) void ppo_eval_kernel(PEvalKernelArgs<SETS> G) {
    constexpr int RB = 4 * RG;
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fm = lane & 15, kq = lane >> 4;
    const int A = G.A;
    const float* h2s = sm + G.off_h2;
    const float* outs = sm + G.off_out;
    float* s_act = sm + G.off_act;              // [RB][RMAX_A] clipped actions
    const int ldh2 = G.ldh2;
    // (SETS) the one shift of the workgroup's set: every parameter read below goes through it
    const size_t shift = eval_set_shift<SETS>(G);

    if constexpr (SETS) {
        if (G.zsum) clear_tiles(G, sm, tid, G.zsum + shift, G.zsumsq + shift, G.zcount + shift, G.zeps);
        else clear_tiles(G, sm, tid, nullptr, nullptr, nullptr, G.zeps);
    } else {
        clear_tiles(G, sm, tid, G.zsum, G.zsumsq, G.zcount, G.zeps);
    }
    EnvLanes<RB, COLS, TASK> E(G, sm, G.zsum ? sm + G.off_z : nullptr, wv, lane, OwnStart{});
    if constexpr (TASK != SMX_TASK_DRIFT) {
        E.begin(eval_rst_arg<PEvalKernelArgs<SETS>>(), 0, G.ev.E);      // (done is false at every step)
        eval_start(E, G.ev, G.ev.rst.enabled != 0);
    } else {
        eval_start(E, G.ev, false);
    }
    SMX_LDS_BARRIER();
    E.start();
    SMX_LDS_BARRIER();
    const long row0 = E.row0;
    const int nrows = E.nrows;
    if constexpr (LSTM) {
        float* cst = sm + G.off_c;
#pragma unroll 1
        for (int q = tid; q < RB * G.H; q += RNTH) cst[q] = 0.f;       // (h: the tile's cleared columns)
        SMX_LDS_BARRIER();
    }
    // ---- the split output layer: ppo_rollout's, word for word (see there) ------------------------------------------------
    const int tiles3 = (A + 15) >> 4, C3 = pack_chunks(G.H2);
    const bool l3res = C3 <= RNWV && tiles3 <= 2;
    constexpr bool W3REG = RG < 4;
    float4 w3a[2], w3b[2];
    auto load_w3 = [&]() {
        const rsrc_t rw3 = make_rsrc(G.P3 + shift, (unsigned)tiles3 * (unsigned)C3 * 2048u);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const unsigned o = (l3res && g < tiles3 && wv < C3)
                ? (((unsigned)g * (unsigned)C3 + (unsigned)wv) * 512u + (unsigned)lane * 4u) * 4u : OOB;
            w3a[g] = ld16(rw3, o);
            w3b[g] = ld16(rw3, o == OOB ? OOB : o + 1024u);
        }
    };
    if (W3REG) load_w3();
    float* red3 = sm + G.off_red3;
    // the head's per-pair constants
    const int hr = tid / A, hj = tid - hr * A;            // RB x A <= 512 pairs
    const float b3v = (G.b3 + shift)[hj];
    const float sd0 = expf((G.log_var + shift)[hj]);
    const bool noisy = G.nstream.enabled != 0;
    // the pair's actor and the draw step of its episode's first step
    long ha = 0;
    int hk0 = 0;
    if (hr < nrows) {
        const long row = row0 + hr;
        ha = row / G.ev.E;
        hk0 = (int)(row - ha * G.ev.E) * G.episode_len;
    }
    EvalReturns ret;
#pragma unroll 1
    for (int step = 0; step < G.steps; ++step) {
        float ev = 0.f;                              // this step's draw, requested before the layers
        if (noisy && hr < nrows) ev = noise_draw(G.nstream, ha, hk0 + step, hj);
        if constexpr (LSTM) {
            const PreLayer gate{G.Pg, G.bg, 4 * G.H, G.Dp + G.H, G.off_g, G.ldg};
            layers4<RG, NT, true>(G, sm, l3res ? 2 : 3, G.out_act, wv, lane, [&](int l) {
                if (l >= 0) return;
                lstm_cells<RB>(G, sm, tid, [](int, int, const float&, float) {});
            }, G.Dp, G.H, gate, shift);
        } else {
            layers4<RG, NT>(G, sm, l3res ? 2 : 3, G.out_act, wv, lane, [](int) {}, 0, G.D, PreLayer{}, shift);
        }
        if (l3res) {
            if (!W3REG) load_w3();
            constexpr int RC = RG < 4 ? RG : 1;
#pragma unroll 1
            for (int rg0 = 0; rg0 < RG; rg0 += RC) {
            const float* bp = h2s + (lane & 3) * ldh2 + 8 * kq + 32 * (wv < C3 ? wv : 0) + 4 * rg0 * ldh2;
            f32x4 a3[2][RC];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int r = 0; r < RC; ++r) a3[g][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float4 x0[RC], x1[RC];
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                x0[r] = *(const float4*)(bp + 4 * r * ldh2);
                x1[r] = *(const float4*)(bp + 4 * r * ldh2 + 4);
            }
#define SMX_L3(X, W, E)                                                      \
            _Pragma("unroll") for (int g = 0; g < 2; ++g)                    \
                _Pragma("unroll") for (int r = 0; r < RC; ++r) a3[g][r] = MFMA4(X[r].E, W[g].E, a3[g][r]);
            SMX_L3(x0, w3a, x) SMX_L3(x0, w3a, y) SMX_L3(x0, w3a, z) SMX_L3(x0, w3a, w)
            SMX_L3(x1, w3b, x) SMX_L3(x1, w3b, y) SMX_L3(x1, w3b, z) SMX_L3(x1, w3b, w)
#undef SMX_L3
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int r = 0; r < RC; ++r) {
                    const float z = meet_rows(a3[g][r]);
                    red3[(wv * RB + 4 * (rg0 + r) + kq) * 32 + 16 * g + fm] = z;
                }
            }
            SMX_LDS_BARRIER();
        }
        // ---- the head: one (row, action) pair per lane -----------------------------------------------------------------
        if (hr < nrows) {
            float mu;
            if (l3res) {
                float p8[RNWV];
#pragma unroll
                for (int w = 0; w < RNWV; ++w) p8[w] = red3[(w * RB + hr) * 32 + hj];
                float z = p8[0];
#pragma unroll
                for (int w = 1; w < RNWV; ++w) z += p8[w];
                mu = act_f(z + b3v, G.out_act);
            } else {
                mu = outs[hr * RLDO + hj];
            }
            s_act[hr * RMAX_A + hj] = gauss_act(mu, sd0, ev, noisy);
        }
        SMX_LDS_BARRIER();
        E.step(s_act, false, [](long) { return EvalNoRow{}; }, [](long, EvalNoRow, int, float, float) {},
               [&](long row, EvalNoRow, float rew) { ret.add(E, row, rew); });
        SMX_LDS_BARRIER();
    }
    if constexpr (SETS) ret.store(E, G.ev.returns + (size_t)blockIdx.y * (size_t)G.n);
    else ret.store(E, G.ev.returns);
}

// DDPG: ddpg_rollout_kernel's step in a deterministic agent mode (tanh, clip; SMX_DDPG_NOISE_NONE) without a record
template <int RG, int NT, int TASK, bool SETS = false>
__global__ __launch_bounds__(RNTH) void ddpg_eval_kernel(DEvalKernelArgs<SETS> G) {
    constexpr int RB = 4 * RG;
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int A = G.A;
    const float* outs = sm + G.off_out;
    float* s_act = sm + G.off_act;                   // [RB][RMAX_A] the actions of this step (unused columns stay 0)

    clear_tiles(G, sm, tid, nullptr, nullptr, nullptr, 0.f);
    EnvLanes<RB, true, TASK> E(G, sm, nullptr, wv, lane, OwnStart{});
    if constexpr (TASK != SMX_TASK_DRIFT) {
        E.begin(eval_rst_arg<DEvalKernelArgs<SETS>>(), 0, G.ev.E);      // (done is false at every step)
        eval_start(E, G.ev, G.ev.rst.enabled != 0);
    } else {
        eval_start(E, G.ev, false);
    }
    SMX_LDS_BARRIER();
    E.start();
    const int hr = tid / A, hj = tid - hr * A;       // RB x A <= 512 pairs
    const bool head = hr < E.nrows;
    const size_t shift = eval_set_shift<SETS>(G);    // (SETS) floats to the workgroup's set
    SMX_LDS_BARRIER();
    EvalReturns ret;
#pragma unroll 1
    for (int step = 0; step < G.steps; ++step) {
        layers4<RG, NT>(G, sm, 3, SMX_ACT_TANH, wv, lane, [](int) {}, 0, G.D, PreLayer{}, shift);
        if (head) s_act[hr * RMAX_A + hj] = clip1(clip1(outs[hr * RLDO + hj]));      // (explore() without noise)
        SMX_LDS_BARRIER();
        E.step(s_act, false, [](long) { return EvalNoRow{}; }, [](long, EvalNoRow, int, float, float) {},
               [&](long row, EvalNoRow, float rew) { ret.add(E, row, rew); });
        SMX_LDS_BARRIER();
    }
    if constexpr (SETS) ret.store(E, G.ev.returns + (size_t)blockIdx.y * (size_t)G.n);
    else ret.store(E, G.ev.returns);
}

// The one-step body both step kernels share, in two phases with a barrier between them.  Phase 1, lane = action j < A
// of actor a: exploration, the open transition's action, the closing transition's (ring row `row`); the actions go to
// s_act_w.  Phase 2, one wavefront: the environment step, the open observation and reward, the closing transition's
// observations, reward and done; the actor's state advances (reset on done) -> element 0 of the next state before the
// reset (lane 0; the terminal one on done).
__device__ __forceinline__ void ddpg_step_act(const DArgs& G, const float* mu, long long ld_mu, long a, int lane,
                                              long long row, float* s_act_w) {
    const int A = G.A, N = G.N, tau = G.t0;
    const bool emit = tau >= N - 1;
    const int slot = tau % N, jslot = (tau + 1) % N;   // (transition j = tau - N + 1 sits in slot j % N)
    double x = 0.0, sig = 0.0;
    if (G.noise != SMX_DDPG_NOISE_NONE) sig = G.sigmas[a];
    if (G.noise == SMX_DDPG_NOISE_OU) x = G.ou[a * A + lane];
    const float e = noise_on(G.eps, G.nstream) ? noise_pick(G.eps, a * A + lane, G.nstream, a, 0, lane) : 0.f;
    const float v = explore(mu[a * ld_mu + lane], G.noise, e, sig, G.theta, G.dt, G.root_dt, tau, x);
    if (G.noise == SMX_DDPG_NOISE_OU) G.ou[a * A + lane] = x;
    s_act_w[lane] = v;
    float* ca = G.cact + (size_t)a * N * A + lane;
    ca[(size_t)slot * A] = v;
    if (emit) G.act[row * A + lane] = ca[(size_t)jslot * A];
}

__device__ __forceinline__ float ddpg_step_env(const DArgs& G, long a, int lane, long long row, const float* s_act_w) {
    const int D = G.D, A = G.A, N = G.N, tau = G.t0;
    const bool emit = tau >= N - 1;
    const int slot = tau % N, jslot = (tau + 1) % N;
    const bool done = (tau + 1 >= G.episode_len);
    float* co = G.cobs + (size_t)a * N * D;
    float sn0 = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float s = G.state[a * D + k];
        const float sn = synth_next(s, s_act_w[k % A], synth_drift(k));
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
            const double v = (double)s_act_w[j];
            q += v * v;
        }
        float* cr = G.crew + (size_t)a * N;
        const float rew = synth_reward(q, sn0);
        cr[slot] = rew;
        if (emit) {
            G.rew[row] = nstep_reward(cr, G.gpow, N, tau);
            G.done[row] = done ? 1.0f : 0.0f;
        }
        if (G.mon.ep_reward) episode_account(G.mon, a, rew, done);
    }
    return sn0;
}

// one step for four actors per workgroup, one wavefront each, given mu [n, A] (ld_mu)
constexpr int SA_MAX = 64;
__global__ __launch_bounds__(256) void ddpg_step_kernel(DArgs G, const float* mu, long long ld_mu) {
    __shared__ float s_act[4][SA_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long a = (long)blockIdx.x * 4 + w;
    const bool live = a < G.n;
    const long long row = (live && G.t0 >= G.N - 1) ? ring_row(G, 0, a) : 0;
    if (live && lane < G.A) ddpg_step_act(G, mu, ld_mu, a, lane, row, s_act[w]);
    __syncthreads();
    if (!live) return;
    ddpg_step_env(G, a, lane, row, s_act[w]);
}

// ---- DDPG with a camera: the step above plus the frames ------------------------------------------------------------
// Per actor a: a history of hist_len >= n_step + frame_stacks raw frames, the frame of episode step u (of the current
// episode) in slot (hist_pos - tau + u) mod hist_len; the step's new frame goes to slot (hist_pos + 1) mod hist_len.
// The stacked observation of step u is frames max(u - S + 1 + i, 0), i < S (stack_sources).  The frames this launch
// reads (steps tau - n_step - S + 2 .. tau) never sit in the slot it writes, so no workgroup reads what another writes.
//
// Grid (1 + X, n).  Workgroup (0, a) runs the step of actor a (wavefront 0), then renders the one frame that needs the
// next state -- step tau + 1's (the terminal frame on done) -- once, and stores it wherever it goes: the history (not on
// done), the last frame of the closing transition's pixel_next, the last frame of the next acting observation (not on
// done).  Workgroups (1 .. X, a) split the rest between them in units of U bytes (16: uint4 loads and stores; 1: frame
// sizes or buffers not on 16 bytes): the history copies and, on done, the new episode's first frame (rendered from
// init_state, which no workgroup writes).
struct PArgs {
    int C, H, W, S, hist_len, hist_pos, X;
    long long F;                               // C H W bytes per frame
    unsigned char *hist, *pix, *pix_next, *obs_pix;
};

// U bytes of frame (t, s0) from byte e0 (e0 + U <= C H W) into b
template <int U>
__device__ __forceinline__ void render_unit(const PArgs& P, long long e0, int shift, unsigned char* b) {
    const int HW = P.H * P.W;
    int c = (int)(e0 / HW);
    const int r = (int)(e0 - (long long)c * HW);
    int y = r / P.W, x = r - y * P.W;
#pragma unroll
    for (int i = 0; i < U; ++i) {
        b[i] = synth_frame_px(c, y, x, shift);
        if (++x == P.W) {
            x = 0;
            if (++y == P.H) { y = 0; ++c; }
        }
    }
}

#include "smx_frame_unit.inc.h"                         // store_unit / load_unit, shared with smx_record.hip

// The frame half of both camera step kernels.  An actor's frames at step tau:
struct FrameCtx {
    long long F, SF, nu;                       // bytes per frame, per stacked observation; units of U bytes per frame
    unsigned char *hist_a, *hnew;              // the actor's history; its slot for the frame of step tau + 1
    int tau;
    bool done;
};

template <int U>
__device__ __forceinline__ FrameCtx frame_ctx(const PArgs& P, long a, int tau, bool done) {
    FrameCtx C;
    C.F = P.F; C.SF = (long long)P.S * P.F; C.nu = P.F / U;
    C.hist_a = P.hist + (size_t)a * P.hist_len * P.F;
    C.hnew = C.hist_a + (size_t)((P.hist_pos + 1) % P.hist_len) * P.F;
    C.tau = tau; C.done = done;
    return C;
}

// workgroup 0's tail: frame tau + 1 from the next state (sn0), rendered once and stored wherever it goes: the history
// and the next acting observation's last frame (not on done), at a closing step pixel_next's last frame of ring row `row`
template <int U>
__device__ __forceinline__ void render_next_frame(const PArgs& P, const FrameCtx& C, long a, float sn0, bool closing,
                                                  long long row) {
    const int shift = synth_frame_shift(C.tau + 1, sn0);
    const size_t last = (size_t)(P.S - 1) * C.F;
    unsigned char* d0 = C.done ? nullptr : C.hnew;
    unsigned char* d1 = closing ? P.pix_next + (size_t)row * C.SF + last : nullptr;
    unsigned char* d2 = C.done ? nullptr : P.obs_pix + (size_t)a * C.SF + last;
    alignas(16) unsigned char b[U];
    for (long long v = threadIdx.x; v < C.nu; v += 256) {
        render_unit<U>(P, v * U, shift, b);
        if (d0) store_unit<U>(d0 + v * U, b);
        if (d1) store_unit<U>(d1 + v * U, b);
        if (d2) store_unit<U>(d2 + v * U, b);
    }
}

// the copy workgroups (blockIdx.x >= 1): item q < nq is one destination frame
//   done:     q < 1 + S: the new episode's first frame (rendered from s0 = init_state[a][0]) -> history (q = 0), acting
//             observation frame q - 1
//   not done: q < S - 1: acting observation frame q <- history, step tau + 2 - S + q
//   then at a closing step the kernel's npix items -- pixel(i, dst, u): destination and source step of item i -- and
//   S - 1 items: pixel_next frame i of ring row `row` <- step tau + 2 - S + i                  (steps < 0: step 0)
template <int U, typename Pixel>
__device__ __forceinline__ void copy_frames(const PArgs& P, const FrameCtx& C, long a, float s0, bool closing,
                                            long long row, int npix, Pixel pixel) {
    const int S = P.S, tau = C.tau, Hd = P.hist_len;
    const long long F = C.F, SF = C.SF, nu = C.nu;
    const int nfirst = C.done ? 1 + S : S - 1;
    const int nq = nfirst + (closing ? npix + S - 1 : 0);
    const int shift0 = synth_frame_shift(0, s0);
    const long long total = (long long)nq * nu, stride = (long long)P.X * 256;
    alignas(16) unsigned char b[U];
    for (long long g = (long long)(blockIdx.x - 1) * 256 + threadIdx.x; g < total; g += stride) {
        const int q = (int)(g / nu);
        const long long e = (g - (long long)q * nu) * U;
        unsigned char* dst;
        int u = 0;                                   // the source step (unless first: the new episode's first frame)
        const bool first = C.done && q < nfirst;
        if (q < nfirst) {
            if (C.done) dst = q == 0 ? C.hnew : P.obs_pix + (size_t)a * SF + (size_t)(q - 1) * F;
            else { dst = P.obs_pix + (size_t)a * SF + (size_t)q * F; u = tau + 2 - S + q; }
        } else if (q < nfirst + npix) {
            pixel(q - nfirst, dst, u);
        } else {
            const int i = q - nfirst - npix;
            dst = P.pix_next + (size_t)row * SF + (size_t)i * F;
            u = tau + 2 - S + i;
        }
        if (first) {
            render_unit<U>(P, e, shift0, b);
        } else {
            u = u < 0 ? 0 : u;
            const int hs = ((P.hist_pos - tau + u) % Hd + Hd) % Hd;
            load_unit<U>(C.hist_a + (size_t)hs * F + e, b);
        }
        store_unit<U>(dst + e, b);
    }
}

template <int U>
__global__ __launch_bounds__(256) void ddpg_pixel_step_kernel(DArgs G, PArgs P, const float* mu, long long ld_mu) {
    __shared__ float s_act[SA_MAX];
    __shared__ float s_sn0;
    const int tid = threadIdx.x, lane = tid & 63;
    const long a = blockIdx.y;
    const int N = G.N, S = P.S, tau = G.t0;
    const bool emit = tau >= N - 1;
    const long long row = emit ? ring_row(G, 0, a) : 0;
    const FrameCtx C = frame_ctx<U>(P, a, tau, tau + 1 >= G.episode_len);
    if (blockIdx.x == 0) {
        // ---- the low-dimensional step, then frame tau + 1 from the next state ----------------------------------
        if (tid < 64 && lane < G.A) ddpg_step_act(G, mu, ld_mu, a, lane, row, s_act);
        __syncthreads();
        if (tid < 64) {
            const float sn0 = ddpg_step_env(G, a, lane, row, s_act);
            if (lane == 0) s_sn0 = sn0;
        }
        __syncthreads();
        render_next_frame<U>(P, C, a, s_sn0, emit, row);
        return;
    }
    // the closing transition j's S items: pixel frame i <- step j - S + 1 + i
    const int j = tau - N + 1;
    copy_frames<U>(P, C, a, G.init_state[(size_t)a * G.D], emit, row, S, [&](int i, unsigned char*& dst, int& u) {
        dst = P.pix + (size_t)row * C.SF + (size_t)i * C.F;
        u = j - S + 1 + i;
    });
}

// ---- DDPG with a camera, frame-pool layout: every frame stored once --------------------------------------------------
// Per actor a pool of P.hist_len = Pl raw frames (PArgs' hist), the frame with counter i in slot i mod Pl.  f = the
// counter of the current step's frame, first = that of the episode's reset frame: the frame of episode step u has counter
// first + u, and the stacked observation under a newest counter `top` is frames max(top - S + 1 + i, first), i < S
// (stack_sources' rule, counters for steps).  A ring row holds two counters where the stacked layout holds 2 S frames.
//
// Grid (1 + X, n).  Workgroup (0, a) runs the step of actor a, renders frame f + 1 from the next state -- the terminal
// one on done -- once into the pool and (not on done) the last frame of the next acting observation; at a closing step it
// writes the row's frame_next = f + 1, frame_first = first and its actor.  Workgroups (1 .. X, a) build the rest of the
// acting observation: its older frames out of the pool (counters f + 2 - S .. f), or on done the new episode's first
// frame (counter f + 2, rendered from init_state) into the pool and S times into the observation.  The counters read,
// f + 2 - S .. f, and the two written, f + 1 and f + 2, are S + 1 consecutive ones: distinct slots with Pl >= S + 2.
struct PoolArgs {
    long long f, first;
    int64_t *frame_next, *frame_first;
    int* frame_actor;
};

__device__ __forceinline__ unsigned char* pool_slot(const PArgs& P, long a, long long counter) {
    const long long Pl = P.hist_len;
    return P.hist + ((size_t)a * Pl + (size_t)(((counter % Pl) + Pl) % Pl)) * P.F;
}

template <int U>
__global__ __launch_bounds__(256) void ddpg_pixel_pool_step_kernel(DArgs G, PArgs P, PoolArgs Q, const float* mu,
                                                                   long long ld_mu) {
    __shared__ float s_act[SA_MAX];
    __shared__ float s_sn0;
    const int tid = threadIdx.x, lane = tid & 63;
    const long a = blockIdx.y;
    const int S = P.S, tau = G.t0;
    const bool emit = tau >= G.N - 1, done = tau + 1 >= G.episode_len;
    const long long row = emit ? ring_row(G, 0, a) : 0;
    const long long F = P.F, nu = F / U;
    unsigned char* obs_a = P.obs_pix + (size_t)a * S * F;
    alignas(16) unsigned char b[U];
    if (blockIdx.x == 0) {
        if (tid < 64 && lane < G.A) ddpg_step_act(G, mu, ld_mu, a, lane, row, s_act);
        __syncthreads();
        if (tid < 64) {
            const float sn0 = ddpg_step_env(G, a, lane, row, s_act);
            if (lane == 0) s_sn0 = sn0;
        }
        if (emit && tid == 64) {
            Q.frame_next[row] = Q.f + 1;
            Q.frame_first[row] = Q.first;
            Q.frame_actor[row] = (int)a;
        }
        __syncthreads();
        const int shift = synth_frame_shift(tau + 1, s_sn0);
        unsigned char* d0 = pool_slot(P, a, Q.f + 1);
        unsigned char* d1 = done ? nullptr : obs_a + (size_t)(S - 1) * F;
        for (long long v = tid; v < nu; v += 256) {
            render_unit<U>(P, v * U, shift, b);
            store_unit<U>(d0 + v * U, b);
            if (d1) store_unit<U>(d1 + v * U, b);
        }
        return;
    }
    // item q: done: the new episode's first frame -> the pool (q = 0), observation frame q - 1; else observation frame q
    // <- counter max(f + 2 - S + q, first)
    const int nq = done ? 1 + S : S - 1;
    const int shift0 = synth_frame_shift(0, G.init_state[(size_t)a * G.D]);
    const long long total = (long long)nq * nu, stride = (long long)P.X * 256;
    for (long long g = (long long)(blockIdx.x - 1) * 256 + tid; g < total; g += stride) {
        const int q = (int)(g / nu);
        const long long e = (g - (long long)q * nu) * U;
        unsigned char* dst;
        if (done) {
            dst = q == 0 ? pool_slot(P, a, Q.f + 2) : obs_a + (size_t)(q - 1) * F;
            render_unit<U>(P, e, shift0, b);
        } else {
            dst = obs_a + (size_t)q * F;
            const long long c = Q.f + 2 - S + q;
            load_unit<U>(pool_slot(P, a, c < Q.first ? Q.first : c) + e, b);
        }
        store_unit<U>(dst + e, b);
    }
}

// ---- PPO with a camera: one step of the moving windows plus the frames ---------------------------------------------
// The record launch of the per-step camera path (the CNN perception, the LSTM step and the actor's layers run between
// two of them): the sampling head, the environment step, WinArgs' carry rings and -- at a closing step -- the window
// into its FIFO row W.cursor + a, as ppo_rollout<WIN> does them; the frames as ddpg_pixel_step_kernel does, with the
// same history (slot rule and proof above PArgs: a closing window reads the frames of steps tau - N - S + 2 .. tau, the
// launch writes the slot of step tau + 1 - hist_len <= tau - N - S + 1).
//
// Grid (1 + X, n).  Workgroup (0, a): thread j < A owns action j (head, rings, the window's actions and pds), then
// thread k owns state element k (+ 256 i), thread 0 the reward and thread j < Hl the cell pair j -- every ring value
// is written and read back by the same thread; then all render frame tau + 1 from the next state (the terminal frame
// on done).  Workgroups (1 .. X, a) split the other destination frames in units of U bytes: the next acting
// observation's older frames (on done: the new episode's first frame, rendered from init_state), and at a closing
// step the window's N S stacked frames and pixel_next's S - 1 older ones.
struct PWArgs {
    int n, D, A, Hl, t0, episode_len;
    const float *log_var, *noise_scale, *eps;
    smx_noise_stream nstream;                  // eps null and nstream.enabled: the draws are formed here (noise_draw)
    float* state;
    const float* init_state;
    const float *h_before, *c_before;          // [n, Hl] the LSTM state before this step, or null
    WinArgs W;                                 // (W.cursor: the row of actor 0 at this step)
    smx_episode_monitor mon;                   // mon.ep_reward null: none
};

template <int U>
__global__ __launch_bounds__(256) void ppo_pixel_window_step_kernel(PWArgs G, PArgs P, const float* mu, long long ld_mu) {
    __shared__ float s_act[SA_MAX];
    __shared__ float s_sn0;
    const WinArgs& W = G.W;
    const int tid = threadIdx.x;
    const long a = blockIdx.y;
    const int N = W.N, S = P.S, tau = G.t0, D = G.D, A = G.A;
    const int j = tau + 1 - N;                       // the window that ends with this step, if one starts there
    const bool wclose = j >= 0 && j % W.adv == 0, done = (tau + 1 >= G.episode_len);
    const int wslot = tau % N, wfirst = (tau + 1) % N;
    const long long row = wclose ? win_row(W, W.cursor, a) : 0;
    const FrameCtx C = frame_ctx<U>(P, a, tau, done);
    if (blockIdx.x == 0) {
        // ---- the sampling head (smx_diaggauss_sample_f32's expressions): one action per thread ----------------------
        if (tid < A) {
            const float m = mu[a * ld_mu + tid];
            float sd = expf(G.log_var[tid]);
            if (G.noise_scale) sd = sd * G.noise_scale[a];
            const float act =
                clip1(noise_on(G.eps, G.nstream) ? noise_pick(G.eps, a * A + tid, G.nstream, a, 0, tid) * sd + m : m);
            s_act[tid] = act;
            float* ca = W.cact + (size_t)a * N * A + tid;
            float* cp = W.cpd + (size_t)a * N * 2 * A + tid;
            ca[(size_t)wslot * A] = act;
            cp[(size_t)wslot * 2 * A] = m;
            cp[(size_t)wslot * 2 * A + A] = sd;
            if (wclose) {
                float* da = W.act + (row * N) * A + tid;
                float* dp = W.pd + (row * N) * 2 * A + tid;
                copy_window<8, 3>(N, wfirst,
                    [&](int s, int c) { return c == 0 ? ca[(size_t)s * A] : cp[(size_t)s * 2 * A + (c - 1) * A]; },
                    [&](int u, int c, float v) {
                        if (c == 0) da[(size_t)u * A] = v;
                        else dp[(size_t)u * 2 * A + (c - 1) * A] = v;
                    });
            }
        }
        __syncthreads();
        // ---- the environment step (smx_synth_env_step_f32's expressions), the rings, the closing window -------------
        float* co = W.cobs + (size_t)a * N * D;
        float sn0 = 0.f;
        for (int k = tid; k < D; k += 256) {
            const float s = G.state[a * D + k];
            const float sn = synth_next(s, s_act[k % A], synth_drift(k));
            co[(size_t)wslot * D + k] = s;
            if (wclose) {
                W.obs_next[row * D + k] = sn;
                float* dst = W.obs + row * N * D + k;
                copy_window<8, 1>(N, wfirst, [&](int s_, int) { return co[(size_t)s_ * D + k]; },
                                  [&](int u, int, float v) { dst[(size_t)u * D] = v; });
            }
            if (k == 0) sn0 = sn;
            G.state[a * D + k] = done ? G.init_state[a * D + k] : sn;
        }
        if (tid == 0) {
            double q = 0.0;
            for (int c = 0; c < A; ++c) {
                const double v = (double)s_act[c];
                q += v * v;
            }
            float* cr = W.crew + (size_t)a * N;
            const float rew = synth_reward(q, sn0);
            cr[wslot] = rew;
            if (wclose) {
                float* dr = W.rew + row * N;
                float* dd = W.done + row * N;
                copy_window<8, 1>(N, wfirst, [&](int s_, int) { return cr[s_]; },
                                  [&](int u, int, float v) {
                                      dr[u] = v;
                                      dd[u] = (done && u == N - 1) ? 1.0f : 0.0f;
                                  });
            }
            if (G.mon.ep_reward) episode_account(G.mon, a, rew, done);
            s_sn0 = sn0;
        }
        if (W.ccell) {
            const int Hl = G.Hl;
            float* cc = W.ccell + (size_t)a * W.S * 2 * Hl;
            for (int c = tid; c < Hl; c += 256) {
                if (G.h_before && tau % W.adv == 0) {
                    float* cw = cc + (size_t)((tau / W.adv) % W.S) * 2 * Hl + c;
                    cw[0] = G.h_before[a * Hl + c];
                    cw[Hl] = G.c_before[a * Hl + c];
                }
                if (wclose && W.cells) {
                    const float* cr = cc + (size_t)((j / W.adv) % W.S) * 2 * Hl + c;
                    float* d = W.cells + row * 2 * Hl + c;
                    d[0] = cr[0];
                    d[Hl] = cr[Hl];
                }
            }
        }
        __syncthreads();
        // ---- frame tau + 1 from the next state, once, to wherever it goes -----------------------------------------
        render_next_frame<U>(P, C, a, s_sn0, wclose, row);
        return;
    }
    // the closing window's N S items: frame i % S of window step i / S <- step j + i / S - S + 1 + i % S
    copy_frames<U>(P, C, a, G.init_state[(size_t)a * D], wclose, row, N * S, [&](int i, unsigned char*& dst, int& u) {
        dst = P.pix + (size_t)row * N * C.SF + (size_t)i * C.F;
        u = j + i / S - S + 1 + i % S;
    });
}

// ---- host side -------------------------------------------------------------------------------------------------------

inline int rr64(int v) { return (v + 63) & ~63; }

// The LDS layout of an RB-actor block: x | h1 | h2 | out | actions [RB][RMAX_A] | the split output layer's partial sums
// [RNWV][RB][32] (split_out) | the z-filter's mean and std [2][D] (ztables) | k % A [D].  Everything before the z tables
// is cleared at the start.
// Row strides on the 4-row loop = 16 mod 64 words: the rows of a group (a word's lanes: row l & 3, k offset 8 (l >> 4)) and
// the epilogue's one-word stores (row kq, feature fm) fall on distinct banks of the 64.  A tile holds pack_chunks(K) * 32
// + 8 columns at least (the loop's last prefetch reads one chunk it does not use).  On the 16x16x4 loop (mma16) a word's
// lanes are row l & 15: strides of 4 mod 64 spread them.  xcols: the columns of the x tile its readers take as K (D;
// the LSTM rollout's [x | 0 | h] row: Dp + rr64(H), so that the actor's first layer, reading from column Dp, stays
// inside the row too).
int carve(RollBase& G, int RB, bool mma16, bool split_out, bool ztables, int xcols) {
    if (mma16) { G.ldx = rr64(xcols) + 4; G.ldh1 = rr64(G.H1) + 4; G.ldh2 = rr64(G.H2) + 4; }
    else { G.ldx = rr64(xcols + 40) + 16; G.ldh1 = rr64(G.H1 + 40) + 16; G.ldh2 = rr64(G.H2 + 40) + 16; }
    G.off_h1 = RB * G.ldx;
    G.off_h2 = G.off_h1 + RB * G.ldh1;
    G.off_out = G.off_h2 + RB * G.ldh2;
    G.off_act = G.off_out + RB * RLDO;
    G.off_red3 = G.off_act + RB * RMAX_A;
    G.off_z = G.off_red3 + (split_out ? RNWV * RB * 32 : 0);
    G.off_kmod = G.off_z + (ztables ? 2 * G.D : 0);
    return (G.off_kmod + G.D) * (int)sizeof(float);
}

// the shapes a persistent kernel takes: A <= 32, H1 and H2 multiples of 4 up to 640, D <= 512, and the 16-actor block's
// layout within the LDS limit
int32_t supported(int32_t D, int32_t H1, int32_t H2, int32_t A, bool mma16, bool split_out, bool ztables) {
    if (!(D > 0 && H1 > 0 && H2 > 0 && A > 0 && A <= RMAX_A && H1 % 4 == 0 && H2 % 4 == 0)) return 0;
    if (!(H1 <= 640 && H2 <= 640 && D <= 64 * RKV)) return 0;
    RollBase G;
    memset(&G, 0, sizeof(G));
    G.D = D; G.H1 = H1; G.H2 = H2; G.A = A;
    return carve(G, 16, mma16, split_out, ztables, D) <= ROLL_MAX_LDS;
}

// The LayerNorm rollouts keep ln1.W | ln1.b | ln2.W | ln2.b behind the layout of `lds` bytes -> the bytes with them
int carve_ln(const RollBase& G, LnTail& ln, int lds) {
    ln.off = lds / (int)sizeof(float);
    return lds + 2 * (G.H1 + G.H2) * (int)sizeof(float);
}

// With a monitor the open episodes of the block's rb actors follow the layout of `lds` bytes: [rb] fp64 sums on 8 bytes,
// then [rb] int32 step counts -> the bytes with them (without one: `lds` as it is, and the kernels never read off_ep)
constexpr int ROLL_EP_LDS = 8 + 16 * 12;         // (what 16 actors add at most: launch()'s dynamic-LDS limit has it)
int carve_episodes(RollBase& G, int rb, int lds) {
    if (!G.mon.ep_reward) return lds;
    G.off_ep = ((lds + 7) & ~7) / (int)sizeof(float);
    return G.off_ep * (int)sizeof(float) + rb * 12;
}

// With per-actor clocks the block's [rb][3] ints (ClkArgs) follow the layout of `lds` bytes -> the bytes with them
constexpr int ROLL_CLK_LDS = 16 * 12;            // (what 16 actors add: launch()'s dynamic-LDS limit has it)
int carve_clocks(ClkArgs& C, int rb, int lds) {
    C.off = (lds + 3) / (int)sizeof(float);
    return C.off * (int)sizeof(float) + rb * 12;
}

// ---- LSTM stem ---------------------------------------------------------------------------------------------------

__host__ __device__ inline int lstm_dp(int D) { return (D + 3) & ~3; }

// The LSTM rollout's LDS: carve()'s layout with the x tile widened to [x | 0 | h], then the gate tile [RB][ldg]
// (rewritten whole by every gate pass: not cleared) and the cells [RB H] (pair q = r H + j: written and read by thread
// q mod RNTH alone)
template <typename LstmArgs>
int carve_lstm(LstmArgs& G, int RB) {
    G.Dp = lstm_dp(G.D);
    carve(G, RB, /*mma16=*/false, /*split_out=*/true, /*ztables=*/true, G.Dp + rr64(G.H));
    G.off_g = (G.off_kmod + G.D + 3) & ~3;
    G.ldg = rr64(4 * G.H) + 16;
    G.off_c = G.off_g + RB * G.ldg;
    return (G.off_c + RB * G.H) * (int)sizeof(float);
}

// the gate pass's packed weights: [4H, Dp + H] = [W_ih | 0 | W_hh] in fragment order (smx_epoch_pack.inc.h), then
// b_ih + b_hh [4H]
long lstm_pack_floats(int D, int H) { return pack_words(4 * H, lstm_dp(D) + H) * 4 + 4 * (long)H; }

__global__ void lstm_pack_kernel(smx_lstm_t net, float* packed) {
    const int D = net.D, H = net.H, Dp = lstm_dp(D), K = Dp + H, C = pack_chunks(K);
    const long nw = pack_words(4 * H, K) * 4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < nw + 4 * H; idx += (long)gridDim.x * blockDim.x) {
        if (idx >= nw) {
            const int m = (int)(idx - nw);
            packed[idx] = net.b_ih[m] + net.b_hh[m];
            continue;
        }
        // float idx = (((t C + c) 2 + h) 64 + 16 kq + i) 4 + e holds X[16 t + i][32 c + 8 kq + 4 h + e] (pack_pos)
        const int e = (int)(idx & 3), i = (int)((idx >> 2) & 15), kq = (int)((idx >> 6) & 3), h = (int)((idx >> 8) & 1);
        const long tc = idx >> 9;
        const int c = (int)(tc % C), t = (int)(tc / C);
        const int m = 16 * t + i, k = 32 * c + 8 * kq + 4 * h + e;
        float v = 0.f;
        if (m < 4 * H) {
            if (k < D) v = net.W_ih[(long)m * D + k];
            else if (k >= Dp && k < K) v = net.W_hh[(long)m * H + (k - Dp)];
        }
        packed[idx] = v;
    }
}

// actors per workgroup: `forced` (4 | 8 | 16), or for 0 the smallest of 4 and 8 whose grid fits the chip once, else 16
int pick_block(int forced, int n) {
    if (forced) return forced;
    for (int c = 4; c <= 8; c *= 2)
        if ((n + c - 1) / c <= smx_cu_count()) return c;
    return 16;
}

// the same for a population whose agents span apa actors (a multiple of 4): a block never spans two agents, so its size
// divides apa -- the automatic choice steps down from pick_block's until it does; a forced size that does not: 0
int pick_population_block(int forced, int n, int apa) {
    int c = pick_block(forced, n);
    if (forced) return apa % c == 0 ? c : 0;
    while (apa % c) c /= 2;
    return c;
}

// one workgroup of RNTH lanes per rb actors, with LDS for one workgroup per CU; each kernel's dynamic-LDS limit is raised
// at its first launch
// (arguments that end with clocks, WithClk: their LDS follows the episodes')
template <typename Args>
constexpr bool has_clocks = false;
template <typename Base>
constexpr bool has_clocks<WithClk<Base>> = true;

// (sets: the grid's second dimension -- the evaluation of several parameter sets, one row of workgroups a set)
template <auto K, typename Args>
int launch(const Args& G, int rb, int lds, smx_stream_t stream, int sets = 1) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       ROLL_MAX_LDS + ROLL_EP_LDS + (has_clocks<Args> ? ROLL_CLK_LDS : 0));
    (void)attr;
    Args A = G;
    lds = carve_episodes(A, rb, lds);
    if constexpr (has_clocks<Args>) lds = carve_clocks(A.clk, rb, lds);
    if (lds < ROLL_EXCLUSIVE_LDS) lds = ROLL_EXCLUSIVE_LDS;
    hipLaunchKernelGGL(K, dim3((A.n + rb - 1) / rb, sets), dim3(RNTH), lds, smx_s(stream), A);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

// the same for a block of rb = 4 | 8 | 16 actors: each has its own instantiation
template <auto K4, auto K8, auto K16, typename Args>
int launch(const Args& G, int rb, int lds, smx_stream_t stream, int sets = 1) {
    if (rb == 4) return launch<K4>(G, rb, lds, stream, sets);
    if (rb == 8) return launch<K8>(G, rb, lds, stream, sets);
    return launch<K16>(G, rb, lds, stream, sets);
}

// the task of a call as a compile-time constant: f(std::integral_constant<int, SMX_TASK_...>) (the callers have checked
// the id, synth_task_ok).  A later task is one case here, and its EnvLanes.
template <typename F>
int with_task(int task, F f) {
    switch (task) {
    case SMX_TASK_REACH: return f(std::integral_constant<int, SMX_TASK_REACH>{});
    case SMX_TASK_ARM: return f(std::integral_constant<int, SMX_TASK_ARM>{});
    default: return f(std::integral_constant<int, SMX_TASK_DRIFT>{});
    }
}

// a task kernel's arguments from its drift twin's and the reset stream (null: none)
template <typename Base>
WithRst<Base> with_resets(const Base& G, const smx_reset_stream* R) {
    WithRst<Base> X;
    memset(&X.rst, 0, sizeof(X.rst));
    static_cast<Base&>(X) = G;
    if (R) X.rst = *R;
    return X;
}

// a CLK kernel's arguments from its shared-clock twin's and the clocks
template <typename Base>
WithClk<Base> with_clocks(const Base& G, const ClkArgs& C) {
    WithClk<Base> X;
    static_cast<Base&>(X) = G;
    X.clk = C;
    return X;
}

// what both clocked entry points ask of the clocks -> the kernels' copy (its LDS offset: launch())
int clock_args(const smx_actor_clocks* c, long long capacity, ClkArgs& C) {
    SMX_REQUIRE(c && c->t && c->episode_len && c->row_off, SMX_E_NULL);
    SMX_REQUIRE(c->rows >= 0 && c->rows <= capacity, SMX_E_SHAPE);
    C.t = c->t; C.L = c->episode_len; C.row_off = c->row_off; C.rows = c->rows; C.off = 0;
    return SMX_OK;
}

// the fields both DDPG entry points take from the argument block
int common_args(const smx_ddpg_rollout_t* a, DArgs& G) {
    SMX_REQUIRE(a && a->state && a->init_state && a->gpow && a->carry_obs && a->carry_act && a->carry_rew, SMX_E_NULL);
    SMX_REQUIRE(a->obs && a->obs_next && a->actions && a->rewards && a->dones, SMX_E_NULL);
    SMX_REQUIRE(a->n > 0 && a->D > 0 && a->A > 0 && a->n_step > 0 && a->episode_len > 0 && a->t >= 0, SMX_E_SHAPE);
    SMX_REQUIRE(a->capacity > 0 && a->cursor >= 0 && a->cursor < a->capacity, SMX_E_SHAPE);
    SMX_REQUIRE(a->noise_type >= SMX_DDPG_NOISE_NONE && a->noise_type <= SMX_DDPG_NOISE_OU, SMX_E_SHAPE);
    SMX_REQUIRE(a->noise_type == SMX_DDPG_NOISE_NONE || (noise_on(a->eps, a->noise) && a->sigmas), SMX_E_NULL);
    SMX_REQUIRE(a->noise_type != SMX_DDPG_NOISE_OU || a->ou, SMX_E_NULL);
    SMX_REQUIRE(episode_pointers_ok(a->mon), SMX_E_NULL);
    SMX_REQUIRE(episode_shape_ok(a->mon) && noise_shape_ok(a->noise, a->n), SMX_E_SHAPE);
    memset(&G, 0, sizeof(G));
    G.mon = a->mon;
    G.D = a->D; G.A = a->A; G.n = a->n; G.steps = a->steps; G.t0 = a->t; G.episode_len = a->episode_len;
    G.N = a->n_step; G.noise = a->noise_type;
    G.eps = a->noise_type == SMX_DDPG_NOISE_NONE ? nullptr : a->eps;
    if (a->noise_type != SMX_DDPG_NOISE_NONE) G.nstream = a->noise;       // (NONE reads neither)
    G.sigmas = a->sigmas; G.theta = a->theta; G.dt = a->dt; G.root_dt = a->root_dt;
    G.gpow = a->gpow; G.ou = a->ou;
    G.state = a->state; G.init_state = a->init_state;
    G.cobs = a->carry_obs; G.cact = a->carry_act; G.crew = a->carry_rew;
    G.obs = a->obs; G.obs_next = a->obs_next; G.act = a->actions; G.rew = a->rewards; G.done = a->dones;
    G.cursor = a->cursor; G.capacity = a->capacity;
    return SMX_OK;
}

// the steps among `steps` steps from clock t whose clock `closes` accepts
template <typename Closes>
long long closing_steps(int t, int steps, int episode_len, Closes closes) {
    long long m = 0;
    for (int s = 0; s < steps; ++s) {
        if (closes(t)) ++m;
        t = (t + 1 >= episode_len) ? 0 : t + 1;
    }
    return m;
}

// a moving window (n_step N, advance adv) closes at clock t
inline bool window_closes(int t, int N, int adv) { return t + 1 >= N && (t + 1 - N) % adv == 0; }

// ---- the argument blocks -> the kernels' arguments -----------------------------------------------------------------

// the actor of every persistent kernel: the packed weights' three layers, the biases, the hidden widths
void net_fields(const smx_mlp3_t& n, const float* packed, RollBase& G) {
    G.P1 = packed;
    G.P2 = packed + 4 * pack_off(n.D, n.H1, n.H2, n.OUT, 1);
    G.P3 = packed + 4 * pack_off(n.D, n.H1, n.H2, n.OUT, 2);
    G.b1 = n.b1; G.b2 = n.b2; G.b3 = n.b3; G.H1 = n.H1; G.H2 = n.H2;
}

// every PPO kernel's network, shapes (D: the observation's width), head, z-filter, state and clock
void roll_fields(const smx_synth_rollout_t* a, int D, RollArgs& G) {
    net_fields(*a->net, a->packed, G);
    G.D = D; G.A = a->net->OUT; G.out_act = a->out_act;
    G.log_var = a->log_var; G.noise_scale = a->noise_scale; G.eps = a->eps;
    G.zsum = a->zsum; G.zsumsq = a->zsumsq; G.zcount = a->zcount; G.zeps = a->zeps;
    G.state = a->state; G.init_state = a->init_state;
    G.n = a->n; G.t0 = a->t; G.episode_len = a->episode_len; G.steps = a->steps;
    G.mon = a->mon;
    G.nstream = a->noise;
}

// the rollout tables (the windowed kernels have none)
void table_fields(const smx_synth_rollout_t* a, RollArgs& G) {
    G.R = a->rows_per_actor; G.slot0 = a->slot;
    G.obs_roll = a->obs_roll; G.act_roll = a->act_roll; G.rew_roll = a->rew_roll; G.done_roll = a->done_roll;
    G.pd_roll = a->pd_roll; G.obs_last = a->obs_last;
}

// the LSTM stem (cell_roll apart: the rollout tables' kernel alone records it)
void lstm_fields(const smx_synth_lstm_rollout& b, LArgs& G) {
    const smx_lstm_t& l = *b.lstm;
    G.H = l.H; G.Hl = b.hidden;
    G.Pg = b.lstm_packed; G.bg = b.lstm_packed + pack_words(4 * l.H, lstm_dp(l.D) + l.H) * 4;
    G.h0 = b.h0; G.c0 = b.c0; G.hN = b.hN; G.cN = b.cN; G.h_before = b.h_before; G.c_before = b.c_before;
}

// the moving windows of either windowed argument block
template <typename Block>
WinArgs win_fields(const Block& a) {
    WinArgs W;
    memset(&W, 0, sizeof(W));
    W.N = a.n_step; W.adv = a.advance; W.S = (W.N + W.adv - 1) / W.adv;
    W.cobs = a.carry_obs; W.cact = a.carry_act; W.crew = a.carry_rew; W.cpd = a.carry_pd; W.ccell = a.carry_cells;
    W.obs = a.obs; W.obs_next = a.obs_next; W.act = a.actions; W.rew = a.rewards; W.done = a.dones; W.pd = a.pds;
    W.cells = a.cells; W.cursor = a.cursor; W.capacity = a.capacity;
    return W;
}

// the camera of either step argument block, with X copy workgroups per actor: ~32 KB each of `frames` destination frames
template <typename Block>
PArgs pixel_fields(const Block& a, long long frames) {
    PArgs P;
    memset(&P, 0, sizeof(P));
    P.C = a.C; P.H = a.H; P.W = a.W; P.S = a.frame_stacks; P.hist_len = a.hist_len; P.hist_pos = a.hist_pos;
    P.F = (long long)a.C * a.H * a.W;
    P.hist = a.hist; P.pix = a.pixel; P.pix_next = a.pixel_next; P.obs_pix = a.obs_pixel;
    const long long X = (frames * P.F + 32767) / 32768;
    P.X = (int)(X < 1 ? 1 : (X > 64 ? 64 : X));
    return P;
}

// a camera step kernel on the grid (1 + X, n): K16 copies 16 bytes a lane where the frame size and every frame buffer
// allow it, else K1 single bytes
template <auto K16, auto K1, typename Args>
int launch_pixel(const Args& G, const PArgs& P, int n, const float* mu, int64_t ld_mu, smx_stream_t stream) {
    const bool vec = P.F % 16 == 0 && (((uintptr_t)P.hist | (uintptr_t)P.pix | (uintptr_t)P.pix_next |
                                        (uintptr_t)P.obs_pix) & 15) == 0;
    hipLaunchKernelGGL(vec ? K16 : K1, dim3(1 + P.X, n), dim3(256), 0, smx_s(stream), G, P, mu, (long long)ld_mu);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

// ---- the rules the entry points share (the SMX_REQUIRE at the call names the code) ---------------------------------

bool block_ok(int apw) { return apw == 0 || apw == 4 || apw == 8 || apw == 16; }      // actors_per_workgroup
bool roll_pointers(const smx_synth_rollout_t* a) {
    return a->net && a->packed && a->log_var && a->state && a->init_state && episode_pointers_ok(a->mon);
}
// the z-filter's running sums: all three or none
bool zfilter_ok(const smx_synth_rollout_t* a) {
    return (a->zsum == nullptr) == (a->zsumsq == nullptr) && (a->zsum == nullptr) == (a->zcount == nullptr);
}
// the packed weights on 16 bytes (lstm_packed: null where there is no stem), the biases on 4
bool aligned_ok(const float* packed, const float* b1, const float* lstm_packed) {
    return (((uintptr_t)packed | (uintptr_t)lstm_packed) & 15) == 0 && ((uintptr_t)b1 & 3) == 0;
}
// sizes, block size, and slot + steps within the tables' rows whenever one of them (`cells`: the LSTM's) is recorded:
// every roll table is indexed by slot + step, so the bound holds whichever of them is
bool rollout_shape_ok(const smx_synth_rollout_t* a, const void* cells) {
    const bool records = a->obs_roll || a->act_roll || a->rew_roll || a->done_roll || a->pd_roll || cells;
    return a->n > 0 && a->steps > 0 && a->episode_len > 0 && a->rows_per_actor > 0 && block_ok(a->actors_per_workgroup) &&
           a->slot >= 0 && (!records || a->slot + a->steps <= a->rows_per_actor) && episode_shape_ok(a->mon) &&
           noise_shape_ok(a->noise, a->n);
}
bool cell_pairs_ok(const float* h0, const float* c0, const float* h_before, const float* c_before) {
    return (h_before == nullptr) == (c_before == nullptr) && (h0 == nullptr) == (c0 == nullptr);
}
// the actor reads the stem's output; `hidden` logical units of the H padded ones (padding < 4)
bool lstm_shape_ok(const smx_mlp3_t& n, const smx_lstm_t& l, int hidden) {
    return n.D == l.H && hidden > 0 && hidden <= l.H && l.H - hidden < 4;
}
template <typename Block>
bool window_pointers(const Block& a) {
    return a.carry_obs && a.carry_act && a.carry_rew && a.carry_pd && a.obs && a.obs_next && a.actions && a.rewards &&
           a.dones && a.pds;
}
template <typename Block>
bool window_shape_ok(const Block& a) {
    return a.n_step > 0 && a.advance > 0 && a.advance <= a.n_step && a.capacity > 0 && a.cursor >= 0 && a.cursor < a.capacity;
}
// the frame buffers, the frame, and a history long enough that no launch reads the slot it writes (proof above PArgs)
template <typename Block>
bool pixel_pointers(const Block& a) { return a.hist && a.pixel && a.pixel_next && a.obs_pixel; }
template <typename Block>
bool pixel_shape_ok(const Block& a, int n_step) {
    return a.C > 0 && a.H > 0 && a.W > 0 && a.frame_stacks > 0 && a.hist_len >= n_step + a.frame_stacks &&
           a.hist_pos >= 0 && a.hist_pos < a.hist_len;
}
// what the step launches ask of mu [n, A] (ld_mu) and of the ring: one row per actor, all distinct
bool step_shape_ok(int n, int A, int64_t ld_mu, long long capacity) { return A <= SA_MAX && ld_mu >= A && n <= capacity; }

}  // namespace

#ifdef SMX_ROLLOUT_TIMING
// timing builds only (not declared in include/surreal_amd.h): where the timestamps go ([workgroups][16] int64)
extern "C" void smx_rollout_debug_tbuf(void* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rtbuf_dev), &p, sizeof(p)); }
#endif

extern "C" int32_t smx_synth_rollout_supported(int32_t D, int32_t H1, int32_t H2, int32_t A) {
    return supported(D, H1, H2, A, /*mma16=*/true, /*split_out=*/true, /*ztables=*/true);
}

extern "C" int smx_synth_rollout_f32(const smx_synth_rollout_t* a, smx_stream_t stream) {
    SMX_REQUIRE(a && roll_pointers(a), SMX_E_NULL);
    const smx_mlp3_t& n = *a->net;
    SMX_REQUIRE(smx_synth_rollout_supported(n.D, n.H1, n.H2, n.OUT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(rollout_shape_ok(a, nullptr), SMX_E_SHAPE);
    SMX_REQUIRE(aligned_ok(a->packed, n.b1, nullptr), SMX_E_ALIGN);
    SMX_REQUIRE(zfilter_ok(a), SMX_E_NULL);
    RollArgs G;
    memset(&G, 0, sizeof(G));
    roll_fields(a, n.D, G);
    table_fields(a, G);
    const int rb = pick_block(a->actors_per_workgroup, a->n);
    const int lds = carve(G, rb, /*mma16=*/rb == 16, /*split_out=*/true, /*ztables=*/true, G.D);
    return launch<rollout_kernel<1>, rollout_kernel<2>, rollout16_kernel>(G, rb, lds, stream);
}

extern "C" int32_t smx_synth_lstm_rollout_supported(int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A) {
    if (!(H > 0 && H % 4 == 0 && H <= 128)) return 0;
    if (!supported(D, H1, H2, A, /*mma16=*/false, /*split_out=*/true, /*ztables=*/true)) return 0;
    LArgs G;
    memset(&G, 0, sizeof(G));
    G.D = D; G.H = H; G.H1 = H1; G.H2 = H2; G.A = A;
    return carve_lstm(G, 16) <= ROLL_MAX_LDS;
}

extern "C" int64_t smx_lstm_rollout_packed_floats(int32_t D, int32_t H) {
    if (D <= 0 || H <= 0 || H % 4) return 0;
    return lstm_pack_floats(D, H);
}

extern "C" int smx_lstm_rollout_pack_f32(const smx_lstm_t* net, float* packed, smx_stream_t stream) {
    SMX_REQUIRE(net && net->W_ih && net->W_hh && net->b_ih && net->b_hh && packed, SMX_E_NULL);
    SMX_REQUIRE(net->D > 0 && net->H > 0 && net->H % 4 == 0, SMX_E_SHAPE);
    const long total = lstm_pack_floats(net->D, net->H);
    const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(blocks), dim3(256), 0, smx_s(stream), *net, packed);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_lstm_rollout_f32(const smx_synth_lstm_rollout* args, smx_stream_t stream) {
    SMX_REQUIRE(args && args->lstm && args->lstm_packed && args->hN && args->cN, SMX_E_NULL);
    const smx_synth_rollout_t* a = &args->roll;
    SMX_REQUIRE(roll_pointers(a), SMX_E_NULL);
    SMX_REQUIRE(cell_pairs_ok(args->h0, args->c0, args->h_before, args->c_before), SMX_E_NULL);
    const smx_mlp3_t& n = *a->net;
    const smx_lstm_t& l = *args->lstm;
    SMX_REQUIRE(lstm_shape_ok(n, l, args->hidden), SMX_E_SHAPE);
    SMX_REQUIRE(smx_synth_lstm_rollout_supported(l.D, l.H, n.H1, n.H2, n.OUT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(rollout_shape_ok(a, args->cell_roll), SMX_E_SHAPE);
    SMX_REQUIRE(aligned_ok(a->packed, n.b1, args->lstm_packed), SMX_E_ALIGN);
    SMX_REQUIRE(zfilter_ok(a), SMX_E_NULL);
    LArgs G;
    memset(&G, 0, sizeof(G));
    roll_fields(a, l.D, G);
    table_fields(a, G);
    lstm_fields(*args, G);
    G.cell_roll = args->cell_roll;
    const int rb = pick_block(a->actors_per_workgroup, a->n);
    const int lds = carve_lstm(G, rb);
    return launch<lstm_rollout_kernel<1>, lstm_rollout_kernel<2>, lstm_rollout_kernel<4>>(G, rb, lds, stream);
}

extern "C" int32_t smx_synth_ppo_window_rollout_supported(int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A) {
    if (H == 0) return supported(D, H1, H2, A, /*mma16=*/false, /*split_out=*/true, /*ztables=*/true);
    return smx_synth_lstm_rollout_supported(D, H, H1, H2, A);
}

// both windowed entry points; clocks: null (the shared clock of base.roll) or the actors' own
// task: SMX_TASK_DRIFT, or (shared clock only) a task smx_synth_task_supported takes; resets: its reset stream or null
static int ppo_window_rollout(const smx_synth_ppo_window_rollout* args, const smx_actor_clocks* clocks, bool clocked,
                              int task, smx_stream_t stream, const smx_reset_stream* resets = nullptr) {
    SMX_REQUIRE(args, SMX_E_NULL);
    const smx_synth_lstm_rollout& b = args->base;
    const smx_synth_rollout_t* a = &b.roll;
    const bool lstm = b.lstm != nullptr;
    SMX_REQUIRE(roll_pointers(a) && window_pointers(*args), SMX_E_NULL);
    SMX_REQUIRE(!lstm || (b.lstm_packed && b.hN && b.cN && args->carry_cells && args->cells), SMX_E_NULL);
    SMX_REQUIRE(cell_pairs_ok(b.h0, b.c0, b.h_before, b.c_before) && zfilter_ok(a), SMX_E_NULL);
    const smx_mlp3_t& n = *a->net;
    SMX_REQUIRE(!lstm || lstm_shape_ok(n, *b.lstm, b.hidden), SMX_E_SHAPE);
    SMX_REQUIRE(smx_synth_ppo_window_rollout_supported(lstm ? b.lstm->D : n.D, lstm ? b.lstm->H : 0, n.H1, n.H2, n.OUT),
                SMX_E_UNSUPPORTED);
    SMX_REQUIRE(synth_task_ok(task, lstm ? b.lstm->D : n.D, n.OUT) && !(clocked && task != SMX_TASK_DRIFT),
                SMX_E_UNSUPPORTED);
    SMX_REQUIRE(a->n > 0 && a->steps > 0, SMX_E_SHAPE);
    SMX_REQUIRE(clocked || (a->episode_len > 0 && a->t >= 0 && a->t < a->episode_len), SMX_E_SHAPE);
    SMX_REQUIRE(block_ok(a->actors_per_workgroup) && window_shape_ok(*args) && episode_shape_ok(a->mon), SMX_E_SHAPE);
    SMX_REQUIRE(noise_shape_ok(a->noise, a->n), SMX_E_SHAPE);
    SMX_REQUIRE(!resets || reset_shape_ok(*resets, a->n), SMX_E_SHAPE);
    SMX_REQUIRE(!resets || disturbance_rollout_ok(*resets, a->t, a->steps, a->episode_len), SMX_E_SHAPE);
    ClkArgs C = {};
    if (clocked) {
        // (the table numbers the call's closing pairs: rows <= capacity keeps them distinct)
        const int rc = clock_args(clocks, args->capacity, C);
        if (rc != SMX_OK) return rc;
    } else {
        // two workgroups must never write the same FIFO row: all n m rows of the call are distinct
        const long long m = closing_steps(a->t, a->steps, a->episode_len,
                                          [&](int t) { return window_closes(t, args->n_step, args->advance); });
        SMX_REQUIRE((long long)a->n * m <= args->capacity, SMX_E_SHAPE);
    }
    SMX_REQUIRE(aligned_ok(a->packed, n.b1, lstm ? b.lstm_packed : nullptr), SMX_E_ALIGN);
    const int rb = pick_block(a->actors_per_workgroup, a->n);
    if (!lstm) {
        RollArgsW G;
        memset(&G, 0, sizeof(G));
        roll_fields(a, n.D, G);
        G.W = win_fields(*args);
        const int lds = carve(G, rb, /*mma16=*/false, /*split_out=*/true, /*ztables=*/true, G.D);
        if (clocked)
            return launch<ppo_window_clk_kernel<1>, ppo_window_clk_kernel<2>, ppo_window_clk_kernel<4>>(
                with_clocks(G, C), rb, lds, stream);
        return with_task(task, [&](auto task_c) {
            constexpr int TASK = decltype(task_c)::value;
            if constexpr (TASK == SMX_TASK_DRIFT)
                return launch<ppo_window_kernel<1>, ppo_window_kernel<2>, ppo_window_kernel<4>>(G, rb, lds, stream);
            else
                return launch<ppo_window_task_kernel<1, TASK>, ppo_window_task_kernel<2, TASK>,
                              ppo_window_task_kernel<4, TASK>>(with_resets(G, resets), rb, lds, stream);
        });
    }
    LArgsW G;
    memset(&G, 0, sizeof(G));
    roll_fields(a, b.lstm->D, G);
    lstm_fields(b, G);
    G.W = win_fields(*args);
    const int lds = carve_lstm(G, rb);
    if (clocked)
        return launch<lstm_window_clk_kernel<1>, lstm_window_clk_kernel<2>, lstm_window_clk_kernel<4>>(
            with_clocks(G, C), rb, lds, stream);
    return with_task(task, [&](auto task_c) {
        constexpr int TASK = decltype(task_c)::value;
        if constexpr (TASK == SMX_TASK_DRIFT)
            return launch<lstm_window_kernel<1>, lstm_window_kernel<2>, lstm_window_kernel<4>>(G, rb, lds, stream);
        else
            return launch<lstm_window_task_kernel<1, TASK>, lstm_window_task_kernel<2, TASK>,
                          lstm_window_task_kernel<4, TASK>>(with_resets(G, resets), rb, lds, stream);
    });
}

extern "C" int smx_synth_ppo_window_rollout_f32(const smx_synth_ppo_window_rollout* args, smx_stream_t stream) {
    return ppo_window_rollout(args, nullptr, false, SMX_TASK_DRIFT, stream);
}

extern "C" int32_t smx_synth_task_supported(int32_t task, int32_t D, int32_t A) { return synth_task_ok(task, D, A); }

// the task entry point, with the reset stream or (null: none, or a disabled one) without
static int ppo_window_rollout_task(const smx_synth_ppo_window_rollout* args, int32_t task, const smx_reset_stream* resets,
                                   smx_stream_t stream) {
    SMX_REQUIRE(!(resets && task == SMX_TASK_DRIFT), SMX_E_UNSUPPORTED);
    if (task == SMX_TASK_DRIFT) return smx_synth_ppo_window_rollout_f32(args, stream);
    SMX_REQUIRE(task == SMX_TASK_REACH || task == SMX_TASK_ARM, SMX_E_UNSUPPORTED);
    return ppo_window_rollout(args, nullptr, false, task, stream, resets);
}

extern "C" int smx_synth_ppo_window_rollout_task_f32(const smx_synth_ppo_window_rollout* args, int32_t task,
                                                     smx_stream_t stream) {
    return ppo_window_rollout_task(args, task, nullptr, stream);
}

extern "C" int smx_synth_ppo_window_rollout_resets_f32(const smx_synth_ppo_window_rollout* args, int32_t task,
                                                       const struct smx_reset_stream* resets, smx_stream_t stream) {
    return ppo_window_rollout_task(args, task, resets && resets->enabled ? resets : nullptr, stream);
}

extern "C" int smx_synth_ppo_window_rollout_clocks_f32(const smx_synth_ppo_window_rollout* args,
                                                       const smx_actor_clocks* clocks, smx_stream_t stream) {
    return ppo_window_rollout(args, clocks, true, SMX_TASK_DRIFT, stream);
}

extern "C" int32_t smx_synth_ddpg_rollout_supported(int32_t D, int32_t H1, int32_t H2, int32_t A, int32_t ln) {
    if (!supported(D, H1, H2, A, /*mma16=*/false, /*split_out=*/false, /*ztables=*/false)) return 0;
    if (!ln) return 1;
    DLnArgs G;
    memset(&G, 0, sizeof(G));
    G.D = D; G.H1 = H1; G.H2 = H2; G.A = A;
    return carve_ln(G, G.ln, carve(G, 16, /*mma16=*/false, /*split_out=*/false, /*ztables=*/false, D)) <= ROLL_MAX_LDS;
}

extern "C" int32_t smx_synth_ddpg_population_block(int32_t n, int32_t actors_per_agent, int32_t forced) {
    if (n <= 0 || actors_per_agent <= 0 || actors_per_agent % 4 || !block_ok(forced)) return 0;
    return pick_population_block(forced, n, actors_per_agent);
}

// what the persistent DDPG launch asks of the block and takes from it, whatever the actor
static int persistent_ddpg_args(const smx_ddpg_rollout_t* a, DArgs& G, bool clocked) {
    SMX_REQUIRE(a && a->net && a->packed, SMX_E_NULL);
    const smx_mlp3_t& net = *a->net;
    SMX_REQUIRE(smx_synth_ddpg_rollout_supported(net.D, net.H1, net.H2, net.OUT, 0), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(net.D == a->D && net.OUT == a->A && a->steps > 0, SMX_E_SHAPE);
    SMX_REQUIRE(block_ok(a->actors_per_workgroup), SMX_E_SHAPE);
    SMX_REQUIRE(aligned_ok(a->packed, net.b1, nullptr), SMX_E_ALIGN);
    const int rc = common_args(a, G);
    if (rc != SMX_OK) return rc;
    if (!clocked) {
        // two workgroups must never write the same ring row: all n m rows of the call are distinct
        const long long m = closing_steps(a->t, a->steps, a->episode_len, [&](int t) { return t >= a->n_step - 1; });
        SMX_REQUIRE((long long)a->n * m <= a->capacity, SMX_E_SHAPE);
    }
    net_fields(net, a->packed, G);
    return SMX_OK;
}

// what a population asks of the variant and takes from it (-> the block size `rb`); copy_floats: what one agent's copy
// holds
static int population_args(const smx_ddpg_rollout_t* a, const smx_ddpg_actor_variant& v, long copy_floats, PopArgs& G,
                           int& rb) {
    const int apa = v.actors_per_agent;
    SMX_REQUIRE(apa > 0 && apa % 4 == 0 && v.agents > 0 && (long long)v.agents * apa == a->n, SMX_E_SHAPE);
    SMX_REQUIRE(v.measure_step >= -1 && v.measure_step < a->steps, SMX_E_SHAPE);
    SMX_REQUIRE(v.measure_step < 0 || v.dist, SMX_E_NULL);
    SMX_REQUIRE(v.packed_stride >= copy_floats && v.packed_stride % 4 == 0, SMX_E_SHAPE);
    SMX_REQUIRE(((uintptr_t)v.packed_pop & 15) == 0, SMX_E_ALIGN);
    rb = pick_population_block(a->actors_per_workgroup, a->n, apa);
    SMX_REQUIRE(rb > 0, SMX_E_SHAPE);
    G.stride = v.packed_stride; G.apa = apa; G.measure_step = v.measure_step; G.dist = v.dist;
    return SMX_OK;
}

// what a LayerNorm asks of the gains and biases
static int ln_args(const smx_mlp3_t& net, const smx_ddpg_actor_variant& v, LnTail& T) {
    SMX_REQUIRE(smx_synth_ddpg_rollout_supported(net.D, net.H1, net.H2, net.OUT, 1), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(v.ln_eps > 0.f, SMX_E_SHAPE);
    SMX_REQUIRE(((uintptr_t)v.ln & 3) == 0, SMX_E_ALIGN);
    T.g = v.ln; T.eps = v.ln_eps;
    return SMX_OK;
}

// the launch for one of the four actors: the block's checks, then the population's, then the LayerNorm's; clocked: with
// the actors' own clocks (checked behind the block: the table numbers the call's closing pairs, rows <= capacity
// keeps them distinct), the block's t / episode_len ignored; task: SMX_TASK_DRIFT, or (on the shared clock only) a task
// smx_synth_task_supported takes; resets: its reset stream or null
template <bool POP, bool LN>
static int ddpg_rollout_launch(const smx_ddpg_rollout_t* a, const smx_ddpg_actor_variant& v, const smx_actor_clocks* clocks,
                               bool clocked, smx_stream_t stream, int task = SMX_TASK_DRIFT,
                               const smx_reset_stream* resets = nullptr) {
    DdpgArgs<POP, LN> G;
    memset(&G, 0, sizeof(G));
    smx_ddpg_rollout_t own;
    if (clocked && a) {
        own = *a;
        own.t = 0;
        own.episode_len = 1;
        a = &own;
    }
    int rc = persistent_ddpg_args(a, G, clocked);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(synth_task_ok(task, a->D, a->A) && !(clocked && task != SMX_TASK_DRIFT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(!resets || reset_shape_ok(*resets, a->n), SMX_E_SHAPE);
    SMX_REQUIRE(!resets || disturbance_rollout_ok(*resets, a->t, a->steps, a->episode_len), SMX_E_SHAPE);
    ClkArgs C = {};
    if (clocked) {
        rc = clock_args(clocks, a->capacity, C);
        if (rc != SMX_OK) return rc;
    }
    const smx_mlp3_t& net = *a->net;
    int rb = POP ? 0 : pick_block(a->actors_per_workgroup, a->n);
    if constexpr (POP) {
        rc = population_args(a, v, LN ? pop_ln_copy_floats(net.D, net.H1, net.H2, net.OUT)
                                      : pop_copy_floats(net.D, net.H1, net.H2, net.OUT), G, rb);
        if (rc != SMX_OK) return rc;
    }
    if constexpr (LN) {
        rc = ln_args(net, v, G.ln);
        if (rc != SMX_OK) return rc;
        if constexpr (POP) G.ln.pop = v.packed_pop + pop_ln_off(net.D, net.H1, net.H2, net.OUT);
    }
    int lds = carve(G, rb, /*mma16=*/false, /*split_out=*/false, /*ztables=*/false, G.D);
    if constexpr (POP) {
        // agent 0's copy in the same tiles: its packed blocks as net_fields lays a net's out, its biases behind them
        G.popnet = G;
        smx_mlp3_t copy0 = net;
        copy0.b1 = v.packed_pop + pop_bias_off(net.D, net.H1, net.H2, net.OUT);
        copy0.b2 = copy0.b1 + net.H1;
        copy0.b3 = copy0.b2 + net.H2;
        net_fields(copy0, v.packed_pop, G.popnet);
    }
    if constexpr (LN) lds = carve_ln(G, G.ln, lds);
    if (clocked)
        return launch<ddpg_rollout_kernel<1, 3, POP, LN, true>, ddpg_rollout_kernel<2, 3, POP, LN, true>,
                      ddpg_rollout_kernel<4, 2, POP, LN, true>>(with_clocks(G, C), rb, lds, stream);
    return with_task(task, [&](auto task_c) {
        constexpr int TASK = decltype(task_c)::value;
        if constexpr (TASK == SMX_TASK_DRIFT)
            return launch<ddpg_rollout_kernel<1, 3, POP, LN>, ddpg_rollout_kernel<2, 3, POP, LN>,
                          ddpg_rollout_kernel<4, 2, POP, LN>>(G, rb, lds, stream);
        else
            return launch<ddpg_rollout_kernel<1, 3, POP, LN, false, TASK>, ddpg_rollout_kernel<2, 3, POP, LN, false, TASK>,
                          ddpg_rollout_kernel<4, 2, POP, LN, false, TASK>>(with_resets(G, resets), rb, lds, stream);
    });
}

// the DDPG entry points: the actor variant picks the instantiation
static int ddpg_rollout_variant(const smx_ddpg_rollout_t* a, const smx_ddpg_actor_variant* variant,
                                const smx_actor_clocks* clocks, bool clocked, smx_stream_t stream,
                                int task = SMX_TASK_DRIFT, const smx_reset_stream* resets = nullptr) {
    static const smx_ddpg_actor_variant plain = {};
    const smx_ddpg_actor_variant& v = variant ? *variant : plain;
    if (v.packed_pop)
        return v.ln ? ddpg_rollout_launch<true, true>(a, v, clocks, clocked, stream, task, resets)
                    : ddpg_rollout_launch<true, false>(a, v, clocks, clocked, stream, task, resets);
    return v.ln ? ddpg_rollout_launch<false, true>(a, v, clocks, clocked, stream, task, resets)
                : ddpg_rollout_launch<false, false>(a, v, clocks, clocked, stream, task, resets);
}

extern "C" int smx_synth_ddpg_rollout_f32(const smx_ddpg_rollout_t* a, const struct smx_ddpg_actor_variant* variant,
                                          smx_stream_t stream) {
    return ddpg_rollout_variant(a, variant, nullptr, false, stream);
}

// the task entry point, with the reset stream or (null: none, or a disabled one) without
static int ddpg_rollout_task(const smx_ddpg_rollout_t* a, int32_t task, const smx_reset_stream* resets, smx_stream_t stream) {
    SMX_REQUIRE(!(resets && task == SMX_TASK_DRIFT), SMX_E_UNSUPPORTED);
    if (task == SMX_TASK_DRIFT) return smx_synth_ddpg_rollout_f32(a, nullptr, stream);
    SMX_REQUIRE(task == SMX_TASK_REACH || task == SMX_TASK_ARM, SMX_E_UNSUPPORTED);
    static const smx_ddpg_actor_variant plain = {};
    return ddpg_rollout_launch<false, false>(a, plain, nullptr, false, stream, task, resets);
}

extern "C" int smx_synth_ddpg_rollout_task_f32(const smx_ddpg_rollout_t* a, int32_t task, smx_stream_t stream) {
    return ddpg_rollout_task(a, task, nullptr, stream);
}

extern "C" int smx_synth_ddpg_rollout_resets_f32(const smx_ddpg_rollout_t* a, int32_t task,
                                                 const struct smx_reset_stream* resets, smx_stream_t stream) {
    return ddpg_rollout_task(a, task, resets && resets->enabled ? resets : nullptr, stream);
}

// any actor variant on a task, with the reset stream or (null, or a disabled one) without
extern "C" int smx_synth_ddpg_rollout_variant_task_f32(const smx_ddpg_rollout_t* a,
                                                       const struct smx_ddpg_actor_variant* variant, int32_t task,
                                                       const struct smx_reset_stream* resets, smx_stream_t stream) {
    if (resets && !resets->enabled) resets = nullptr;
    SMX_REQUIRE(!(resets && task == SMX_TASK_DRIFT), SMX_E_UNSUPPORTED);
    if (task == SMX_TASK_DRIFT) return smx_synth_ddpg_rollout_f32(a, variant, stream);
    SMX_REQUIRE(task == SMX_TASK_REACH || task == SMX_TASK_ARM, SMX_E_UNSUPPORTED);
    return ddpg_rollout_variant(a, variant, nullptr, false, stream, task, resets);
}

extern "C" int smx_synth_ddpg_rollout_clocks_f32(const smx_ddpg_rollout_t* a, const struct smx_ddpg_actor_variant* variant,
                                                 const struct smx_actor_clocks* clocks, smx_stream_t stream) {
    return ddpg_rollout_variant(a, variant, clocks, true, stream);
}

extern "C" int smx_synth_ddpg_step_f32(const smx_ddpg_rollout_t* a, const float* mu, int64_t ld_mu, smx_stream_t stream) {
    SMX_REQUIRE(mu, SMX_E_NULL);
    DArgs G;
    const int rc = common_args(a, G);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(step_shape_ok(a->n, a->A, ld_mu, a->capacity), SMX_E_SHAPE);
    G.steps = 1;
    hipLaunchKernelGGL(ddpg_step_kernel, dim3((a->n + 3) / 4), dim3(256), 0, smx_s(stream), G, mu, (long long)ld_mu);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_ddpg_pixel_step(const struct smx_ddpg_pixel_step* args, const float* mu, int64_t ld_mu,
                                         smx_stream_t stream) {
    SMX_REQUIRE(args && mu && pixel_pointers(*args), SMX_E_NULL);
    const smx_ddpg_rollout_t* a = &args->base;
    DArgs G;
    const int rc = common_args(a, G);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(step_shape_ok(a->n, a->A, ld_mu, a->capacity) && a->n <= 65535, SMX_E_SHAPE);
    SMX_REQUIRE(pixel_shape_ok(*args, a->n_step), SMX_E_SHAPE);
    G.steps = 1;
    // (the copy workgroups: sized for the at most 3 S frames of a closing step; one frame's units each at least)
    const PArgs P = pixel_fields(*args, 3LL * args->frame_stacks);
    return launch_pixel<ddpg_pixel_step_kernel<16>, ddpg_pixel_step_kernel<1>>(G, P, a->n, mu, ld_mu, stream);
}

extern "C" int smx_synth_ddpg_pixel_pool_step(const struct smx_ddpg_pixel_pool_step* args, const float* mu, int64_t ld_mu,
                                              smx_stream_t stream) {
    SMX_REQUIRE(args && mu && args->pool && args->obs_pixel && args->frame_next && args->frame_first && args->frame_actor,
                SMX_E_NULL);
    const smx_ddpg_rollout_t* a = &args->base;
    DArgs G;
    const int rc = common_args(a, G);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(step_shape_ok(a->n, a->A, ld_mu, a->capacity) && a->n <= 65535, SMX_E_SHAPE);
    const int S = args->frame_stacks;
    SMX_REQUIRE(args->C > 0 && args->H > 0 && args->W > 0 && S > 0 && args->pool_len <= 0x7fffffffLL, SMX_E_SHAPE);
    // a pool that holds every frame a live row can name and the two this launch writes
    SMX_REQUIRE(args->pool_len >= (int64_t)a->n_step + S + 1, SMX_E_SHAPE);
    SMX_REQUIRE(args->episode_first >= 0 && args->frame >= args->episode_first, SMX_E_SHAPE);
    SMX_REQUIRE((((uintptr_t)args->frame_next | (uintptr_t)args->frame_first) & 7) == 0 &&
                ((uintptr_t)args->frame_actor & 3) == 0, SMX_E_ALIGN);
    G.steps = 1;
    PArgs P;
    memset(&P, 0, sizeof(P));
    P.C = args->C; P.H = args->H; P.W = args->W; P.S = S; P.hist_len = (int)args->pool_len;
    P.F = (long long)args->C * args->H * args->W;
    P.hist = args->pool; P.obs_pix = args->obs_pixel;
    // (the copy workgroups: the at most 1 + S frames of a terminal step, ~32 KB each)
    const long long X = ((1LL + S) * P.F + 32767) / 32768;
    P.X = (int)(X < 1 ? 1 : (X > 64 ? 64 : X));
    PoolArgs Q;
    Q.f = args->frame; Q.first = args->episode_first;
    Q.frame_next = args->frame_next; Q.frame_first = args->frame_first; Q.frame_actor = args->frame_actor;
    const bool vec = P.F % 16 == 0 && (((uintptr_t)P.hist | (uintptr_t)P.obs_pix) & 15) == 0;
    hipLaunchKernelGGL(vec ? ddpg_pixel_pool_step_kernel<16> : ddpg_pixel_pool_step_kernel<1>, dim3(1 + P.X, a->n),
                       dim3(256), 0, smx_s(stream), G, P, Q, mu, (long long)ld_mu);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_ppo_pixel_window_step(const struct smx_synth_ppo_pixel_window_step* args, const float* mu,
                                               int64_t ld_mu, smx_stream_t stream) {
    SMX_REQUIRE(args && mu && args->log_var && args->state && args->init_state, SMX_E_NULL);
    SMX_REQUIRE(window_pointers(*args) && pixel_pointers(*args) && episode_pointers_ok(args->mon), SMX_E_NULL);
    SMX_REQUIRE(cell_pairs_ok(nullptr, nullptr, args->h_before, args->c_before), SMX_E_NULL);
    // an LSTM policy's cells: the ring whenever a state comes in or a window's cells go out
    SMX_REQUIRE((!args->h_before && !args->cells) || args->carry_cells, SMX_E_NULL);
    SMX_REQUIRE(args->n > 0 && args->n <= 65535 && args->D > 0 && args->A > 0 && args->hidden >= 0, SMX_E_SHAPE);
    SMX_REQUIRE(!args->carry_cells || args->hidden > 0, SMX_E_SHAPE);
    SMX_REQUIRE(args->A <= SMX_PPO_PIXEL_STEP_MAX_A, SMX_E_UNSUPPORTED);
    static_assert(SMX_PPO_PIXEL_STEP_MAX_A <= SA_MAX, "the action tile of the step kernels");
    SMX_REQUIRE(args->episode_len > 0 && args->t >= 0 && args->t < args->episode_len, SMX_E_SHAPE);
    SMX_REQUIRE(window_shape_ok(*args) && step_shape_ok(args->n, args->A, ld_mu, args->capacity), SMX_E_SHAPE);
    SMX_REQUIRE(pixel_shape_ok(*args, args->n_step), SMX_E_SHAPE);
    SMX_REQUIRE(args->copy_workgroups >= 0 && args->copy_workgroups <= 1024 && episode_shape_ok(args->mon), SMX_E_SHAPE);
    SMX_REQUIRE(noise_shape_ok(args->noise, args->n), SMX_E_SHAPE);
    PWArgs G;
    memset(&G, 0, sizeof(G));
    G.n = args->n; G.D = args->D; G.A = args->A; G.Hl = args->hidden; G.t0 = args->t; G.episode_len = args->episode_len;
    G.log_var = args->log_var; G.noise_scale = args->noise_scale; G.eps = args->eps;
    G.state = args->state; G.init_state = args->init_state;
    G.h_before = args->h_before; G.c_before = args->c_before;
    G.W = win_fields(*args);
    G.mon = args->mon;
    G.nstream = args->noise;
    // the copy workgroups of this step: its destination frames -- (N + 1) S - 1 more at a closing step than the S - 1
    // (S + 1 on done) of any other
    const int S = args->frame_stacks;
    const bool done = args->t + 1 >= args->episode_len;
    PArgs P = pixel_fields(*args, (done ? 1 + S : S - 1) +
                                      (window_closes(args->t, args->n_step, args->advance)
                                           ? (long long)(args->n_step + 1) * S - 1 : 0));
    if (args->copy_workgroups) P.X = args->copy_workgroups;
    return launch_pixel<ppo_pixel_window_step_kernel<16>, ppo_pixel_window_step_kernel<1>>(G, P, args->n, mu, ld_mu, stream);
}

// ---- evaluation: whole episodes in one launch, nothing recorded ---------------------------------------------------------

extern "C" int32_t smx_synth_eval_supported(int32_t ddpg, int32_t task, int32_t D, int32_t H, int32_t H1, int32_t H2,
                                            int32_t A) {
    if (!synth_task_ok(task, D, A)) return 0;
    if (ddpg) return H == 0 && smx_synth_ddpg_rollout_supported(D, H1, H2, A, 0);
    if (H < 0) return 0;
    return smx_synth_ppo_window_rollout_supported(D, H, H1, H2, A);
}

// what both evaluation entry points ask of the rows and the reset stream -> the kernels' tail
static int eval_tail(int32_t n, int32_t episodes, int32_t episode_len, int32_t task, const smx_reset_stream& resets,
                     double* returns, EvalTail& V) {
    SMX_REQUIRE(!(resets.enabled && task == SMX_TASK_DRIFT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(n > 0 && episodes >= 1 && episode_len >= 1, SMX_E_SHAPE);
    SMX_REQUIRE((long long)n * episodes < (1LL << 31) && (long long)episodes * episode_len < (1LL << 31), SMX_E_SHAPE);
    SMX_REQUIRE(reset_shape_ok(resets, n) && disturbance_shape_ok(resets, resets.episode, episodes - 1), SMX_E_SHAPE);
    memset(&V, 0, sizeof(V));
    V.E = episodes;
    if (resets.enabled) V.rst = resets;
    V.returns = returns;
    return SMX_OK;
}

// ---- evaluation of several parameter sets in one launch ---------------------------------------------------------------------
// A snapshot is one policy's parameters as one blob (smx_eval_snapshot_floats): [smx_epoch_pack_f32's copy of the actor |
// b1 | b2 | b3], which is one agent's copy of a plain-actor population (pop_copy_floats); a PPO policy's goes on with
// log_var [A], the z-filter's zsum [D] | zsumsq [D] | zcount [1] and the LSTM's gate pass (smx_lstm_rollout_pack_f32),
// each on 16 bytes.  The offsets are floats from the blob's start; 0: the policy has no such block.
namespace {

struct SnapLayout {
    long bias, log_var, zsum, zsumsq, zcount, lstm, lstm_n, total;
};
inline long up4(long x) { return (x + 3) & ~3L; }

// D: the observation's width (the LSTM's input width where H > 0: the actor then reads the H units)
SnapLayout snap_layout(bool ddpg, int D, int H, int H1, int H2, int A, bool zfilter) {
    SnapLayout S;
    memset(&S, 0, sizeof(S));
    S.bias = pop_bias_off(H > 0 ? H : D, H1, H2, A);
    long o = S.bias + H1 + H2 + A;
    if (!ddpg) {
        S.log_var = o = up4(o);
        o += A;
        if (zfilter) {
            S.zsum = o = up4(o);
            o += D;
            S.zsumsq = o = up4(o);
            o += D;
            S.zcount = o = up4(o);
            o += 1;
        }
        if (H > 0) {
            S.lstm = o = up4(o);
            S.lstm_n = lstm_pack_floats(D, H);
            o += S.lstm_n;
        }
    }
    S.total = (o + 63) & ~63L;
    return S;
}

// floats of a snapshot, 0 for a policy no evaluation launch takes on any task (a DDPG actor has no z-filter)
long snap_floats(int ddpg, int D, int H, int H1, int H2, int A, int zfilter) {
    if ((zfilter != 0 && zfilter != 1) || (ddpg && zfilter)) return 0;
    if (!smx_synth_eval_supported(ddpg, SMX_TASK_DRIFT, D, H, H1, H2, A) &&
        !smx_synth_eval_supported(ddpg, SMX_TASK_REACH, D, H, H1, H2, A))
        return 0;
    return snap_layout(ddpg != 0, D, H, H1, H2, A, zfilter != 0).total;
}

// everything behind the packed weights but the LSTM's block: the small arrays, zeros between and behind them
struct SnapTailArgs {
    const float *b1, *b2, *b3, *log_var, *zsum, *zsumsq, *zcount;
    int D, H1, H2, A;
    SnapLayout S;
    float* blob;
};
__global__ __launch_bounds__(256) void eval_snapshot_tail_kernel(SnapTailArgs P) {
    const SnapLayout& S = P.S;
    for (long i = S.bias + (long)blockIdx.x * 256 + threadIdx.x; i < S.total; i += (long)gridDim.x * 256) {
        if (S.lstm_n && i >= S.lstm && i < S.lstm + S.lstm_n) continue;     // (the gate pass's pack kernel writes these)
        const long e = i - S.bias;
        float v = 0.f;
        if (e < P.H1) v = P.b1[e];
        else if (e < P.H1 + P.H2) v = P.b2[e - P.H1];
        else if (e < P.H1 + P.H2 + P.A) v = P.b3[e - P.H1 - P.H2];
        else if (P.log_var && i >= S.log_var && i < S.log_var + P.A) v = P.log_var[i - S.log_var];
        else if (P.zsum && i >= S.zsum && i < S.zsum + P.D) v = P.zsum[i - S.zsum];
        else if (P.zsum && i >= S.zsumsq && i < S.zsumsq + P.D) v = P.zsumsq[i - S.zsumsq];
        else if (P.zsum && i == S.zcount) v = P.zcount[0];
        P.blob[i] = v;
    }
}

template <typename Base>
WithSets<Base> with_sets(const Base& G, long long stride) {
    WithSets<Base> X;
    static_cast<Base&>(X) = G;
    X.set_stride = stride;
    return X;
}

// what both entry points ask of the sets (need: the floats of one snapshot; rows: n * episodes of one set)
int sets_ok(const struct smx_eval_sets* s, long need, long long rows) {
    SMX_REQUIRE(s->sets >= 1 && s->sets <= 65535 && (long long)s->sets * rows < (1LL << 31), SMX_E_SHAPE);
    SMX_REQUIRE(need > 0 && s->stride >= need && s->stride % 4 == 0, SMX_E_SHAPE);
    SMX_REQUIRE(((uintptr_t)s->blobs & 15) == 0, SMX_E_ALIGN);
    return SMX_OK;
}

// the actor's fields from set 0's snapshot
void snap_net_fields(const smx_mlp3_t& n, const float* blob, const SnapLayout& S, RollBase& G) {
    smx_mlp3_t m = n;
    m.b1 = const_cast<float*>(blob) + S.bias;
    m.b2 = m.b1 + n.H1;
    m.b3 = m.b2 + n.H2;
    net_fields(m, blob, G);
}

// the evaluation kernels of a policy family and task at the three block sizes; SETS: the argument block ends with the stride
template <bool LSTM, int TASK, bool SETS, typename Args>
int ppo_eval_sets_launch(const Args& G, int rb, int lds, smx_stream_t stream, int sets) {
    return launch<ppo_eval_kernel<1, 3, LSTM, true, TASK, SETS>, ppo_eval_kernel<2, 3, LSTM, true, TASK, SETS>,
                  ppo_eval_kernel<4, 2, LSTM, false, TASK, SETS>>(G, rb, lds, stream, sets);
}
template <int TASK, bool SETS, typename Args>
int ddpg_eval_sets_launch(const Args& G, int rb, int lds, smx_stream_t stream, int sets) {
    return launch<ddpg_eval_kernel<1, 3, TASK, SETS>, ddpg_eval_kernel<2, 3, TASK, SETS>,
                  ddpg_eval_kernel<4, 2, TASK, SETS>>(G, rb, lds, stream, sets);
}

// Both PPO evaluation entry points.  s null: the one policy of the block's own pointers (smx_synth_ppo_eval_f32); else the
// parameter sets, every parameter pointer into set 0's snapshot (smx_synth_ppo_eval_sets_f32, which has checked s itself).
// The checks run in the order either entry point has always had: the pointers, the shapes, the rows and the stream
// (eval_tail), then the sets (sets_ok) or the single policy's alignment.
int ppo_eval(const smx_synth_ppo_eval* a, const smx_eval_sets* s, smx_stream_t stream) {
    SMX_REQUIRE(a && a->net && a->init_state && a->returns && (s ? s->blobs != nullptr : a->packed && a->log_var), SMX_E_NULL);
    const bool lstm = a->lstm != nullptr;
    SMX_REQUIRE(s || !lstm || a->lstm_packed, SMX_E_NULL);
    SMX_REQUIRE(s || ((a->zsum == nullptr) == (a->zsumsq == nullptr) && (a->zsum == nullptr) == (a->zcount == nullptr)),
                SMX_E_NULL);
    const smx_mlp3_t& n = *a->net;
    const int D = lstm ? a->lstm->D : n.D, H = lstm ? a->lstm->H : 0;
    SMX_REQUIRE(!lstm || lstm_shape_ok(n, *a->lstm, a->hidden), SMX_E_SHAPE);
    SMX_REQUIRE(smx_synth_eval_supported(0, a->task, D, H, n.H1, n.H2, n.OUT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(block_ok(a->actors_per_workgroup) && noise_shape_ok(a->noise, a->n), SMX_E_SHAPE);
    PEvalArgs G;
    memset(&G, 0, sizeof(G));
    int rc = eval_tail(a->n, a->episodes, a->episode_len, a->task, a->resets, a->returns, G.ev);
    if (rc != SMX_OK) return rc;
    G.n = a->n * a->episodes;                        // the rows (of one set)
    const float* gate = nullptr;                     // the LSTM's gate pass
    if (s) {
        SMX_REQUIRE(s->zfilter == 0 || s->zfilter == 1, SMX_E_SHAPE);
        const SnapLayout S = snap_layout(false, D, H, n.H1, n.H2, n.OUT, s->zfilter != 0);
        rc = sets_ok(s, S.total, G.n);
        if (rc != SMX_OK) return rc;
        snap_net_fields(n, s->blobs, S, G);
        G.log_var = s->blobs + S.log_var;
        if (s->zfilter) {
            G.zsum = s->blobs + S.zsum; G.zsumsq = s->blobs + S.zsumsq; G.zcount = s->blobs + S.zcount;
        }
        gate = s->blobs + S.lstm;
    } else {
        SMX_REQUIRE(aligned_ok(a->packed, n.b1, lstm ? a->lstm_packed : nullptr), SMX_E_ALIGN);
        net_fields(n, a->packed, G);
        G.log_var = a->log_var;
        G.zsum = a->zsum; G.zsumsq = a->zsumsq; G.zcount = a->zcount;
        gate = a->lstm_packed;
    }
    G.D = D; G.A = n.OUT; G.out_act = a->out_act; G.zeps = a->zeps;
    G.init_state = a->init_state;
    G.steps = G.episode_len = a->episode_len;
    if (a->noise.enabled) G.nstream = a->noise;
    const int sets = s ? s->sets : 1;
    const int rb = pick_block(a->actors_per_workgroup, sets * G.n);
    int lds;
    if (lstm) {
        G.H = H; G.Hl = a->hidden;
        G.Pg = gate; G.bg = G.Pg + pack_words(4 * G.H, lstm_dp(D) + G.H) * 4;
        lds = carve_lstm(G, rb);
    } else {
        lds = carve(G, rb, /*mma16=*/false, /*split_out=*/true, /*ztables=*/true, G.D);
    }
    auto go = [&](auto lstm_c, auto task_c) {
        constexpr bool LSTM = decltype(lstm_c)::value;
        constexpr int TASK = decltype(task_c)::value;
        return s ? ppo_eval_sets_launch<LSTM, TASK, true>(with_sets(G, s->stride), rb, lds, stream, sets)
                 : ppo_eval_sets_launch<LSTM, TASK, false>(G, rb, lds, stream, sets);
    };
    return with_task(a->task, [&](auto task_c) {
        return lstm ? go(std::true_type{}, task_c) : go(std::false_type{}, task_c);
    });
}

// both DDPG evaluation entry points, as ppo_eval
int ddpg_eval(const smx_synth_ddpg_eval* a, const smx_eval_sets* s, smx_stream_t stream) {
    SMX_REQUIRE(a && a->net && a->init_state && a->returns && (s ? s->blobs != nullptr : a->packed != nullptr), SMX_E_NULL);
    const smx_mlp3_t& n = *a->net;
    SMX_REQUIRE(smx_synth_eval_supported(1, a->task, n.D, 0, n.H1, n.H2, n.OUT), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(block_ok(a->actors_per_workgroup), SMX_E_SHAPE);
    DEvalArgs G;
    memset(&G, 0, sizeof(G));
    int rc = eval_tail(a->n, a->episodes, a->episode_len, a->task, a->resets, a->returns, G.ev);
    if (rc != SMX_OK) return rc;
    G.n = a->n * a->episodes;                        // the rows (of one set)
    if (s) {
        SMX_REQUIRE(s->zfilter == 0, SMX_E_SHAPE);   // (a DDPG actor has no z-filter)
        const SnapLayout S = snap_layout(true, n.D, 0, n.H1, n.H2, n.OUT, false);
        rc = sets_ok(s, S.total, G.n);
        if (rc != SMX_OK) return rc;
        snap_net_fields(n, s->blobs, S, G);
    } else {
        SMX_REQUIRE(aligned_ok(a->packed, n.b1, nullptr), SMX_E_ALIGN);
        net_fields(n, a->packed, G);
    }
    G.D = n.D; G.A = n.OUT;
    G.init_state = a->init_state;
    G.steps = G.episode_len = a->episode_len;
    const int sets = s ? s->sets : 1;
    const int rb = pick_block(a->actors_per_workgroup, sets * G.n);
    const int lds = carve(G, rb, /*mma16=*/false, /*split_out=*/false, /*ztables=*/false, G.D);
    return with_task(a->task, [&](auto task_c) {
        constexpr int TASK = decltype(task_c)::value;
        return s ? ddpg_eval_sets_launch<TASK, true>(with_sets(G, s->stride), rb, lds, stream, sets)
                 : ddpg_eval_sets_launch<TASK, false>(G, rb, lds, stream, sets);
    });
}

}  // namespace

extern "C" int64_t smx_eval_snapshot_floats(int32_t ddpg, int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A,
                                            int32_t zfilter) {
    return snap_floats(ddpg, D, H, H1, H2, A, zfilter);
}

extern "C" int smx_eval_snapshot_store_f32(const struct smx_eval_snapshot_src* src, float* blob, smx_stream_t stream) {
    SMX_REQUIRE(src && blob && src->net, SMX_E_NULL);
    const smx_mlp3_t& n = *src->net;
    SMX_REQUIRE(n.W1 && n.b1 && n.W2 && n.b2 && n.W3 && n.b3 && (src->ddpg || src->log_var), SMX_E_NULL);
    const bool zf = src->zsum != nullptr;
    SMX_REQUIRE(zf == (src->zsumsq != nullptr) && zf == (src->zcount != nullptr), SMX_E_NULL);
    const smx_lstm_t* l = src->lstm;
    SMX_REQUIRE(!l || (l->W_ih && l->W_hh && l->b_ih && l->b_hh), SMX_E_NULL);
    SMX_REQUIRE(!l || n.D == l->H, SMX_E_SHAPE);
    const int D = l ? l->D : n.D, H = l ? l->H : 0;
    SMX_REQUIRE(snap_floats(src->ddpg, D, H, n.H1, n.H2, n.OUT, zf) > 0, SMX_E_UNSUPPORTED);
    SMX_REQUIRE(((uintptr_t)blob & 15) == 0, SMX_E_ALIGN);
    const SnapLayout S = snap_layout(src->ddpg != 0, D, H, n.H1, n.H2, n.OUT, zf);
    smx_epoch_pack_t item;
    memset(&item, 0, sizeof(item));
    item.net = src->net;
    item.packed = blob;
    int rc = smx_epoch_pack_f32(&item, 1, stream);
    if (rc != SMX_OK) return rc;
    if (l) {
        rc = smx_lstm_rollout_pack_f32(l, blob + S.lstm, stream);
        if (rc != SMX_OK) return rc;
    }
    SnapTailArgs P;
    memset(&P, 0, sizeof(P));
    P.b1 = n.b1; P.b2 = n.b2; P.b3 = n.b3;
    if (!src->ddpg) P.log_var = src->log_var;
    P.zsum = src->zsum; P.zsumsq = src->zsumsq; P.zcount = src->zcount;
    P.D = D; P.H1 = n.H1; P.H2 = n.H2; P.A = n.OUT;
    P.S = S;
    P.blob = blob;
    const long tail = S.total - S.bias;
    hipLaunchKernelGGL(eval_snapshot_tail_kernel, dim3((unsigned)((tail + 255) / 256 < 64 ? (tail + 255) / 256 : 64)),
                       dim3(256), 0, smx_s(stream), P);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_ppo_eval_f32(const struct smx_synth_ppo_eval* a, smx_stream_t stream) {
    return ppo_eval(a, nullptr, stream);
}

extern "C" int smx_synth_ddpg_eval_f32(const struct smx_synth_ddpg_eval* a, smx_stream_t stream) {
    return ddpg_eval(a, nullptr, stream);
}

extern "C" int smx_synth_ppo_eval_sets_f32(const struct smx_synth_ppo_eval* a, const struct smx_eval_sets* s,
                                           smx_stream_t stream) {
    SMX_REQUIRE(s, SMX_E_NULL);
    return ppo_eval(a, s, stream);
}

extern "C" int smx_synth_ddpg_eval_sets_f32(const struct smx_synth_ddpg_eval* a, const struct smx_eval_sets* s,
                                            smx_stream_t stream) {
    SMX_REQUIRE(s, SMX_E_NULL);
    return ddpg_eval(a, s, stream);
}
