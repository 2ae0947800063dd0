// One DDPG iteration on ROW BLOCKS (surreal/learner/ddpg.py:244-352; low-dimensional observations, one critic):
// the layer-by-layer schedule is ~19 dependent launches of 512-row problems, each a few microseconds of work behind a
// launch boundary and an L2 first touch (0.19 ms per iteration, 70 % of it in 15 dense launches).  Batch rows are
// independent up to the weight gradients, so here a workgroup owns FOUR rows and carries them through whole chains on the
// 4-row loop of the rollout kernel (smx_rows4_mma.inc.h: v_mfma_f32_4x4x1, weights in the fragment order of
// smx_epoch_pack.inc.h) -- configs[2]'s batch of 512 is 128 workgroups:
//
//   ddpg_rows4_kernel<0>      target actor -> target critic -> Q'(s', mu'(s'));  critic -> Q(s, a);  y and dLoss/dQ;
//                             the critic's data gradients dz2, dz1;  the actor's forward pass for ITS update (it reads
//                             only the actor's parameters, which the critic update does not touch)
//   ddpg_rows_wgrad_update    the critic's weight gradients, Adam, its target network's update, the packed copies
//   ddpg_rows4_kernel<1>      Q(s, mu(s)) through the UPDATED critic; d(-mean Q)/d(action); tanh'; the actor's data
//                             gradients dz2, dz1
//   ddpg_rows_wgrad_update    the same for the actor;  [statistics: smx_ddpg_stats_f32]
//
// TD3 (ddpg.py:119-147, 266-283, 312-319: a second critic, clipped noise on the target policy's action) is the same
// schedule with a longer first chain and one more group:
//
//   ddpg_rows4_kernel<2>      target actor -> both target critics (the second at the noised, clamped action);  y = min of
//                             the two Bellman targets;  each critic's Q(s, a), dLoss/dQ against that y and data gradients;
//                             the actor's forward pass (20 layers; td3_critic_chain)
//   ddpg_rows_wgrad_update    critic 1;  ddpg_rows_wgrad_update  critic 2 (its blocks live in a packed buffer of their own)
//   ddpg_rows4_kernel<1>      unchanged: the actor goes through critic 1 only
//   ddpg_rows_wgrad_update    the actor;  [statistics: a second block for (q2, y) by the same workgroup]
//
// use_layernorm (builders.py:42-48, 65-75: Linear -> ReLU -> LayerNorm on every hidden layer; one critic) is the same
// four launches: LayerNorm is a rule BEHIND a hidden layer's step, not a layer (ddpg_rows4_ln_kernel<0>, <1>; the three
// instantiations above keep their code):
//
//   forward    behind the barrier that ends the layer the block's 4 rows are normalised in LDS (ln_rows of
//              smx_ln_rows.inc.h, shared with the rollout: the bits of smx_layernorm_forward_f32 given the same row); the
//              pre-LayerNorm tile stays in LDS beside the output, both go to HBM with the row's mean and rstd
//   backward   layernorm_bwd_kernel's expressions, one wave per row, from the dn / pre-LayerNorm tiles and the statistics
//              in LDS: the gradient at the ReLU's input (the x > 0 mask folded in) to LDS and HBM
//   gradients  dgamma = sum_rows dn xhat, dbeta = sum_rows dn: further workgroups of the group's gradient-and-step
//              launch, behind the tiles and in front of the statistics workgroup; no atomics
// The gains and biases are read row-major from the parameter buffers, as the dense biases are: no packed copy.
//
// use_layernorm together with TD3 is the composition, TD3's five launches (ddpg_rows4_ln_kernel<2>: the chain body with
// PHASE == 2 and LN; td3_critic_chain: the 20 products, a forward rule behind each of the 12 hidden layers, a backward
// rule behind each critic's loss and behind each critic's W2^T product -- 16 rules; only that instantiation takes the
// 20-step rule table, LnProgT<20>):
//
//   ddpg_rows4_ln_kernel<2>   target actor -> target critic 1 at mu'(s') -> target critic 2 at clamp(mu'(s') + noise);
//                             critic 1 forward, y = min(y1, y2) kept in LDS, dn2, LayerNorm-2 backward, W2^T lo, LayerNorm-1
//                             backward; the same for critic 2 against the kept y (dn2_2, dz1c2: buffers of its own); the
//                             actor's forward pass
//   ddpg_rows_wgrad_update    critic 1;  critic 2 (SMX_DDPG_GROUP_CRITIC2: its three weight gradients, dgamma / dbeta of its
//                             two LayerNorms, Adam, its target, the copies inside packed2)
//   ddpg_rows4_ln_kernel<1>   unchanged;  ddpg_rows_wgrad_update  the actor, both statistics blocks
//
// Activations and gradients that the weight-gradient launches read go to HBM row-major, exactly the buffers of the
// layer-by-layer schedule.  Products are summed in the MFMA loop's order (32-wide K chunks, k ascending per lane group),
// not in smx_linear_f32's: results agree with the layered schedule to fp32 rounding, not bit for bit.
//
// History: round 5 built this on 16-row blocks and one noinline dense function (32 workgroups bound by the matrix pipes of
// 32 CUs, 92 + 46 us for the two chains against the 145 us of the launches they replaced: slower, off by default); round 6
// moved it to 4-row blocks (bound by what a CU pulls from L2 -- every workgroup streams every weight once per layer -- on
// four times as many CUs: 42 + 22 us) and removed the 16-row kernels: they were never faster than the level schedule.
#include "smx_common.h"
#include <string.h>

#define SMX_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

namespace {
#include "smx_epoch_pack.inc.h"
#include "smx_epoch_mma.inc.h"
#include "smx_rows4_mma.inc.h"
#include "smx_ddpg_stats.inc.h"
#include "smx_ln_rows.inc.h"

constexpr int DNWV = 8;           // wavefronts per workgroup: two per SIMD (one's loads hide under the other's MFMAs)
constexpr int DNTH = 64 * DNWV;
constexpr int RBLK = 4;           // batch rows per workgroup
constexpr int LDO = 36;           // row stride of an output tile (<= 32 outputs)
constexpr int LDK4 = 80;          // row stride of a tile that is the K <= 32 input of a product (two zero-padded chunks; strides = 16 mod 64: the 16 (row, kq) readers on distinct banks)
constexpr int DTG4 = 4;           // feature tiles a wave carries per pass (8 x 4 = 32 tiles: 400 features in one pass)
constexpr int MAX_LDS = 128 * 1024;
enum { A_NONE = 0, A_RELU = 1, A_TANH = 2, A_MASK = 3 };

__host__ __device__ inline int r64(int v) { return (v + 63) & ~63; }

struct PMat {                     // a matrix in fragment order (smx_epoch_pack.inc.h): M features x K inputs
    const float* P;
    int M, K;
};

// Phase timestamps (cycle counter of thread 0 of every workgroup into a caller-supplied buffer, 128 slots per workgroup:
// 0 .. 15 the launch's phases, 16 + 5 k .. the k-th layer's entry / K loop / epilogue / barrier) exist only in a build with
// -DSMX_DDPG_TIMING (scripts/bench_ddpg_rows.py); the product build has none.
#ifdef SMX_DDPG_TIMING
#define TSTAMP(i) do { if (G.tbuf && threadIdx.x == 0) G.tbuf[(size_t)blockIdx.x * 128 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define TSTAMP(i) do { } while (0)
#endif

struct RNet {                     // a network's biases (row-major parameter buffer) and packed weights
    const float *b1, *b2, *b3;
    PMat W1, W2, W3;
};

struct RArgs {
    int rows, D, A, H1, H2, c1, c2;
    RNet a, c, ta, tc;
    PMat cW2Tlo, cW2Thi, aW3T, aW2T;      // the transposed blocks of the backward products
    const float* cW3;                     // the critic's output layer, row-major [c2]
    const float *x, *xn, *actions, *rewards, *dones;
    float gamma_n;
    float *xcat, *h2c, *q, *q_next, *y, *dz3, *dz2, *dxcat;         // critic phase (xcat / dxcat: row stride c1 + A)
    float *h1a, *h2a, *act;                                          // the actor's forward pass
    float *q_actor, *dz3a, *dz2a, *dz1a;                             // actor phase
    int* step;
    // LDS carve-up (float offsets)
    int ldx, ldA, ldB, ldC, oX, oXn, oA, oB, oC, oO, oO2, oO3, oZ, oS, oR, total;
    long long* tbuf;              // SMX_DDPG_TIMING builds
    // TD3 (ddpg_rows4_kernel<2> only): the second critic and its target, the clipped noise of the target policy's action
    RNet c2n, tc2;
    PMat c2W2Tlo;
    const float* c2W3;                    // the second critic's output layer, row-major [c2]
    const float* noise;                   // [rows][A] or null
    float *xcat2, *h2c2, *q2, *q_next2, *dz3_2, *dz2_2, *dxcat2;
    int oY;                               // the Bellman target, kept for the second critic's loss
};

__device__ __forceinline__ void zero_lds(int total) {
    extern __shared__ float sm[];
    for (int i = threadIdx.x; i < (total >> 2); i += DNTH) *(float4*)(sm + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// rows row0 .. row0 + 3 of a row-major [rows][D] matrix -> an LDS tile (zero past the batch)
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int ld_src, int cols, long row0, int nrows,
                                           int off, int ld) {
    extern __shared__ float sm[];
    for (int idx = threadIdx.x; idx < RBLK * cols; idx += DNTH) {
        const int n = idx / cols, j = idx - n * cols;
        sm[off + n * ld + j] = (n < nrows) ? src[(size_t)(row0 + n) * ld_src + j] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The two chains as a LAYER PROGRAM.  With one noinline dense function called a dozen times (round 5's structure) the
// calls were the larger half of a launch whose K loops are 2 - 9 k cycles (phase stamps: 3.3 k cycles per layer between
// return and the next entry -- callee-saved registers through scratch -- and 1.1 k from entry to the first product).
// Here the host writes the chain as a table of steps in the kernel arguments and the
// kernel is ONE loop over it: the layer body exists once, inline, its operands arrive by scalar loads.  What sits between
// two layers of a chain (the concat of the action, the Bellman target and dLoss/dQ, tanh') is the `post` of the step
// before it.
//
//  * lane (fm, kq) keeps row kq of feature 16 t + fm: the kq groups meet by meet_rows (3 swaps, 3 adds)
//  * layers of at most two feature tiles (the heads: 6 actions, 1 value; the action gradient) split K over the eight
//    wavefronts instead of leaving 64 - 80 dependent products to one: a wave takes ceil(C2 / 8) chunks, the eight partial
//    sums meet through LDS in wave order (k ascending inside a wave's chunks: a fixed order, not the full-K order)
// ---------------------------------------------------------------------------------------------------------------
enum { P_NONE = 0, P_TC_CAT, P_C_CAT, P_LOSS, P_A_CAT, P_A_DQ, P_A_TANH, P_TC2_CAT, P_C2_CAT, P_LOSS2 };
constexpr int MAX_STEPS = 20;        // the TD3 critic chain

struct Step {
    const float* W;               // packed weights
    const float* bias;            // [M] or null
    float* g;                     // HBM output [rows][ldg] or null
    int M, K, in_off, ldi, act, mask_off, ldm, out_off, ldo, ldg, post;
};
struct Prog {
    int n;
    Step s[MAX_STEPS];
};

// LayerNorm (ddpg_rows4_ln_kernel): what the step's LayerNorm rule needs, beside the step.  FWD: the layer has written
// relu(z) to the pre-LayerNorm tile (its out tile) and to HBM (its g); the rule writes the normalised rows to tile `t`
// and to `n`, the statistics to slot `st` of the LDS statistics and to mean / rstd.  BWD: the layer (or the loss rule)
// has left dn in tile `d`; the rule writes the gradient at the ReLU's input to tile `t` (< 0: none) and to `n`.
enum { LN_NONE = 0, LN_FWD = 1, LN_BWD = 2 };
constexpr int LN_STEPS = 13;         // the LayerNorm critic chain
constexpr int LN_STEPS_TD3 = 20;     // ... of TD3 (ddpg_rows4_ln_kernel<2> alone takes the longer table)
constexpr int LNR_MAXC = 16;         // columns per lane: F <= 1024, as layernorm_fwd_kernel
struct LnStep {
    const float *gamma, *beta;    // (BWD: gamma only)
    float* n;                     // HBM [rows][ldn] or null
    float *mean, *rstd;           // FWD: HBM [rows] or null
    int kind, F, ldn;
    int p_off, ldp;               // the pre-LayerNorm tile
    int t_off, ldt;
    int d_off, ldd;
    int st;
};
struct LnTail {                                       // what a chain's rules share, behind either table
    float eps;
    float* dn2;                                       // critic chain: d/d(LayerNorm 2's output) [rows][c2]
    const float *a1, *a2, *am1, *ar1, *am2, *ar2;     // actor chain: the actor's pre-LayerNorm rows and statistics
    int oP1, ldP1, oP2, ldP2, oD, ldD, oM;            // LDS (float offsets): two pre-LayerNorm tiles, dn, statistics [4][2][4]
    float* dn2_2;                                     // TD3's critic chain: the same for the second critic (else null)
};
template <int N>
struct LnProgT {
    LnStep s[N];
    LnTail t;
};
typedef LnProgT<LN_STEPS_TD3> LnProg;                 // what the host fills; the 13-step launches take its narrow() copy
static_assert(sizeof(RArgs) + sizeof(Prog) + sizeof(LnProg) < 4096, "all go by value in the kernel arguments");

// The rule's fields are wanted BEHIND the layer's K loop: at an offset the compiler cannot see through, or it loads them
// at the head of the step (the chain's own before the loop over the steps) and keeps two dozen scalar registers occupied
// across the K loop, which is at the register file's limit as it is
template <class LP>
__device__ __forceinline__ const LnStep& ln_late(const LP* Q, int si) {
    asm volatile("" : "+s"(si));
    return Q->s[si];
}
template <class LP>
__device__ __forceinline__ const LP* ln_late(const LP* Q) {
    int z = 0;
    asm volatile("" : "+s"(z));
    return (const LP*)((const char*)Q + z);
}

__device__ __forceinline__ int behind_here(int v) {      // the same value, formed no earlier than this point
    asm volatile("" : "+v"(v));
    return v;
}

struct LnEmitRows {               // ln_rows' outputs beside the LDS tile
    float* n;
    int ldn;
    float *mean, *rstd, *st;      // st: LDS [2][RBLK]
    long row0;
    int nrows, lane;
    __device__ __forceinline__ void value(int r, int j, float y) const {
        if (n && r < nrows) n[(size_t)(row0 + r) * ldn + j] = y;
    }
    __device__ __forceinline__ void stats(int r, float m, float rs) const {
        if (lane == 0) {
            st[r] = m;
            st[RBLK + r] = rs;
            if (mean && r < nrows) { mean[row0 + r] = m; rstd[row0 + r] = rs; }
        }
    }
};

// the LayerNorm's backward rule on the block's rows: layernorm_bwd_kernel's expressions and order (smx_ddpg.hip; its zero
// terms for the columns past F left out), one wave per row -- g = dn gamma, the two wave sums, rs ((g - m1) - xhat m2), the
// x > 0 mask of the ReLU in front.  Given the same dn, pre-LayerNorm row and statistics: its bits.
__device__ __forceinline__ void ln_bwd_rows(const float* dn, int ldd, const float* pre, int ldp, const float* st, int F,
                                            const float* __restrict__ gamma, float* tz, int ldt, float* gz, int ldg,
                                            long row0, int nrows, int wv, int lane) {
#pragma unroll 1
    for (int r = wv; r < RBLK; r += DNWV) {
        const float m = st[r], rs = st[RBLK + r];
        const float* xr = pre + r * ldp;
        const float* dr = dn + r * ldd;
        float g[LNR_MAXC];           // (x and xhat are formed again from LDS in the second pass: the same bits)
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < LNR_MAXC; ++c) {
            if (64 * c >= F) break;                  // (wave-uniform)
            const int j = lane + 64 * c;
            const bool in = j < F;
            const float xv = in ? xr[j] : 0.f;
            const float d = in ? dr[j] : 0.f;
            const float xh = in ? (xv - m) * rs : 0.f;
            g[c] = in ? d * gamma[in ? j : 0] : 0.f;
            s1 += g[c];
            s2 += g[c] * xh;
        }
        const float m1 = smx_wave_sum(s1) / (float)F, m2 = smx_wave_sum(s2) / (float)F;
#pragma unroll
        for (int c = 0; c < LNR_MAXC; ++c) {
            if (64 * c >= F) break;
            const int j = lane + 64 * c;
            if (j < F) {
                const float xv = xr[j];
                const float xh = (xv - m) * rs;
                float v = rs * ((g[c] - m1) - xh * m2);
                v = (xv > 0.f) ? v : 0.f;
                if (tz) tz[r * ldt + j] = v;
                if (gz && r < nrows) gz[(size_t)(row0 + r) * ldg + j] = v;
            }
        }
    }
}

#ifdef SMX_DDPG_TIMING
#define PSTAMP(k, i) do { if (G.tbuf && threadIdx.x == 0) G.tbuf[(size_t)blockIdx.x * 128 + 16 + 5 * (k) + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define PSTAMP(k, i) do { } while (0)
#endif

// PHASE 0: the critic chain, 1: the actor chain, 2: the critic chain of TD3 (two critics, y = min of their targets; its
// rules exist in that instantiation only)
// LN: the LayerNorm variant, its rules behind `if constexpr (LN)`; Q is null without
template <int PHASE, bool LN, class LP>
__device__ __forceinline__ void ddpg_rows4_chain(const RArgs& G, const Prog& P, const LP* Q) {
    extern __shared__ float sm[];
    constexpr int RB = RBLK;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fm = lane & 15, kq = lane >> 4;
    const long row0 = (long)blockIdx.x * RB;
    int nrows = G.rows - (int)row0;
    nrows = nrows > RB ? RB : nrows;
    const int A = G.A, c1 = G.c1, c2 = G.c2, ldc = c1 + A;
    TSTAMP(0);
    zero_lds(G.total);
    __syncthreads();
    stage_rows(G.x, G.D, G.D, row0, nrows, G.oX, G.ldx);
    float rew = 0.f, dn = 0.f;
    if (PHASE == 0 || PHASE == 2) {
        stage_rows(G.xn, G.D, G.D, row0, nrows, G.oXn, G.ldx);
        if (tid < nrows) { rew = G.rewards[row0 + tid]; dn = G.dones[row0 + tid]; }
    } else {
        stage_rows(G.act, A, A, row0, nrows, G.oO, LDO);
    }
    SMX_LDS_BARRIER();

#pragma unroll 1
    for (int si = 0; si < P.n; ++si) {
        const Step& S = P.s[si];
        const int M = S.M, K = S.K, act = S.act, ldi = S.ldi, ldm = S.ldm, ldo = S.ldo, ldg = S.ldg;
        const int mask_off = S.mask_off, out_off = S.out_off;
        const int tiles = (M + 15) >> 4, C2 = pack_chunks(K);
        const rsrc_t rw = make_rsrc(S.W, (unsigned)tiles * (unsigned)C2 * 2048u);
        const rsrc_t rb = make_rsrc(S.bias ? S.bias : S.W, S.bias ? (unsigned)M * 4u : 0u);
        const rsrc_t rg = make_rsrc(S.g ? S.g : S.W, S.g ? (unsigned)G.rows * (unsigned)ldg * 4u : 0u);
        const float* in = sm + S.in_off;
        PSTAMP(si, 0);
        // row `r` of feature f is finished: bias, activation, the tile for the next layer, the row-major copy
        auto finish = [&](float z, float bias_v, int f, int r) {
            z += bias_v;
            if (act == A_RELU) z = (z < 0.f) ? 0.f : z;
            else if (act == A_TANH) z = tanhf(z);
            else if (act == A_MASK) z = (sm[mask_off + r * ldm + f] > 0.f) ? z : 0.f;
            const float v = (f < M) ? z : 0.f;
            if (out_off >= 0) sm[out_off + r * ldo + f] = v;
            const bool ok = r < nrows && f < M;                      // (no HBM output: every offset is out of range)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rg,
                                                  ok ? ((unsigned)(row0 + r) * (unsigned)ldg + (unsigned)f) * 4u : OOB, 0, 0);
        };
        if (tiles <= 2) {
            // ---- split K: wave w takes chunks [w per, w per + per) of both tiles ----
            const int per = (C2 + DNWV - 1) / DNWV;
            const int ca = wv * per;
            int cb = ca + per;
            cb = cb > C2 ? C2 : cb;
            const int ft = 16 * (tid >> 6) + fm;                     // the (tile, row, feature) thread tid finishes
            const float bfin = ld4(rb, (tid < 64 * tiles && ft < M) ? (unsigned)ft * 4u : OOB);
            f32x4 a2[2][1];
            a2[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
            a2[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* bp = in + (lane & 3) * ldi + 8 * kq;
            unsigned wo[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) wo[g] = (g < tiles) ? ((unsigned)g * (unsigned)C2 * 512u + (unsigned)lane * 4u) * 4u : OOB;
#pragma unroll 1
            for (int c = ca; c < cb; c += 2) {
                const unsigned none[2] = {OOB, OOB};
                WFrag4<2, 1> F0, F1;
                ld_wfrag4<2, 1>(F0, rw, wo, bp, ldi, c);
                if (c + 1 < cb) ld_wfrag4<2, 1>(F1, rw, wo, bp, ldi, c + 1);
                else ld_wfrag4<2, 1>(F1, rw, none, bp, ldi, 0);
                mma4_chunk<2, 1>(a2, F0);
                mma4_chunk<2, 1>(a2, F1);
            }
            PSTAMP(si, 1);
            float* red = sm + G.oR;                                  // [wave][tile][row][16]
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (g < tiles) red[((wv * 2 + g) * 4 + kq) * 16 + fm] = meet_rows(a2[g][0]);
            SMX_LDS_BARRIER();
            PSTAMP(si, 2);
            if (tid < 64 * tiles) {
                const int g = tid >> 6;
                float z = red[(g * 4 + kq) * 16 + fm];
#pragma unroll
                for (int w = 1; w < DNWV; ++w) z += red[((w * 2 + g) * 4 + kq) * 16 + fm];
                finish(z, bfin, ft, kq);
            }
        } else {
#pragma unroll 1
            for (int tb = 0; tb < tiles; tb += DNWV * DTG4) {
                const int t0 = tb + wv;
                int nt = (tiles - t0 + DNWV - 1) / DNWV;
                nt = nt < 0 ? 0 : (nt > DTG4 ? DTG4 : nt);
                float bs[DTG4];
#pragma unroll
                for (int g = 0; g < DTG4; ++g) {
                    const int f = 16 * (t0 + DNWV * g) + fm;
                    bs[g] = ld4(rb, (g < nt && f < M) ? (unsigned)f * 4u : OOB);
                }
                f32x4 acc[DTG4];
#pragma unroll
                for (int g = 0; g < DTG4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#define SMX_RUN4(N)                                                                  \
    {                                                                                \
        f32x4 a[N][1];                                                               \
        _Pragma("unroll") for (int g = 0; g < N; ++g) a[g][0] = acc[g];              \
        fwd_tiles4<N, 1>(a, rw, tiles, C2, in, ldi, t0, DNWV, lane);                 \
        _Pragma("unroll") for (int g = 0; g < N; ++g) acc[g] = a[g][0];              \
    }
                if (nt > 3) SMX_RUN4(4)
                else if (nt > 2) SMX_RUN4(3)
                else if (nt > 1) SMX_RUN4(2)
                else if (nt > 0) SMX_RUN4(1)
#undef SMX_RUN4
                if (tb == 0) PSTAMP(si, 1);
                float z[DTG4];
#pragma unroll
                for (int g = 0; g < DTG4; ++g) z[g] = meet_rows(acc[g]);
#pragma unroll
                for (int g = 0; g < DTG4; ++g)
                    if (g < nt) finish(z[g], bs[g], 16 * (t0 + DNWV * g) + fm, kq);      // (wave-uniform)
            }
            PSTAMP(si, 2);
        }
        PSTAMP(si, 3);
        SMX_LDS_BARRIER();
        PSTAMP(si, 4);

        // ---- what follows the layer in its chain ----
        const int post = S.post;
        // LayerNorm: the rules' thread-derived indices and addresses are formed HERE, behind the K loop -- carried across it
        // (as the plain chains carry them) they no longer fit beside the loop's registers
        const int tp = LN ? behind_here(tid) : tid;
        if constexpr (LN) {
            // Linear -> ReLU -> LayerNorm: the rows the layer has just finished, normalised from the pre-LayerNorm tile
            const LnStep& T = ln_late(Q, si);
            if (T.kind == LN_FWD) {
                const LnEmitRows emit = {T.n, T.ldn, T.mean, T.rstd, sm + Q->t.oM + 2 * RB * T.st, row0, nrows, lane};
                ln_rows<RB, DNWV, LNR_MAXC>(sm + T.p_off, T.ldp, sm + T.t_off, T.ldt, T.F, T.gamma, T.beta, Q->t.eps, wv, lane,
                                            emit);
                SMX_LDS_BARRIER();
            }
        }
        if (PHASE == 0) {
            if (post == P_TC_CAT) {            // [h1' | mu'(s')]: the action behind the first c1 columns of the concat tile
                if (tp < RB * A) {
                    const int n = tp / A, j = tp - n * A;
                    sm[G.oC + n * G.ldC + c1 + j] = sm[G.oO + n * LDO + j];
                }
                SMX_LDS_BARRIER();
            } else if (post == P_C_CAT) {      // [h1 | a] and its row-major copy
                if (tp < RB * A) {
                    const int n = tp / A, j = tp - n * A;
                    const float v = (n < nrows) ? G.actions[(size_t)(row0 + n) * A + j] : 0.f;
                    sm[G.oC + n * G.ldC + c1 + j] = v;
                    if (n < nrows) G.xcat[(size_t)(row0 + n) * ldc + c1 + j] = v;
                }
                SMX_LDS_BARRIER();
            } else if (post == P_LOSS) {
                // y = r + gamma^n Q' (1 - done) (ddpg.py:279); dLoss/dQ of the mean squared error (ddpg.py:307-308)
                if (tp < RB) {
                    const float qn = sm[G.oO2 + tp * LDO], q = sm[G.oO + tp * LDO];
                    const float t = (G.gamma_n * qn) * (1.0f - dn);
                    const float yy = rew + t;
                    const float d3 = (2.0f * (q - yy)) / (float)G.rows;
                    sm[G.oS + tp] = (tp < nrows) ? d3 : 0.f;
                    if (tp < nrows) {
                        G.q[row0 + tp] = q;
                        G.q_next[row0 + tp] = qn;
                        G.y[row0 + tp] = yy;
                        G.dz3[row0 + tp] = d3;
                    }
                }
                if (blockIdx.x == 0 && tp == 0 && G.step) *G.step += 1;      // this iteration's Adam step (both groups)
                SMX_LDS_BARRIER();
                // dz2 = (dz3 W3) relu'(h2), a K = 1 product: elementwise
                for (int idx = tp; idx < RB * c2; idx += DNTH) {
                    const int n = idx / c2, j = idx - n * c2;
                    float v = sm[G.oS + n] * G.cW3[j];
                    if constexpr (LN) {              // d/d(LayerNorm 2's output): its backward rule follows below
                        sm[Q->t.oD + n * Q->t.ldD + j] = v;
                        if (n < nrows) Q->t.dn2[(size_t)(row0 + n) * c2 + j] = v;
                    } else {
                        v = (sm[G.oB + n * G.ldB + j] > 0.f) ? v : 0.f;
                        sm[G.oA + n * G.ldA + j] = v;
                        if (n < nrows) G.dz2[(size_t)(row0 + n) * c2 + j] = v;
                    }
                }
                SMX_LDS_BARRIER();
            }
        } else if (PHASE == 2) {
            if (post == P_TC_CAT || post == P_TC2_CAT) {
                // [h1' | mu'(s')] for the first target critic; the second sees the action under the clipped noise:
                // min(max(mu' + noise, -1), 1), an fp32 add then the clamp (ddpg.py:266-283 adds it after Q1' was formed)
                if (tp < RB * A) {
                    const int n = tp / A, j = tp - n * A;
                    float v = sm[G.oO + n * LDO + j];
                    if (post == P_TC2_CAT && G.noise) {
                        const float nz = (n < nrows) ? G.noise[(size_t)(row0 + n) * A + j] : 0.f;
                        v = fminf(fmaxf(v + nz, -1.0f), 1.0f);
                    }
                    sm[G.oC + n * G.ldC + c1 + j] = v;
                }
                SMX_LDS_BARRIER();
            } else if (post == P_C_CAT || post == P_C2_CAT) {      // [h1 | a] and its row-major copy, per critic
                float* xc = post == P_C_CAT ? G.xcat : G.xcat2;
                if (tp < RB * A) {
                    const int n = tp / A, j = tp - n * A;
                    const float v = (n < nrows) ? G.actions[(size_t)(row0 + n) * A + j] : 0.f;
                    sm[G.oC + n * G.ldC + c1 + j] = v;
                    if (n < nrows) xc[(size_t)(row0 + n) * ldc + c1 + j] = v;
                }
                SMX_LDS_BARRIER();
            } else if (post == P_LOSS || post == P_LOSS2) {
                // first critic: y = min(y1, y2) of the two targets, each formed as the one-critic rule forms it (r + t is
                // monotone in Q': the same value as the Bellman target of min(Q1', Q2')); y stays in LDS for the second
                const bool first = post == P_LOSS;
                if (tp < RB) {
                    const float q = sm[G.oO + tp * LDO];
                    float yy;
                    if (first) {
                        const float qn1 = sm[G.oO2 + tp * LDO], qn2 = sm[G.oO3 + tp * LDO];
                        const float t1 = (G.gamma_n * qn1) * (1.0f - dn), t2 = (G.gamma_n * qn2) * (1.0f - dn);
                        const float y1 = rew + t1, y2 = rew + t2;
                        yy = fminf(y1, y2);
                        sm[G.oY + tp] = yy;
                        if (tp < nrows) {
                            G.q_next[row0 + tp] = qn1;
                            G.q_next2[row0 + tp] = fminf(qn1, qn2);
                            G.y[row0 + tp] = yy;
                        }
                    } else {
                        yy = sm[G.oY + tp];
                    }
                    const float d3 = (2.0f * (q - yy)) / (float)G.rows;
                    sm[G.oS + tp] = (tp < nrows) ? d3 : 0.f;
                    if (tp < nrows) {
                        (first ? G.q : G.q2)[row0 + tp] = q;
                        (first ? G.dz3 : G.dz3_2)[row0 + tp] = d3;
                    }
                }
                if (first && blockIdx.x == 0 && tp == 0 && G.step) *G.step += 1;      // ONE Adam step count for all groups
                SMX_LDS_BARRIER();
                const float* W3 = first ? G.cW3 : G.c2W3;
                float* dz2 = first ? G.dz2 : G.dz2_2;
                for (int idx = tp; idx < RB * c2; idx += DNTH) {
                    const int n = idx / c2, j = idx - n * c2;
                    float v = sm[G.oS + n] * W3[j];
                    if constexpr (LN) {              // d/d(LayerNorm 2's output) of this critic: its backward rule follows
                        sm[Q->t.oD + n * Q->t.ldD + j] = v;
                        if (n < nrows) (first ? Q->t.dn2 : Q->t.dn2_2)[(size_t)(row0 + n) * c2 + j] = v;
                    } else {
                        v = (sm[G.oB + n * G.ldB + j] > 0.f) ? v : 0.f;
                        sm[G.oA + n * G.ldA + j] = v;
                        if (n < nrows) dz2[(size_t)(row0 + n) * c2 + j] = v;
                    }
                }
                SMX_LDS_BARRIER();
            }
        } else {
            if (post == P_A_CAT) {
                if (tp < RB * A) {
                    const int n = tp / A, j = tp - n * A;
                    sm[G.oC + n * G.ldC + c1 + j] = sm[G.oO + n * LDO + j];
                }
                SMX_LDS_BARRIER();
            } else if (post == P_A_DQ) {
                // the masks of the actor's backward pass (its forward pass ran in the critic phase): h1a -> the concat
                // tile, whose layer-2 product is done; h2a follows once dz2 has read the critic's ReLU mask
                if constexpr (!LN) stage_rows(G.h1a, G.H1, G.H1, row0, nrows, G.oC, G.ldC);
                const float dq = -1.0f / (float)G.rows;            // d(-mean Q)/d(h2) = (-1/rows) W3 relu'(h2)
                for (int idx = tp; idx < RB * c2; idx += DNTH) {
                    const int n = idx / c2, j = idx - n * c2;
                    float v = dq * G.cW3[j];
                    if constexpr (LN) {              // d/d(LayerNorm 2's output) of the critic, as in the critic chain
                        sm[Q->t.oD + n * Q->t.ldD + j] = (n < nrows) ? v : 0.f;
                    } else {
                        v = (n < nrows && sm[G.oB + n * G.ldB + j] > 0.f) ? v : 0.f;
                        sm[G.oA + n * G.ldA + j] = v;
                    }
                }
                SMX_LDS_BARRIER();
                if constexpr (!LN) stage_rows(G.h2a, G.H2, G.H2, row0, nrows, G.oB, G.ldB);
            } else if (post == P_A_TANH) {     // through tanh: the action gradient times 1 - a^2
                if (tp < RB * A) {
                    const int n = tp / A, j = tp - n * A;
                    const float a = sm[G.oO + n * LDO + j];
                    const float v = sm[G.oO2 + n * LDO + j] * (1.0f - a * a);
                    sm[G.oZ + n * LDK4 + j] = v;
                    if (n < nrows) G.dz3a[(size_t)(row0 + n) * A + j] = v;
                }
                SMX_LDS_BARRIER();
            }
        }
        if constexpr (LN) {
            const LnStep& T = ln_late(Q, si);
            if (T.kind == LN_BWD) {
                ln_bwd_rows(sm + T.d_off, T.ldd, sm + T.p_off, T.ldp, sm + Q->t.oM + 2 * RB * T.st, T.F, T.gamma,
                            T.t_off >= 0 ? sm + T.t_off : nullptr, T.ldt, T.n, T.ldn, row0, nrows, wv, lane);
                SMX_LDS_BARRIER();
                if (PHASE == 1 && post == P_A_DQ) {
                    // the actor's backward pass (its forward pass ran in the critic phase): its pre-LayerNorm rows and
                    // statistics into the tiles and slots the critic's LayerNorms are done with (the barriers of the next
                    // step stand between this and the rules that read them)
                    stage_rows(Q->t.a1, G.H1, G.H1, row0, nrows, Q->t.oP1, Q->t.ldP1);
                    stage_rows(Q->t.a2, G.H2, G.H2, row0, nrows, Q->t.oP2, Q->t.ldP2);
                    if (tp < 4 * RB) {
                        const int w = tp >> 2, n = tp & 3;       // (am1, ar1, am2, ar2) -> slots 2, 3
                        const float* src = w == 0 ? Q->t.am1 : w == 1 ? Q->t.ar1 : w == 2 ? Q->t.am2 : Q->t.ar2;
                        sm[Q->t.oM + 4 * RB + RB * w + n] = (n < nrows) ? src[row0 + n] : 0.f;
                    }
                }
            }
        }
        TSTAMP(si + 1);
    }
}

template <int PHASE>
__global__ __launch_bounds__(DNTH) void ddpg_rows4_kernel(RArgs G, Prog P) {
    ddpg_rows4_chain<PHASE, false>(G, P, (const LnProgT<LN_STEPS>*)nullptr);
}

template <int PHASE>
__global__ __launch_bounds__(DNTH) void ddpg_rows4_ln_kernel(RArgs G, Prog P,
                                                             LnProgT<PHASE == 2 ? LN_STEPS_TD3 : LN_STEPS> Q) {
    ddpg_rows4_chain<PHASE, true>(G, P, &Q);
}

// ---------------------------------------------------------------------------------------------------------------
// the packed copies: one thread per 16-byte word of [tile][chunk][half][lane][4]
// ---------------------------------------------------------------------------------------------------------------
constexpr int N_MAT = 16;
struct PItem {
    const float* src;
    int ld, M, K, tr;             // X[m][k] = tr ? src[k ld + m] : src[m ld + k]
    long base;                    // first 16-byte word of the block in the packed buffer
};
struct PArgs {
    PItem it[N_MAT];
    float* packed;
    int count;
    long total;                   // words covered by the launch (items are contiguous from it[0].base)
};

__global__ __launch_bounds__(256) void ddpg_pack_kernel(PArgs P) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.total) return;
    const long w0 = i + P.it[0].base;
    int pi = 0;
#pragma unroll
    for (int k = 1; k < N_MAT; ++k) pi += (k < P.count && w0 >= P.it[k].base) ? 1 : 0;
    const PItem N = P.it[pi];
    const long w = w0 - N.base;
    const int C2 = pack_chunks(N.K);
    const int lane = (int)(w & 63), half = (int)((w >> 6) & 1);
    const long tc = w >> 7;
    const int c = (int)(tc % C2), t = (int)(tc / C2);
    const int m = 16 * t + (lane & 15), k = 32 * c + 8 * (lane >> 4) + 4 * half;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (m < N.M) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (k + r < N.K) v[r] = N.tr ? N.src[(size_t)(k + r) * N.ld + m] : N.src[(size_t)m * N.ld + k + r];
    }
    *(float4*)(P.packed + 4 * w0) = make_float4(v[0], v[1], v[2], v[3]);
}

// beta^n for Adam's bias corrections by repeated squaring: ~40 double multiplications instead of pow()'s several hundred
// instructions -- the two powers were 3 us of ONE lane with the whole launch waiting behind it (phase stamps: 7 k cycles
// at the barrier).  Within a few ulp of pow's double result; the coefficients are rounded to float afterwards.
__device__ __forceinline__ double ipow(double b, int n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
// one optimiser group's step for the row schedule: Adam (smx_adam_step_dev_f32's expressions), the target update of the
// group's target network (smx_soft_update_f32 / smx_hard_update_every_f32's) and BOTH fragment-order copies, element by
// element in one launch -- the schedule's two pack launches and its target-update launch (12 + 4 us of a 135 us
// iteration) disappear.  Nothing reads the target critic between the critic's Adam step and the end of the iteration
// (the actor phase goes through the MODEL critic), so updating it here forms the same values as ddpg.py:344-352 does at
// the end.
// ---------------------------------------------------------------------------------------------------------------
struct UMat {
    long off;                     // first element of the matrix inside the group's buffer
    int M, K;                     // [M, K] row-major
    long base, base_tgt;          // packed blocks (float offsets): the model's copy, the target's
    long base_t0, base_t1;        // transposed copies (< 0: none): columns < split -> t0, the rest -> t1
    int split;
};
struct UArgs {
    float* theta;
    const float* grads;
    float* grads_out;             // the fused weight-gradient launch writes the gradient it steps with here
    float *m, *v, *target, *packed;
    long n;
    const float* lr;
    const int* step;
    float wd, clip_value, tau;
    int interval;
    UMat mat[3];
};

__global__ __launch_bounds__(256) void ddpg_rows_update_kernel(UArgs U) {
    __shared__ float coef[2];
    __shared__ int upd;
    if (threadIdx.x == 0) {
        const int st = *U.step;
        const double bc1 = 1.0 - ipow(0.9, st), bc2 = 1.0 - ipow(0.999, st);
        coef[0] = (float)(-((double)*U.lr / bc1));
        coef[1] = (float)sqrt(bc2);
        upd = U.interval > 0 ? (st % U.interval == 0) : 1;
    }
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= U.n) return;
    const float neg_step_size = coef[0], bc2_sqrt = coef[1];
    const float w1 = (float)(1.0 - 0.9), b2f = (float)0.999, w2 = (float)(1.0 - 0.999), eps = 1e-8f;
    float g = U.grads[i];
    if (U.clip_value > 0.f && g == g) g = fminf(fmaxf(g, -U.clip_value), U.clip_value);   // clip_grad_value_
    const float p = U.theta[i];
    if (U.wd != 0.f) g = g + U.wd * p;
    float mi = U.m[i], vi = U.v[i];
    mi = mi + w1 * (g - mi);
    vi = vi * b2f + w2 * (g * g);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float pn = p + (neg_step_size * mi) / denom;
    U.theta[i] = pn;
    U.m[i] = mi;
    U.v[i] = vi;
    // the target network's element (torchx Module.soft_update: target * (1 - tau) + source * tau; a hard update copies)
    bool tw = false;
    float tn = 0.f;
    if (U.target && upd) {
        tn = (U.interval > 0 || U.tau >= 1.0f) ? pn : (U.target[i] * (1.0f - U.tau) + pn * U.tau);
        U.target[i] = tn;
        tw = true;
    }
    // the fragment-order copies
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const UMat& X = U.mat[j];
        const long r = i - X.off;
        if (r >= 0 && r < (long)X.M * X.K) {
            const int mm = (int)(r / X.K), kk = (int)(r - (long)mm * X.K);
            const long pos = pack_pos(X.K, mm, kk);
            U.packed[X.base + pos] = pn;
            if (tw) U.packed[X.base_tgt + pos] = tn;
            if (kk < X.split) {
                if (X.base_t0 >= 0) U.packed[X.base_t0 + pack_pos(X.M, kk, mm)] = pn;
            } else if (X.base_t1 >= 0) {
                U.packed[X.base_t1 + pack_pos(X.M, kk - X.split, mm)] = pn;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The group's weight gradients AND its step in one launch (single rank): dW = dz^T x and db = column sums of dz over the
// batch rows, then -- the gradient still in the accumulators -- the element's Adam step, target update and packed copies
// as in ddpg_rows_update_kernel (value clipping is elementwise: no norm over the group is needed first, which is what keeps
// PPO's clip-norm step a launch of its own).  Replaces smx_linear_multi_f32 (9 us at batch 512) + the update launch (6 us)
// and the gap between them.
//
// A workgroup owns a 32 x 32 tile of one matrix: wave w forms ALL of it over the w-th eighth of the rows on
// v_mfma_f32_16x16x4 (four quadrant accumulators; lane (i, g): a = dz[k + g][m0 + i], b = x[k + g][n0 + i], four rows
// per instruction), the operands of its 64 rows requested at once; the eight partial tiles meet through LDS in row order
// and every thread steps two elements.  Another summation order than smx_linear_wgrad_f32's: equal within fp32 rounding.
// ---------------------------------------------------------------------------------------------------------------
struct WMat {
    const float* dz;              // [rows][M], row stride ldz
    const float* x;               // [rows][N], row stride ldx
    int ldz, ldx, tiles_n, tile0; // tile0: first workgroup of this matrix
    long boff;                    // the bias [M] inside the group's buffer
};
struct WLn {                      // dgamma = sum_rows dn xhat, dbeta = sum_rows dn of one LayerNorm
    const float *dn, *pre, *mean, *rstd;      // [rows][lddn], [rows][ldp] (in front of the LayerNorm), [rows] x 2
    int lddn, ldp, F, blk0;       // blk0: the LayerNorm's first workgroup among the ln_blocks
    long goff, boff;              // gamma [F], beta [F] inside the group's buffer
};
struct WUArgs {
    UArgs U;
    WMat w[3];
    int rows;
    // optional: the iteration's statistics as one more workgroup of this launch (the last one of the iteration)
    float* stats;
    float* stats_host;            // host-mapped mirror, two slots of 8 floats: slot *step & 1 (of 16 with a second critic)
    float* stats2;                // TD3: a second block, as smx_ddpg_stats_f32 forms it for (q2, y)
    const float* s_q2;
    const float *s_q, *s_y, *s_rewards, *s_actions, *s_q_actor;
    int s_A, tiles;
    long long* tbuf;              // SMX_DDPG_TIMING builds
    // LayerNorm: the group's two gain / bias pairs as ln_blocks further workgroups behind the tiles (0: none)
    WLn ln[2];
    int ln_blocks;
};
#ifdef SMX_DDPG_TIMING
#define WSTAMP(i) do { if (G.tbuf && threadIdx.x == 0) G.tbuf[(size_t)blockIdx.x * 128 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define WSTAMP(i) do { } while (0)
#endif

#define MFMA16W(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ void ddpg_step_element(const UArgs& U, long i, float g, float p, float mi, float vi, float tg,
                                                  float neg_step_size, float bc2_sqrt, int upd, float& pn, float& tn,
                                                  bool& tw) {
    const float w1 = (float)(1.0 - 0.9), b2f = (float)0.999, w2 = (float)(1.0 - 0.999), eps = 1e-8f;
    if (U.clip_value > 0.f && g == g) g = fminf(fmaxf(g, -U.clip_value), U.clip_value);
    if (U.wd != 0.f) g = g + U.wd * p;
    mi = mi + w1 * (g - mi);
    vi = vi * b2f + w2 * (g * g);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pn = p + (neg_step_size * mi) / denom;
    U.theta[i] = pn;
    U.m[i] = mi;
    U.v[i] = vi;
    tw = false;
    tn = 0.f;
    if (U.target && upd) {
        tn = (U.interval > 0 || U.tau >= 1.0f) ? pn : (tg * (1.0f - U.tau) + pn * U.tau);
        U.target[i] = tn;
        tw = true;
    }
}

constexpr int WNW = 8;            // waves per tile: wave w takes the w-th eighth of the rows, the WHOLE 32 x 32 tile
constexpr int WUB = 16;           // steps (of four rows) a wave requests at once: 64 rows, 64 loads in flight
constexpr int LNC = 16;           // columns of a LayerNorm's gain and bias per workgroup
constexpr int LUB = 8;            // steps (of four rows) one of its waves requests at once

// A LayerNorm's parameter gradients and their step: a workgroup owns LNC columns; wave w sums the w-th eighth of the rows
// (the tiles' qrows split), lane (i, g) the rows k + g of column i, four rows a step and LUB steps requested at once; the
// four row phases meet by meet_kq1, the eight waves through LDS in wave order (no atomics: a fixed order).  xhat is formed
// from the pre-LayerNorm buffer, mean and rstd as layernorm_bwd_kernel forms it.  Threads 0 .. 2 LNC - 1 then step
// gamma's and beta's elements.
__device__ __forceinline__ void ddpg_ln_pgrad_block(const WUArgs& G, int b, float* part, float* coef, int* upd_s) {
    const UArgs& U = G.U;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const WLn W = G.ln[b >= G.ln[1].blk0 ? 1 : 0];
    const int col = LNC * (b - W.blk0) + i;
    const bool ok = col < W.F;
    const int rows = G.rows;
    const int qrows = ((rows + 4 * WNW - 1) / (4 * WNW)) << 2;
    const int k_lo = wv * qrows;
    int k_hi = k_lo + qrows;
    k_hi = k_hi < rows ? k_hi : rows;
    // the element this thread steps: which = 0 gamma, 1 beta
    const int which = tid >> 4, ci = LNC * (b - W.blk0) + (tid & 15);
    const bool eok = tid < 2 * LNC && ci < W.F;
    const long ei = eok ? (which ? W.boff : W.goff) + ci : W.goff;
    const float ep = U.theta[ei], em = U.m[ei], ev = U.v[ei], et = U.target ? U.target[ei] : 0.f;
    if (tid == 64 * (WNW - 1)) {
        const int st = *U.step;
        const double bc1 = 1.0 - ipow(0.9, st), bc2 = 1.0 - ipow(0.999, st);
        coef[0] = (float)(-((double)*U.lr / bc1));
        coef[1] = (float)sqrt(bc2);
        *upd_s = U.interval > 0 ? (st % U.interval == 0) : 1;
    }
    // addressing as the tiles': the lane's part a vector offset formed once, the step's rows a scalar offset; the
    // descriptors end at the wave's last row, so a row past k_hi (or a column past F: OOB) loads 0
    const unsigned kb = (unsigned)(k_hi > 0 ? k_hi : 0);
    const rsrc_t rd = make_rsrc(W.dn, kb * (unsigned)W.lddn * 4u), rx = make_rsrc(W.pre, kb * (unsigned)W.ldp * 4u);
    const rsrc_t rm = make_rsrc(W.mean, kb * 4u), rr = make_rsrc(W.rstd, kb * 4u);
    const unsigned vd = ok ? ((unsigned)g * (unsigned)W.lddn + (unsigned)col) * 4u : OOB;
    const unsigned vx = ok ? ((unsigned)g * (unsigned)W.ldp + (unsigned)col) * 4u : OOB;
    const unsigned vs = ok ? (unsigned)g * 4u : OOB;
#define SMX_LDL(R, v, k, sb) __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(R, v, (unsigned)(k) * (sb), 0))
    float ag = 0.f, ab = 0.f;
#pragma unroll 1
    for (int k = k_lo; k < k_hi; k += 4 * LUB) {
        float d[LUB], x[LUB], m[LUB], rs[LUB];
#pragma unroll
        for (int u = 0; u < LUB; ++u) {
            d[u] = SMX_LDL(rd, vd, k + 4 * u, 4u * (unsigned)W.lddn);
            x[u] = SMX_LDL(rx, vx, k + 4 * u, 4u * (unsigned)W.ldp);
            m[u] = SMX_LDL(rm, vs, k + 4 * u, 4u);
            rs[u] = SMX_LDL(rr, vs, k + 4 * u, 4u);
        }
#pragma unroll
        for (int u = 0; u < LUB; ++u) {
            const float xh = (x[u] - m[u]) * rs[u];
            ag += d[u] * xh;
            ab += d[u];
        }
    }
#undef SMX_LDL
    ag = meet_kq1(ag);
    ab = meet_kq1(ab);
    if (g == 0) { part[(wv * 2 + 0) * LNC + i] = ag; part[(wv * 2 + 1) * LNC + i] = ab; }
    __syncthreads();
    if (eok) {
        float gsum = part[(0 * 2 + which) * LNC + (tid & 15)];
#pragma unroll
        for (int w = 1; w < WNW; ++w) gsum += part[(w * 2 + which) * LNC + (tid & 15)];      // the waves' row ranges in order
        U.grads_out[ei] = gsum;
        float pn, tn;
        bool tw;
        ddpg_step_element(U, ei, gsum, ep, em, ev, et, coef[0], coef[1], *upd_s, pn, tn, tw);
    }
}

__global__ __launch_bounds__(64 * WNW) void ddpg_rows_wgrad_update_kernel(WUArgs G) {
    __shared__ float red[WNW][4][64][4];            // every wave's four quadrant accumulators (32 KB)
    __shared__ float redb[WNW][32];                 // ... and its column sums of dz
    __shared__ float coef[2];
    __shared__ int upd_s;
    const UArgs& U = G.U;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    if ((int)blockIdx.x >= G.tiles) {               // behind the last tile: the LayerNorms' workgroups, then the statistics
        if ((int)blockIdx.x < G.tiles + G.ln_blocks) {
            ddpg_ln_pgrad_block(G, (int)blockIdx.x - G.tiles, &red[0][0][0][0], coef, &upd_s);
            return;
        }
        float* mirror = G.stats_host ? G.stats_host + (G.stats2 ? 16 : 8) * (*G.U.step & 1) : nullptr;
        ddpg_stats_block<64 * WNW>(G.s_q, G.s_y, G.s_rewards, G.s_actions, G.s_A, G.s_A, G.s_q_actor, (long)G.rows, G.stats,
                                   mirror);
        if (G.stats2)
            ddpg_stats_block<64 * WNW>(G.s_q2, G.s_y, G.s_rewards, G.s_actions, G.s_A, G.s_A, G.s_q2, (long)G.rows, G.stats2,
                                       mirror ? mirror + 8 : nullptr);
        return;
    }
    WSTAMP(0);
    // consecutive workgroup ids land on the eight XCDs round-robin, each with its own L2: XCD x takes the x-th contiguous
    // eighth of the tile list (tiles are row-major in M: a band of dz columns and all of x) instead of every eighth tile,
    // or all eight L2s pull every operand across the fabric (as smx_gemm.hip's gemm32 does)
    int bid = blockIdx.x;
    {
        const int total = G.tiles, qd = total >> 3, rem = total & 7;
        const int xcd = bid & 7, slot = bid >> 3;
        bid = (xcd < rem ? xcd * (qd + 1) : rem * (qd + 1) + (xcd - rem) * qd) + slot;
    }
    const int j = (bid >= G.w[2].tile0) ? 2 : (bid >= G.w[1].tile0) ? 1 : 0;
    const WMat W = G.w[j];
    const UMat X = U.mat[j];
    const int tile = bid - W.tile0;
    const int tm = tile / W.tiles_n, tn_ = tile - tm * W.tiles_n;
    const int m0 = 32 * tm, n0 = 32 * tn_;
    const int rows = G.rows;
    const int qrows = ((rows + 4 * WNW - 1) / (4 * WNW)) << 2;      // rows per wave (a multiple of four)
    const int k_lo = wv * qrows;
    int k_hi = k_lo + qrows;
    k_hi = k_hi < rows ? k_hi : rows;
    // addressing: the lane's part (row g of a step, its column) is a vector offset formed ONCE, the step's rows a SCALAR
    // offset -- no vector instruction between the loads.  The descriptors end at the wave's last row: the range check
    // counts the scalar offset in, so a row past k_hi (or a column past the matrix: OOB) loads 0.
    const rsrc_t rzk = make_rsrc(W.dz, (unsigned)(k_hi > 0 ? k_hi : 0) * (unsigned)W.ldz * 4u);
    const rsrc_t rxk = make_rsrc(W.x, (unsigned)(k_hi > 0 ? k_hi : 0) * (unsigned)W.ldx * 4u);
    const unsigned gz = (unsigned)g * (unsigned)W.ldz, gx = (unsigned)g * (unsigned)W.ldx;
    const unsigned vz0 = (m0 + i < X.M) ? (gz + (unsigned)(m0 + i)) * 4u : OOB;
    const unsigned vz1 = (m0 + 16 + i < X.M) ? (gz + (unsigned)(m0 + 16 + i)) * 4u : OOB;
    const unsigned vx0 = (n0 + i < X.K) ? (gx + (unsigned)(n0 + i)) * 4u : OOB;
    const unsigned vx1 = (n0 + 16 + i < X.K) ? (gx + (unsigned)(n0 + 16 + i)) * 4u : OOB;
    const unsigned sz = 16u * (unsigned)W.ldz, sx = 16u * (unsigned)W.ldx;      // bytes per step of four rows
#define SMX_LDW(R, v, k, sb) __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(R, v, (unsigned)(k) / 4u * (sb), 0))
    // Every wave forms the whole tile over ITS rows: a step is four loads (two halves of the dz columns, two of the x
    // columns: each 64-byte segment is requested once per workgroup) for four products.  As quadrant waves over half the
    // rows each segment was requested twice and the launch waited on its 4096 requests per workgroup (phase stamps: the
    // last wave's operands arrived 17 k cycles in).
    float a0[WUB], a1[WUB], b0[WUB], b1[WUB];
#pragma unroll
    for (int u = 0; u < WUB; ++u) {
        a0[u] = SMX_LDW(rzk, vz0, k_lo + 4 * u, sz); a1[u] = SMX_LDW(rzk, vz1, k_lo + 4 * u, sz);
        b0[u] = SMX_LDW(rxk, vx0, k_lo + 4 * u, sx); b1[u] = SMX_LDW(rxk, vx1, k_lo + 4 * u, sx);
    }
    WSTAMP(1);
    // the two elements this THREAD steps once the waves' sums have met: (ml, nl) and (ml + 16, nl) of the tile, threads
    // along n (coalesced); their parameters and moments are requested behind the operands
    const int ml = tid >> 5, nl = tid & 31;
    long ei[2];
    float p2[2], m2[2], v2[2], t2[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int m = m0 + ml + 16 * e, n = n0 + nl;
        const bool ok = m < X.M && n < X.K;
        ei[e] = ok ? X.off + (long)m * X.K + n : -1;
        const long c = ok ? ei[e] : X.off;
        p2[e] = U.theta[c]; m2[e] = U.m[c]; v2[e] = U.v[c];
        t2[e] = U.target ? U.target[c] : 0.f;
    }
    // the bias of row m0 + tid (column tile 0, the first 32 threads)
    const bool bok = tn_ == 0 && tid < 32 && m0 + tid < X.M;
    const long bi = bok ? W.boff + m0 + tid : W.boff;
    const float bp = U.theta[bi], bm = U.m[bi], bv = U.v[bi], bt = U.target ? U.target[bi] : 0.f;
    if (tid == 64 * (WNW - 1)) {                    // Adam's bias corrections, while the loads are on their way
        const int st = *U.step;
        const double bc1 = 1.0 - ipow(0.9, st), bc2 = 1.0 - ipow(0.999, st);
        coef[0] = (float)(-((double)*U.lr / bc1));
        coef[1] = (float)sqrt(bc2);
        upd_s = U.interval > 0 ? (st % U.interval == 0) : 1;
    }
    f32x4 acc[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) acc[qq] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float as0 = 0.f, as1 = 0.f;
    WSTAMP(2);
#pragma unroll 1
    for (int k = k_lo; k < k_hi; k += 4 * WUB) {
#pragma unroll
        for (int u = 0; u < WUB; ++u) {
            acc[0] = MFMA16W(a0[u], b0[u], acc[0]);
            acc[1] = MFMA16W(a0[u], b1[u], acc[1]);
            acc[2] = MFMA16W(a1[u], b0[u], acc[2]);
            acc[3] = MFMA16W(a1[u], b1[u], acc[3]);
            as0 += a0[u];
            as1 += a1[u];
        }
        if (k + 4 * WUB < k_hi) {                   // (more than 512 rows: the next 64 of this wave's)
#pragma unroll
            for (int u = 0; u < WUB; ++u) {
                a0[u] = SMX_LDW(rzk, vz0, k + 4 * (WUB + u), sz); a1[u] = SMX_LDW(rzk, vz1, k + 4 * (WUB + u), sz);
                b0[u] = SMX_LDW(rxk, vx0, k + 4 * (WUB + u), sx); b1[u] = SMX_LDW(rxk, vx1, k + 4 * (WUB + u), sx);
            }
        }
    }
#undef SMX_LDW
    WSTAMP(3);
    // quadrant qq = 2 (m half) + (n half): lane (i, g) holds rows 16 (qq >> 1) + 4 g + r, column 16 (qq & 1) + i
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) *(f32x4*)&red[wv][qq][lane][0] = acc[qq];
    as0 = meet_kq1(as0);                            // every lane of column i: the sum over this wave's rows
    as1 = meet_kq1(as1);
    if (g == 0) { redb[wv][i] = as0; redb[wv][16 + i] = as1; }
    __syncthreads();
    WSTAMP(4);
    const float neg_step_size = coef[0], bc2_sqrt = coef[1];
    const int upd = upd_s;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (ei[e] >= 0) {
            const int mm = ml + 16 * e;                                       // (inside the tile)
            const int qq = ((mm >> 4) << 1) | (nl >> 4), ln = 16 * ((mm & 15) >> 2) + (nl & 15), r = mm & 3;
            float gsum = red[0][qq][ln][r];
#pragma unroll
            for (int w = 1; w < WNW; ++w) gsum += red[w][qq][ln][r];          // the waves' row ranges in order
            U.grads_out[ei[e]] = gsum;
            float pn, tn;
            bool tw;
            ddpg_step_element(U, ei[e], gsum, p2[e], m2[e], v2[e], t2[e], neg_step_size, bc2_sqrt, upd, pn, tn, tw);
            const int gm = m0 + mm, kk = n0 + nl;
            const long pos = pack_pos(X.K, gm, kk);
            U.packed[X.base + pos] = pn;
            if (tw) U.packed[X.base_tgt + pos] = tn;
            if (kk < X.split) {
                if (X.base_t0 >= 0) U.packed[X.base_t0 + pack_pos(X.M, kk, gm)] = pn;
            } else if (X.base_t1 >= 0) {
                U.packed[X.base_t1 + pack_pos(X.M, kk - X.split, gm)] = pn;
            }
        }
    }
    if (bok) {
        float gb = redb[0][tid];
#pragma unroll
        for (int w = 1; w < WNW; ++w) gb += redb[w][tid];
        U.grads_out[bi] = gb;
        float pn, tn;
        bool tw;
        ddpg_step_element(U, bi, gb, bp, bm, bv, bt, neg_step_size, bc2_sqrt, upd, pn, tn, tw);
    }
    WSTAMP(5);
}

// block order of the packed buffer
enum { B_AW1, B_AW2, B_AW3, B_AW3T, B_AW2T, B_CW1, B_CW2, B_CW3, B_CW2TLO, B_CW2THI, B_TAW1, B_TAW2, B_TAW3, B_TCW1,
       B_TCW2, B_TCW3, B_COUNT };
static_assert(B_COUNT == N_MAT, "one item per block");

struct Dims { int D, A, H1, H2, c1, c2; };

void block_shape(const Dims& d, int b, int& M, int& K) {
    switch (b) {
        case B_AW1: case B_TAW1: M = d.H1; K = d.D; break;
        case B_AW2: case B_TAW2: M = d.H2; K = d.H1; break;
        case B_AW3: case B_TAW3: M = d.A; K = d.H2; break;
        case B_AW3T: M = d.H2; K = d.A; break;
        case B_AW2T: M = d.H1; K = d.H2; break;
        case B_CW1: case B_TCW1: M = d.c1; K = d.D; break;
        case B_CW2: case B_TCW2: M = d.c2; K = d.c1 + d.A; break;
        case B_CW3: case B_TCW3: M = 1; K = d.c2; break;
        case B_CW2TLO: M = d.c1; K = d.c2; break;
        default: M = d.A; K = d.c2; break;       // B_CW2THI
    }
}

// the second critic's blocks (TD3) live in a buffer of their own, so the sixteen above stay where they are.  No W2^T hi:
// nothing differentiates the second critic with respect to the action
enum { B2_CW1, B2_CW2, B2_CW3, B2_CW2TLO, B2_TCW1, B2_TCW2, B2_TCW3, B2_COUNT };

// A packed buffer: its blocks in order, each with the shape of one of the sixteen
struct Layout {
    const int* as_first;          // block b has the shape of block as_first[b] of the first buffer
    int count;
    void shape(const Dims& d, int b, int& M, int& K) const { block_shape(d, as_first[b], M, K); }
    long base(const Dims& d, int b) const {      // in 16-byte words; b == count: the buffer's size
        long o = 0;
        for (int k = 0; k < b; ++k) {
            int M, K;
            shape(d, k, M, K);
            o += pack_words(M, K);
        }
        return o;
    }
    PMat pmat(const Dims& d, const float* packed, int b) const {
        PMat m;
        shape(d, b, m.M, m.K);
        m.P = packed + 4 * base(d, b);
        return m;
    }
};
const int first_as_first[B_COUNT] = {B_AW1, B_AW2, B_AW3, B_AW3T, B_AW2T, B_CW1, B_CW2, B_CW3, B_CW2TLO, B_CW2THI,
                                     B_TAW1, B_TAW2, B_TAW3, B_TCW1, B_TCW2, B_TCW3};
const int second_as_first[B2_COUNT] = {B_CW1, B_CW2, B_CW3, B_CW2TLO, B_TCW1, B_TCW2, B_TCW3};      // (same shapes)
const Layout L_FIRST = {first_as_first, B_COUNT}, L_SECOND = {second_as_first, B2_COUNT};
// W1, W2, W3 of the networks: actor, critic, their targets in `packed`; the second critic and its target in `packed2`
const int NET_W[4][3] = {{B_AW1, B_AW2, B_AW3}, {B_CW1, B_CW2, B_CW3}, {B_TAW1, B_TAW2, B_TAW3}, {B_TCW1, B_TCW2, B_TCW3}};
const int NET2_W[2][3] = {{B2_CW1, B2_CW2, B2_CW3}, {B2_TCW1, B2_TCW2, B2_TCW3}};

long long* g_tbuf = nullptr;

inline int imax(int a, int b) { return a > b ? a : b; }

// The chains' LDS carve-up (float offsets, into G and Q where given) -> its size.  With LayerNorm tile A is wide enough
// for either network's rows (the networks take turns in tiles A and B), and behind the plain regions come the two
// pre-LayerNorm tiles (layer 1's, layer 2's: kept for the backward rules beside the LayerNorm outputs), the dn tile and
// four statistics slots of (mean [4], rstd [4]).  TD3's y, kept between the two critics' losses, sits in front of the
// prefetch pad in the plain carve and at the very end in the LayerNorm one.
int lds_floats(const Dims& d, bool td3, bool ln, RArgs* G = nullptr, LnProg* Q = nullptr) {
    constexpr int RB = RBLK;
    const int pad = 16;             // row strides = 16 mod 64: the 16 (row, kq) readers of the 4-row loop on distinct banks
    const int ldx = r64(d.D) + pad;
    const int wa = imax(imax(d.H1, d.c2), ln ? d.H2 : 0), wb = imax(d.H2, d.c2), wc = imax(d.c1 + d.A, d.H1);
    const int ldA = r64(wa) + pad, ldB = r64(wb) + pad, ldC = r64(wc) + pad;
    const int ldP1 = r64(imax(d.H1, d.c1)) + pad, ldP2 = r64(imax(d.H2, d.c2)) + pad;
    const int ldD = r64(imax(imax(d.H1, d.H2), imax(d.c1, d.c2))) + pad;
    const int ny = td3 ? 16 : 0;
    int o = 0;
    const int oX = o; o += RB * ldx;
    const int oXn = o; o += RB * ldx;
    const int oA = o; o += RB * ldA;
    const int oB = o; o += RB * ldB;
    const int oC = o; o += RB * ldC;
    const int oO = o; o += RB * LDO;
    const int oO2 = o; o += RB * LDO;
    const int oO3 = o; o += RB * LDO;
    const int oZ = o; o += RB * LDK4;
    const int oS = o; o += 16;
    const int oR = o; o += DNWV * 2 * 4 * 16;      // the split-K layers' partial sums
    int oY = o; o += ln ? 0 : ny;
    o += 128;                     // the K loop's prefetch reads up to two chunks past a tile's last row
    int oP1 = 0, oP2 = 0, oD = 0, oM = 0;
    if (ln) {
        oP1 = o; o += RB * ldP1;
        oP2 = o; o += RB * ldP2;
        oD = o; o += RB * ldD;
        oM = o; o += 4 * 2 * RB;
        oY = o; o += ny;
    }
    if (G) {
        G->ldx = ldx; G->ldA = ldA; G->ldB = ldB; G->ldC = ldC;
        G->oX = oX; G->oXn = oXn; G->oA = oA; G->oB = oB; G->oC = oC; G->oO = oO; G->oO2 = oO2; G->oO3 = oO3;
        G->oZ = oZ; G->oS = oS; G->oR = oR; G->oY = oY; G->total = o;
    }
    if (Q) {
        Q->t.oP1 = oP1; Q->t.ldP1 = ldP1; Q->t.oP2 = oP2; Q->t.ldP2 = ldP2; Q->t.oD = oD; Q->t.ldD = ldD; Q->t.oM = oM;
    }
    return o;
}

// (a LayerNorm shape must fit the plain carve as well: dims_ok_ln adds its own to dims_ok's)
bool dims_ok(const Dims& d, bool td3 = false) {
    return d.D > 0 && d.A > 0 && d.A <= 32 && d.H1 > 0 && d.H2 > 0 && d.c1 > 0 && d.c2 > 0 && d.D <= 2048 &&
           d.H1 % 4 == 0 && d.H2 % 4 == 0 && d.c1 % 4 == 0 && d.c2 % 4 == 0 && d.H1 <= 1024 && d.H2 <= 1024 &&
           d.c1 <= 1024 && d.c2 <= 1024 && lds_floats(d, td3, false) * (int)sizeof(float) <= MAX_LDS;
}
bool dims_ok_ln(const Dims& d, bool td3 = false) {
    return dims_ok(d, td3) && lds_floats(d, td3, true) * (int)sizeof(float) <= MAX_LDS;
}

Dims dims_of(const smx_ddpg_rows_t& a) { return Dims{a.D, a.A, a.H1, a.H2, a.c1, a.c2}; }

bool rows_ok(int64_t rows) { return rows > 0 && rows < (1 << 24); }

// Every row-major output is addressed through a buffer descriptor: 31-bit byte offsets into the widest of them.  The
// observations count only `with_input`: the chains stage x and x_next with size_t indices (stage_rows), not through a
// descriptor, so the plain chains need no bound on D; the TD3 and LayerNorm paths have bounded it since they came, and
// the shapes they accept stay as they are.
bool offsets_ok(const Dims& d, int64_t rows, bool with_input) {
    const int widest = imax(imax(imax(d.c1 + d.A, d.H1), imax(d.c2, d.H2)), with_input ? d.D : 0);
    return rows * widest * 4 < (1ll << 31);
}

// LayerNorm with a second critic: both parts present (an `ln` without its second part beside a `second` is refused)
bool ln_second(const smx_ddpg_rows_t* a) { return a->ln && a->ln->second && a->second; }

bool net_present(const smx_ddpg_net_t& n) { return n.W1 && n.b1 && n.W2 && n.b2 && n.W3 && n.b3; }

void set_net(RNet& r, const smx_ddpg_net_t& n, const Layout& L, const Dims& d, const float* packed, const int w[3]) {
    r.b1 = n.b1; r.b2 = n.b2; r.b3 = n.b3;
    r.W1 = L.pmat(d, packed, w[0]); r.W2 = L.pmat(d, packed, w[1]); r.W3 = L.pmat(d, packed, w[2]);
}

int fill(RArgs& G, const smx_ddpg_rows_t* a, bool td3 = false, LnProg* Q = nullptr) {
    SMX_REQUIRE(a && a->packed, SMX_E_NULL);
    const Dims d = dims_of(*a);
    // LayerNorm: its own launches; with a second critic only where its LayerNorm part came along
    SMX_REQUIRE(!a->ln || (Q && (a->second ? ln_second(a) : !td3)), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(rows_ok(a->rows), SMX_E_SHAPE);
    SMX_REQUIRE(dims_ok(d, td3), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(offsets_ok(d, a->rows, false), SMX_E_SHAPE);
    SMX_REQUIRE(((uintptr_t)a->packed & 15) == 0, SMX_E_ALIGN);
    const smx_ddpg_net_t* nets[4] = {&a->actor, &a->critic, &a->target_actor, &a->target_critic};
    for (int k = 0; k < 4; ++k) SMX_REQUIRE(net_present(*nets[k]), SMX_E_NULL);
    memset(&G, 0, sizeof(G));
    G.rows = (int)a->rows; G.D = d.D; G.A = d.A; G.H1 = d.H1; G.H2 = d.H2; G.c1 = d.c1; G.c2 = d.c2;
    RNet* rn[4] = {&G.a, &G.c, &G.ta, &G.tc};
    for (int k = 0; k < 4; ++k) set_net(*rn[k], *nets[k], L_FIRST, d, a->packed, NET_W[k]);
    G.cW2Tlo = L_FIRST.pmat(d, a->packed, B_CW2TLO); G.cW2Thi = L_FIRST.pmat(d, a->packed, B_CW2THI);
    G.aW3T = L_FIRST.pmat(d, a->packed, B_AW3T); G.aW2T = L_FIRST.pmat(d, a->packed, B_AW2T);
    G.cW3 = a->critic.W3;
    G.x = a->x; G.xn = a->x_next; G.actions = a->actions; G.rewards = a->rewards; G.dones = a->dones;
    G.gamma_n = a->gamma_n;
    G.xcat = a->xcat; G.h2c = a->h2c; G.q = a->q; G.q_next = a->q_next; G.y = a->y; G.dz3 = a->dz3; G.dz2 = a->dz2;
    G.dxcat = a->dxcat; G.h1a = a->h1a; G.h2a = a->h2a; G.act = a->act;
    G.q_actor = a->q_actor; G.dz3a = a->dz3a; G.dz2a = a->dz2a; G.dz1a = a->dz1a;
    G.step = a->step;
    lds_floats(d, td3, false, &G);
    G.tbuf = g_tbuf;
    if (a->ln) {
        const smx_ddpg_rows_ln* l = a->ln;
        const bool two = ln_second(a);
        SMX_REQUIRE(dims_ok_ln(d, two), SMX_E_UNSUPPORTED);
        SMX_REQUIRE(offsets_ok(d, a->rows, true), SMX_E_SHAPE);
        const smx_ddpg_ln_net* ln[6] = {&l->actor, &l->critic, &l->target_actor, &l->target_critic,
                                        two ? &l->second->critic2 : nullptr, two ? &l->second->target_critic2 : nullptr};
        for (int k = 0; k < (two ? 6 : 4); ++k) SMX_REQUIRE(ln[k]->g1 && ln[k]->b1 && ln[k]->g2 && ln[k]->b2, SMX_E_NULL);
        SMX_REQUIRE(l->eps > 0.f, SMX_E_SHAPE);
        memset(Q, 0, sizeof(*Q));
        lds_floats(d, two, true, &G, Q);
        Q->t.eps = l->eps;
    }
    if (td3) {
        const smx_ddpg_rows_second* s = a->second;
        SMX_REQUIRE(s && s->packed2, SMX_E_NULL);
        SMX_REQUIRE(((uintptr_t)s->packed2 & 15) == 0, SMX_E_ALIGN);
        SMX_REQUIRE(offsets_ok(d, a->rows, true), SMX_E_SHAPE);
        const smx_ddpg_net_t* n2[2] = {&s->critic2, &s->target_critic2};
        RNet* r2[2] = {&G.c2n, &G.tc2};
        for (int k = 0; k < 2; ++k) {
            SMX_REQUIRE(net_present(*n2[k]), SMX_E_NULL);
            set_net(*r2[k], *n2[k], L_SECOND, d, s->packed2, NET2_W[k]);
        }
        G.c2W2Tlo = L_SECOND.pmat(d, s->packed2, B2_CW2TLO);
        G.c2W3 = s->critic2.W3;
        G.noise = s->noise;
        G.xcat2 = s->xcat2; G.h2c2 = s->h2c2; G.q2 = s->q2; G.q_next2 = s->q_next2; G.dz3_2 = s->dz3_2;
        G.dz2_2 = s->dz2_2; G.dxcat2 = s->dxcat2;
    }
    return SMX_OK;
}

Step step(int in_off, int ldi, const PMat& W, const float* bias, int act, int out_off, int ldo, float* g, int ldg, int post) {
    Step S;
    memset(&S, 0, sizeof(S));
    S.W = W.P; S.bias = bias; S.g = g; S.M = W.M; S.K = W.K; S.in_off = in_off; S.ldi = ldi; S.act = act;
    S.out_off = out_off; S.ldo = ldo; S.ldg = ldg; S.post = post;
    return S;
}

void ln_fwd(LnProg& Q, int si, const Step& S, const float* gamma, const float* beta, int t_off, int ldt, float* n, int ldn,
            float* mean, float* rstd, int st) {
    LnStep& T = Q.s[si];
    T.kind = LN_FWD; T.F = S.M; T.gamma = gamma; T.beta = beta; T.p_off = S.out_off; T.ldp = S.ldo; T.t_off = t_off;
    T.ldt = ldt; T.n = n; T.ldn = ldn; T.mean = mean; T.rstd = rstd; T.st = st;
}
void ln_bwd(LnProg& Q, int si, int F, const float* gamma, int p_off, int ldp, int t_off, int ldt, float* n, int ldn, int st) {
    LnStep& T = Q.s[si];
    T.kind = LN_BWD; T.F = F; T.gamma = gamma; T.p_off = p_off; T.ldp = ldp; T.d_off = Q.t.oD; T.ldd = Q.t.ldD; T.t_off = t_off;
    T.ldt = ldt; T.n = n; T.ldn = ldn; T.st = st;
}

// ---------------------------------------------------------------------------------------------------------------
// The chains, written as segments.  A segment emits its plain steps and, where the chain has LayerNorm (Q set), the
// rule behind each; what differs between the two forms is stated in the segment, once:
//  * a hidden layer writes relu(z) to a pre-LayerNorm tile (P1 behind a first layer, P2 behind a second) and to HBM with
//    the layer's own width as stride; the rule puts the normalised rows where the plain chain has the layer's output.
//    So with LayerNorm xcat, h2c, h1a, h2a name the LayerNorm OUTPUTS (what the weight gradients multiply)
//  * a backward product leaves dn in the dn tile, unmasked; the rule (the x > 0 mask folded in) puts the gradient at the
//    ReLU's input where the plain chain has the masked product
// P1 / P2 hold the pre-LayerNorm rows of the network in flight, statistics slots 0 / 1 its two LayerNorms'.
// ---------------------------------------------------------------------------------------------------------------
struct Keep {                     // what a hidden layer leaves in HBM ({}: nothing)
    float* h = nullptr;           // its output [rows][ldh] -- the LayerNorm's where there is one
    int ldh = 0;
    float *pre = nullptr, *mean = nullptr, *rstd = nullptr;       // LayerNorm: relu(z) [rows][F], the rows' statistics
};
const smx_ddpg_rows_ln NO_LN = {};                // what the plain chains read the LayerNorm fields from: all null
const smx_ddpg_rows_ln_second NO_LN2 = {};

struct Chain {
    const RArgs& G;
    Prog& P;
    LnProg* Q;                    // null: no LayerNorm
    int n;

    const Step& emit(const Step& S) {
        P.s[n] = S;
        P.n = n + 1;
        return P.s[n++];
    }
    int pre_off(int level) const { return level == 1 ? Q->t.oP1 : Q->t.oP2; }
    int pre_ld(int level) const { return level == 1 ? Q->t.ldP1 : Q->t.ldP2; }

    // hidden layer `level` of a network: relu(W in + b) -> tile (t, ldt) and k
    void hidden(int level, int in, int ldi, const PMat& W, const float* b, const float* gamma, const float* beta, int t, int ldt,
                int post, const Keep& k) {
        if (!Q) {
            emit(step(in, ldi, W, b, A_RELU, t, ldt, k.h, k.ldh, post));
            return;
        }
        const Step& S = emit(step(in, ldi, W, b, A_RELU, pre_off(level), pre_ld(level), k.pre, k.pre ? W.M : 0, post));
        ln_fwd(*Q, n - 1, S, gamma, beta, t, ldt, k.h, k.ldh, k.mean, k.rstd, level - 1);
    }
    // a network's two hidden layers from the observations at `in`: layer 1 (and its `post`) -> tile (t1, ldt1), layer 2 -> B
    void hidden2(const RNet& N, const smx_ddpg_ln_net& ln, int in, int t1, int ldt1, int post1, const Keep& k1, const Keep& k2) {
        hidden(1, in, G.ldx, N.W1, N.b1, ln.g1, ln.b1, t1, ldt1, post1, k1);
        hidden(2, t1, ldt1, N.W2, N.b2, ln.g2, ln.b2, G.oB, G.ldB, P_NONE, k2);
    }
    // ... and its output layer -> tile `out` (< 0: none) and HBM g
    void forward(const RNet& N, const smx_ddpg_ln_net& ln, int in, int t1, int ldt1, int post1, const Keep& k1, const Keep& k2,
                 int act3, int out, int ldo, float* g = nullptr, int ldg = 0) {
        hidden2(N, ln, in, t1, ldt1, post1, k1, k2);
        emit(step(G.oB, G.ldB, N.W3, N.b3, act3, out, ldo, g, ldg, P_NONE));
    }
    // the LayerNorm-2 backward rule behind a critic's output layer, whose `post` has left dn2 in the dn tile: -> tile A, dz2
    void back_ln2(const float* gamma2, float* dz2) {
        if (Q) ln_bwd(*Q, n - 1, G.c2, gamma2, pre_off(2), pre_ld(2), G.oA, G.ldA, dz2, dz2 ? G.c2 : 0, 1);
    }
    // A backward product, W^T times the tile at `in`, through hidden layer `level`: plain, masked by the layer's output
    // tile (m, ldm) -> tile (t, ldt; < 0: none) and HBM dz; LayerNorm, unmasked -> the dn tile and HBM dn (the same
    // stride ldg), then the rule with the statistics of slot st -> tile t and HBM dzn
    void back(int level, int in, int ldi, const PMat& WT, const float* gamma, int m, int ldm, int t, int ldt, float* dz, int ldg,
              float* dn, float* dzn, int st) {
        if (!Q) {
            Step S = step(in, ldi, WT, nullptr, A_MASK, t, ldt, dz, ldg, P_NONE);
            S.mask_off = m; S.ldm = ldm;
            emit(S);
            return;
        }
        emit(step(in, ldi, WT, nullptr, A_NONE, Q->t.oD, Q->t.ldD, dn, ldg, P_NONE));
        ln_bwd(*Q, n - 1, WT.M, gamma, pre_off(level), pre_ld(level), t, ldt, dzn, WT.M, st);
    }
};

void target_actor(Chain& C, const smx_ddpg_rows_ln& l) {                                    // mu'(s') -> tile O
    C.forward(C.G.ta, l.target_actor, C.G.oXn, C.G.oA, C.G.ldA, P_NONE, {}, {}, A_TANH, C.G.oO, LDO);
}
// Q'(s', .) at the action `cat` puts beside layer 1's output (P_TC_CAT: mu'; P_TC2_CAT: clamp(mu' + noise)) -> tile `out`
void target_critic(Chain& C, const RNet& N, const smx_ddpg_ln_net& ln, int cat, int out) {
    C.forward(N, ln, C.G.oXn, C.G.oC, C.G.ldC, cat, {}, {}, A_NONE, out, LDO);
}
// A critic at (s, a), kept; its loss (P_LOSS: y, dz3 and dz2 -- LayerNorm: dn2; P_LOSS2: against the kept y) and the
// W2^T-lo product: dz1 (LayerNorm: dn1 into dxcat, dz1 into a buffer of its own).  Its backward rules run before the next
// network overwrites the pre-LayerNorm tiles and the statistics.
void critic_sa(Chain& C, const RNet& N, const smx_ddpg_ln_net& ln, const PMat& W2Tlo, int cat, int loss, const Keep& k1,
               const Keep& k2, float* dz2, float* dxcat, float* dz1c) {
    const RArgs& G = C.G;
    C.hidden2(N, ln, G.oX, G.oC, G.ldC, cat, k1, k2);
    C.emit(step(G.oB, G.ldB, N.W3, N.b3, A_NONE, G.oO, LDO, nullptr, 0, loss));
    C.back_ln2(ln.g2, dz2);
    C.back(1, G.oA, G.ldA, W2Tlo, ln.g1, G.oC, G.ldC, -1, 0, dxcat, G.c1 + G.A, dxcat, dz1c, 0);
}
void first_critic(Chain& C, const smx_ddpg_rows_ln& l) {
    const RArgs& G = C.G;
    critic_sa(C, G.c, l.critic, G.cW2Tlo, P_C_CAT, P_LOSS, {G.xcat, G.c1 + G.A, l.c_a1, l.cm1, l.cr1},
              {G.h2c, G.c2, l.c_a2, l.cm2, l.cr2}, G.dz2, G.dxcat, l.dz1c);
}
void second_critic(Chain& C, const smx_ddpg_rows_ln_second& l2) {
    const RArgs& G = C.G;
    critic_sa(C, G.c2n, l2.critic2, G.c2W2Tlo, P_C2_CAT, P_LOSS2, {G.xcat2, G.c1 + G.A, l2.c2_a1, l2.c2m1, l2.c2r1},
              {G.h2c2, G.c2, l2.c2_a2, l2.c2m2, l2.c2r2}, G.dz2_2, G.dxcat2, l2.dz1c2);
}
void actor_kept(Chain& C, const smx_ddpg_rows_ln& l) {                                      // mu(s), kept for ITS update
    const RArgs& G = C.G;
    C.forward(G.a, l.actor, G.oX, G.oA, G.ldA, P_NONE, {G.h1a, G.H1, l.a1, l.am1, l.ar1}, {G.h2a, G.H2, l.a2, l.am2, l.ar2},
              A_TANH, -1, 0, G.act, G.A);
}
// The actor phase behind Q(s, mu(s))'s hidden layers: q and the masks (P_A_DQ: dz2 -- LayerNorm: dn2, back through the
// critic's LayerNorm 2 only, nothing to HBM), d/d(action) with tanh', the actor's dz2 and dz1.  With LayerNorm the kernel
// stages the actor's pre-LayerNorm rows and statistics (a2, a1: slots 3, 2) from HBM for the two rules.
void actor_tail(Chain& C, const smx_ddpg_rows_ln& l) {
    const RArgs& G = C.G;
    C.emit(step(G.oB, G.ldB, G.c.W3, G.c.b3, A_NONE, -1, 0, G.q_actor, 1, P_A_DQ));
    C.back_ln2(l.critic.g2, nullptr);
    C.emit(step(G.oA, G.ldA, G.cW2Thi, nullptr, A_NONE, G.oO2, LDO, nullptr, 0, P_A_TANH));
    C.back(2, G.oZ, LDK4, G.aW3T, l.actor.g2, G.oB, G.ldB, G.oA, G.ldA, G.dz2a, G.H2, l.dn2a, G.dz2a, 3);
    C.back(1, G.oA, G.ldA, G.aW2T, l.actor.g1, G.oC, G.ldC, -1, 0, G.dz1a, G.H1, l.dn1a, G.dz1a, 2);
}

// the three chains (l, l2: NO_LN, NO_LN2 without LayerNorm)
// (actor false: the critic-only programs of a delayed policy update -- the same chain without its last segment)
void critic_chain(Chain& C, const smx_ddpg_rows_ln& l, bool actor = true) {
    target_actor(C, l);
    target_critic(C, C.G.tc, l.target_critic, P_TC_CAT, C.G.oO2);
    first_critic(C, l);
    if (actor) actor_kept(C, l);
    if (C.Q) C.Q->t.dn2 = l.dn2;
}
static_assert(LN_STEPS >= 13, "the critic chain has 13 layers");

void actor_chain(Chain& C, const smx_ddpg_rows_ln& l) {
    C.hidden2(C.G.c, l.critic, C.G.oX, C.G.oC, C.G.ldC, P_A_CAT, {}, {});                   // Q(s, mu(s))
    actor_tail(C, l);
    if (C.Q) {
        LnProg& Q = *C.Q;
        Q.t.a1 = l.a1; Q.t.a2 = l.a2; Q.t.am1 = l.am1; Q.t.ar1 = l.ar1; Q.t.am2 = l.am2; Q.t.ar2 = l.ar2;
    }
}

// TD3's critic chain (ddpg.py:266-283, 312-319): both target critics (the second at the noised action), then each
// critic's forward pass, loss and data gradients against y = min(y1, y2), then the actor's forward pass.  With LayerNorm:
// the same 20 products, a forward rule behind each of the 12 hidden layers, a backward rule behind each critic's loss and
// behind its W2^T product -- 16 rules
void td3_critic_chain(Chain& C, const smx_ddpg_rows_ln& l, const smx_ddpg_rows_ln_second& l2, bool actor = true) {
    target_actor(C, l);
    target_critic(C, C.G.tc, l.target_critic, P_TC_CAT, C.G.oO2);
    target_critic(C, C.G.tc2, l2.target_critic2, P_TC2_CAT, C.G.oO3);
    first_critic(C, l);
    second_critic(C, l2);
    if (actor) actor_kept(C, l);
    if (C.Q) {
        C.Q->t.dn2 = l.dn2;
        C.Q->t.dn2_2 = l2.dn2_2;
    }
}
static_assert(MAX_STEPS >= 20 && LN_STEPS_TD3 >= 20 && LN_STEPS_TD3 <= MAX_STEPS, "the TD3 critic chain has 20 layers");

// the 13-step launches' copy of the host's table (its dn2_2 is null: the 13-step chains have no second critic)
LnProgT<LN_STEPS> narrow(const LnProg& Q) {
    LnProgT<LN_STEPS> R;
    memset(&R, 0, sizeof(R));
    memcpy(R.s, Q.s, sizeof(R.s));
    R.t = Q.t;
    return R;
}

// One chain launch, K(G, P) or K(G, P, Q).  A kernel's LDS limit is an attribute of the function, so the high-water mark
// of what has been asked for is one static per kernel: per instantiation of this template.
template <auto K, class... LQ>
int launch_chain(const RArgs& G, const Prog& P, smx_stream_t stream, const LQ&... Q) {
    const int bytes = G.total * (int)sizeof(float);
    static int set = 0;
    if (set < bytes) {
        const int e = (int)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e) return e;
        set = bytes;
    }
    hipLaunchKernelGGL(K, dim3((unsigned)((G.rows + RBLK - 1) / RBLK)), dim3(DNTH), bytes, smx_s(stream), G, P, Q...);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

// The LayerNorm chains' launches by phase (0: critic, 1: actor, 2: TD3's critic).  Only TD3's kernel takes the 20-step rule
// table; the other two take its narrow() copy
int launch_chain_ln(int phase, const RArgs& G, const Prog& P, const LnProg& Q, smx_stream_t stream) {
    switch (phase) {
        case 0: return launch_chain<ddpg_rows4_ln_kernel<0>>(G, P, stream, narrow(Q));
        case 1: return launch_chain<ddpg_rows4_ln_kernel<1>>(G, P, stream, narrow(Q));
        default: return launch_chain<ddpg_rows4_ln_kernel<2>>(G, P, stream, Q);
    }
}

// the buffers the critic chains read and write; those they write with LayerNorm (actor false: a critic-only program,
// which leaves the actor's buffers alone)
bool critic_io(const smx_ddpg_rows_t* a, bool actor = true) {
    return a->x && a->x_next && a->actions && a->rewards && a->dones && a->xcat && a->h2c && a->q && a->q_next && a->y &&
           a->dz3 && a->dz2 && a->dxcat && (!actor || (a->h1a && a->h2a && a->act));
}
bool critic_io_ln(const smx_ddpg_rows_ln& l, bool actor = true) {
    return l.c_a1 && l.cm1 && l.cr1 && l.c_a2 && l.cm2 && l.cr2 && l.dn2 && l.dz1c &&
           (!actor || (l.a1 && l.am1 && l.ar1 && l.a2 && l.am2 && l.ar2));
}

int launch_pack(const float* const* src, const int* ld, const int* tr, int first, int last, const Layout& L, const Dims& d,
                float* packed, smx_stream_t stream) {
    PArgs P;
    memset(&P, 0, sizeof(P));
    P.packed = packed;
    P.count = last - first;
    for (int b = first; b < last; ++b) {
        SMX_REQUIRE(src[b], SMX_E_NULL);
        PItem& it = P.it[b - first];
        it.src = src[b]; it.ld = ld[b]; it.tr = tr[b];
        L.shape(d, b, it.M, it.K);
        it.base = L.base(d, b);
    }
    P.total = L.base(d, last) - L.base(d, first);
    hipLaunchKernelGGL(ddpg_pack_kernel, dim3((unsigned)((P.total + 255) / 256)), dim3(256), 0, smx_s(stream), P);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

}  // namespace

extern "C" void smx_ddpg_rows_debug_tbuf(void* p) { g_tbuf = (long long*)p; }

extern "C" int32_t smx_ddpg_rows_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2) {
    return dims_ok(Dims{D, A, H1, H2, c1, c2}) ? 1 : 0;
}

extern "C" int32_t smx_ddpg_rows_supported_at(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2,
                                              int64_t rows) {
    return rows_ok(rows) && dims_ok(Dims{D, A, H1, H2, c1, c2}) ? 1 : 0;
}

extern "C" int64_t smx_ddpg_rows_packed_floats(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2) {
    const Dims d{D, A, H1, H2, c1, c2};
    return dims_ok(d) ? 4 * L_FIRST.base(d, B_COUNT) : 0;
}

extern "C" int32_t smx_ddpg_rows_second_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2,
                                                  int64_t rows) {
    const Dims d{D, A, H1, H2, c1, c2};
    return rows_ok(rows) && dims_ok(d, true) && offsets_ok(d, rows, true) ? 1 : 0;
}

extern "C" int32_t smx_ddpg_rows_ln_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2,
                                              int64_t rows) {
    const Dims d{D, A, H1, H2, c1, c2};
    return rows_ok(rows) && dims_ok_ln(d) && offsets_ok(d, rows, true) ? 1 : 0;
}

extern "C" int32_t smx_ddpg_rows_ln_second_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2,
                                                     int64_t rows) {
    return smx_ddpg_rows_ln_supported(D, A, H1, H2, c1, c2, rows) && dims_ok_ln(Dims{D, A, H1, H2, c1, c2}, true) ? 1 : 0;
}

extern "C" int64_t smx_ddpg_rows_second_packed_floats(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2) {
    const Dims d{D, A, H1, H2, c1, c2};
    return dims_ok(d, true) ? 4 * L_SECOND.base(d, B2_COUNT) : 0;
}

extern "C" int smx_ddpg_rows_pack_f32(const smx_ddpg_rows_t* a, int32_t which, smx_stream_t stream) {
    SMX_REQUIRE(a && a->packed, SMX_E_NULL);
    const Dims d = dims_of(*a);
    SMX_REQUIRE(dims_ok(d), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(!a->ln || ln_second(a) || (!a->second && which != SMX_DDPG_PACK_SECOND), SMX_E_UNSUPPORTED);
    const int ldc = d.c1 + d.A;
    if (which == SMX_DDPG_PACK_SECOND) {             // the second critic's seven blocks into ITS packed buffer
        const smx_ddpg_rows_second* s = a->second;
        SMX_REQUIRE(s && s->packed2, SMX_E_NULL);
        SMX_REQUIRE(dims_ok(d, true), SMX_E_UNSUPPORTED);
        SMX_REQUIRE(((uintptr_t)s->packed2 & 15) == 0, SMX_E_ALIGN);
        const float* src[B2_COUNT] = {s->critic2.W1, s->critic2.W2, s->critic2.W3, s->critic2.W2,
                                      s->target_critic2.W1, s->target_critic2.W2, s->target_critic2.W3};
        const int ld[B2_COUNT] = {d.D, ldc, d.c2, ldc, d.D, ldc, d.c2};
        const int tr[B2_COUNT] = {0, 0, 0, 1, 0, 0, 0};
        return launch_pack(src, ld, tr, 0, B2_COUNT, L_SECOND, d, s->packed2, stream);
    }
    SMX_REQUIRE(which == SMX_DDPG_PACK_ALL || which == SMX_DDPG_PACK_CRITIC, SMX_E_SHAPE);
    const float* src[B_COUNT] = {a->actor.W1, a->actor.W2, a->actor.W3, a->actor.W3, a->actor.W2,
                                 a->critic.W1, a->critic.W2, a->critic.W3, a->critic.W2, a->critic.W2 ? a->critic.W2 + d.c1 : nullptr,
                                 a->target_actor.W1, a->target_actor.W2, a->target_actor.W3,
                                 a->target_critic.W1, a->target_critic.W2, a->target_critic.W3};
    const int ld[B_COUNT] = {d.D, d.H1, d.H2, d.H2, d.H1, d.D, ldc, d.c2, ldc, ldc, d.D, d.H1, d.H2, d.D, ldc, d.c2};
    const int tr[B_COUNT] = {0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0};
    const bool cr = which == SMX_DDPG_PACK_CRITIC;
    return launch_pack(src, ld, tr, cr ? B_CW1 : 0, cr ? B_CW2THI + 1 : B_COUNT, L_FIRST, d, a->packed, stream);
}

namespace {
// the one-critic critic chain's launch, with (an iteration that updates the actor) or without the actor's forward pass
int launch_critic(const smx_ddpg_rows_t* a, bool actor, smx_stream_t stream) {
    RArgs G;
    LnProg Q;
    SMX_REQUIRE(!(a && a->ln && a->second), SMX_E_UNSUPPORTED);      // (two LayerNorm critics: smx_ddpg_rows_critic_td3_f32)
    const int rc = fill(G, a, false, &Q);
    if (rc) return rc;
    SMX_REQUIRE(critic_io(a, actor), SMX_E_NULL);
    SMX_REQUIRE(!a->ln || critic_io_ln(*a->ln, actor), SMX_E_NULL);
    Prog P;
    memset(&P, 0, sizeof(P));
    Chain C{G, P, a->ln ? &Q : nullptr, 0};
    critic_chain(C, a->ln ? *a->ln : NO_LN, actor);
    return a->ln ? launch_chain_ln(0, G, P, Q, stream) : launch_chain<ddpg_rows4_kernel<0>>(G, P, stream);
}

// ... and TD3's
int launch_critic_td3(const smx_ddpg_rows_t* a, bool actor, smx_stream_t stream) {
    RArgs G;
    LnProg Q;
    const int rc = fill(G, a, true, &Q);
    if (rc) return rc;
    const smx_ddpg_rows_second* s = a->second;
    SMX_REQUIRE(critic_io(a, actor), SMX_E_NULL);
    SMX_REQUIRE(s->xcat2 && s->h2c2 && s->q2 && s->q_next2 && s->dz3_2 && s->dz2_2 && s->dxcat2, SMX_E_NULL);
    const smx_ddpg_rows_ln_second* l2 = a->ln ? a->ln->second : nullptr;     // (fill: there beside `second`)
    SMX_REQUIRE(!a->ln || critic_io_ln(*a->ln, actor), SMX_E_NULL);
    SMX_REQUIRE(!l2 || (l2->c2_a1 && l2->c2m1 && l2->c2r1 && l2->c2_a2 && l2->c2m2 && l2->c2r2 && l2->dn2_2 && l2->dz1c2),
                SMX_E_NULL);
    Prog P;
    memset(&P, 0, sizeof(P));
    Chain C{G, P, a->ln ? &Q : nullptr, 0};
    td3_critic_chain(C, a->ln ? *a->ln : NO_LN, l2 ? *l2 : NO_LN2, actor);
    return a->ln ? launch_chain_ln(2, G, P, Q, stream) : launch_chain<ddpg_rows4_kernel<2>>(G, P, stream);
}

// The tail of a delayed learner's UPDATE iteration, one workgroup between the actor chain and the actor's
// gradient-and-step launch: the iteration's statistics as the gradient-and-step launch's extra workgroup forms them --
// the host slot chosen by the ITERATION's step word, which the actor's launch no longer reads --, then the actor's own
// Adam step word moves on
struct DTail {
    int* actor_step;
    const int* step;
    float *stats, *stats2, *stats_host;
    const float *q, *y, *rewards, *actions, *q_actor, *q2;
    int A, rows;
};
__global__ __launch_bounds__(64 * WNW) void ddpg_rows_delay_tail_kernel(DTail T) {
    if (T.stats) {
        float* mirror = T.stats_host ? T.stats_host + (T.stats2 ? 16 : 8) * (*T.step & 1) : nullptr;
        ddpg_stats_block<64 * WNW>(T.q, T.y, T.rewards, T.actions, T.A, T.A, T.q_actor, (long)T.rows, T.stats, mirror);
        if (T.stats2)
            ddpg_stats_block<64 * WNW>(T.q2, T.y, T.rewards, T.actions, T.A, T.A, T.q2, (long)T.rows, T.stats2,
                                       mirror ? mirror + 8 : nullptr);
    }
    if (threadIdx.x == 0) *T.actor_step += 1;
}
}  // namespace

extern "C" int smx_ddpg_rows_critic_f32(const smx_ddpg_rows_t* a, smx_stream_t stream) {
    return launch_critic(a, true, stream);
}

extern "C" int smx_ddpg_rows_critic_td3_f32(const smx_ddpg_rows_t* a, smx_stream_t stream) {
    return launch_critic_td3(a, true, stream);
}

extern "C" int smx_ddpg_rows_critic_only_f32(const smx_ddpg_rows_t* a, smx_stream_t stream) {
    return launch_critic(a, false, stream);
}

extern "C" int smx_ddpg_rows_critic_only_td3_f32(const smx_ddpg_rows_t* a, smx_stream_t stream) {
    return launch_critic_td3(a, false, stream);
}

extern "C" int smx_ddpg_rows_delay_tail_f32(const smx_ddpg_rows_t* a, int32_t* actor_step, float* stats, float* stats_host,
                                            smx_stream_t stream) {
    SMX_REQUIRE(actor_step, SMX_E_NULL);
    SMX_REQUIRE(stats || !stats_host, SMX_E_NULL);
    DTail T;
    memset(&T, 0, sizeof(T));
    T.actor_step = actor_step;
    if (stats) {
        SMX_REQUIRE(a && a->step && a->q && a->y && a->rewards && a->actions && a->q_actor, SMX_E_NULL);
        SMX_REQUIRE(rows_ok(a->rows), SMX_E_SHAPE);
        T.step = a->step; T.stats = stats; T.stats_host = stats_host;
        T.q = a->q; T.y = a->y; T.rewards = a->rewards; T.actions = a->actions; T.q_actor = a->q_actor;
        T.A = a->A; T.rows = (int)a->rows;
        if (a->second && a->second->stats2) {        // the second critic's block, (q2, y), as the fused launch writes it
            SMX_REQUIRE(a->second->q2, SMX_E_NULL);
            T.stats2 = a->second->stats2; T.q2 = a->second->q2;
        }
    }
    hipLaunchKernelGGL(ddpg_rows_delay_tail_kernel, dim3(1), dim3(64 * WNW), 0, smx_s(stream), T);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_ddpg_rows_actor_f32(const smx_ddpg_rows_t* a, smx_stream_t stream) {
    RArgs G;
    LnProg Q;
    const int rc = fill(G, a, false, &Q);
    if (rc) return rc;
    SMX_REQUIRE(a->x && a->h1a && a->h2a && a->act && a->q_actor && a->dz3a && a->dz2a && a->dz1a, SMX_E_NULL);
    const smx_ddpg_rows_ln* l = a->ln;
    SMX_REQUIRE(!l || (l->a1 && l->am1 && l->ar1 && l->a2 && l->am2 && l->ar2 && l->dn2a && l->dn1a), SMX_E_NULL);
    Prog P;
    memset(&P, 0, sizeof(P));
    Chain C{G, P, l ? &Q : nullptr, 0};
    actor_chain(C, l ? *l : NO_LN);
    return l ? launch_chain_ln(1, G, P, Q, stream) : launch_chain<ddpg_rows4_kernel<1>>(G, P, stream);
}

namespace {
// An optimiser group's side of the packed buffers: its network and target, the buffer and its layout, the blocks of W1, W2,
// W3, of the target's, and of the transposed copies (< 0: none; columns < split -> t0, the rest -> t1)
struct UGroup {
    const smx_ddpg_net_t *net, *tnet;
    float* packed;
    const Layout* L;
    int w[3], tw[3], t0[3], t1[3];
    bool split_w2;                // a critic's W2: the columns of layer 1's output apart from the action's
};

int fill_update(UArgs& U, const smx_ddpg_rows_t* a, int32_t group, const smx_ddpg_update_t* u, const Dims& d) {
    SMX_REQUIRE(u->theta && u->grads && u->exp_avg && u->exp_avg_sq && u->lr && u->step, SMX_E_NULL);
    SMX_REQUIRE(group == SMX_DDPG_GROUP_ACTOR || group == SMX_DDPG_GROUP_CRITIC || group == SMX_DDPG_GROUP_CRITIC2,
                SMX_E_SHAPE);
    SMX_REQUIRE(u->n > 0 && u->interval >= 0 && (u->target == nullptr || u->interval > 0 || u->tau > 0.f), SMX_E_SHAPE);
    const smx_ddpg_rows_second* s = a->second;
    if (group == SMX_DDPG_GROUP_CRITIC2) {
        SMX_REQUIRE(s && s->packed2, SMX_E_NULL);
        SMX_REQUIRE(dims_ok(d, true), SMX_E_UNSUPPORTED);
    }
    // the second critic: its own networks and packed buffer, the first critic's shapes; W2^T's low block only
    const UGroup g =
        group == SMX_DDPG_GROUP_CRITIC2
            ? UGroup{&s->critic2, &s->target_critic2, s->packed2, &L_SECOND, {B2_CW1, B2_CW2, B2_CW3},
                     {B2_TCW1, B2_TCW2, B2_TCW3}, {-1, B2_CW2TLO, -1}, {-1, -1, -1}, true}
        : group == SMX_DDPG_GROUP_CRITIC
            ? UGroup{&a->critic, &a->target_critic, a->packed, &L_FIRST, {B_CW1, B_CW2, B_CW3}, {B_TCW1, B_TCW2, B_TCW3},
                     {-1, B_CW2TLO, -1}, {-1, B_CW2THI, -1}, true}
            : UGroup{&a->actor, &a->target_actor, a->packed, &L_FIRST, {B_AW1, B_AW2, B_AW3}, {B_TAW1, B_TAW2, B_TAW3},
                     {-1, B_AW2T, B_AW3T}, {-1, -1, -1}, false};
    SMX_REQUIRE(g.net->W1 && g.net->W2 && g.net->W3, SMX_E_NULL);
    memset(&U, 0, sizeof(U));
    U.theta = u->theta; U.grads = u->grads; U.m = u->exp_avg; U.v = u->exp_avg_sq; U.target = u->target;
    U.packed = g.packed; U.n = u->n; U.lr = u->lr; U.step = u->step; U.wd = u->weight_decay;
    U.clip_value = u->clip_value; U.tau = u->tau; U.interval = u->interval;
    const float* W[3] = {g.net->W1, g.net->W2, g.net->W3};
    const float* TW[3] = {g.tnet->W1, g.tnet->W2, g.tnet->W3};
    for (int j = 0; j < 3; ++j) {
        UMat& X = U.mat[j];
        g.L->shape(d, g.w[j], X.M, X.K);
        X.off = W[j] - u->theta;
        // the matrices lie inside the group's buffer, the target's at the same offsets inside the target's
        SMX_REQUIRE(X.off >= 0 && X.off + (long)X.M * X.K <= u->n, SMX_E_SHAPE);
        if (u->target) SMX_REQUIRE(TW[j] && TW[j] - u->target == X.off, SMX_E_SHAPE);
        X.base = 4 * g.L->base(d, g.w[j]);
        X.base_tgt = 4 * g.L->base(d, g.tw[j]);
        X.base_t0 = g.t0[j] < 0 ? -1 : 4 * g.L->base(d, g.t0[j]);
        X.base_t1 = g.t1[j] < 0 ? -1 : 4 * g.L->base(d, g.t1[j]);
        X.split = g.split_w2 && j == 1 ? d.c1 : X.K;
    }
    return SMX_OK;
}

// What a group's gradient-and-step launch reads: (gradient, input) of the three layers -- the buffers the chain launches
// wrote -- and the networks; with LayerNorm (dn, pre-LayerNorm rows, statistics) of the two LayerNorms and their parameters.
// LayerNorm: a critic's dz1 is a buffer of its own, dxcat keeps dn1; xcat / h2c / h1a / h2a are the LayerNorm outputs
struct WIo {
    const float* dz[3];
    int ldz[3];
    const float* x[3];
    int ldx[3];
    const smx_ddpg_net_t *net, *tnet;
    const float *dn[2], *pre[2], *mean[2], *rstd[2];
    int F[2], lddn[2];
    const smx_ddpg_ln_net *p, *tp;
};
}  // namespace

extern "C" int smx_ddpg_rows_update_f32(const smx_ddpg_rows_t* a, int32_t group, const smx_ddpg_update_t* u,
                                        smx_stream_t stream) {
    SMX_REQUIRE(a && a->packed && u, SMX_E_NULL);
    SMX_REQUIRE(!a->ln, SMX_E_UNSUPPORTED);          // (the LayerNorm path steps with its gradients: _wgrad_update_f32)
    const Dims d = dims_of(*a);
    SMX_REQUIRE(dims_ok(d), SMX_E_UNSUPPORTED);
    UArgs U;
    const int rc = fill_update(U, a, group, u, d);
    if (rc) return rc;
    hipLaunchKernelGGL(ddpg_rows_update_kernel, dim3((unsigned)((u->n + 255) / 256)), dim3(256), 0, smx_s(stream), U);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_ddpg_rows_wgrad_update_f32(const smx_ddpg_rows_t* a, int32_t group, const smx_ddpg_update_t* u,
                                              smx_stream_t stream) {
    SMX_REQUIRE(a && a->packed && u, SMX_E_NULL);
    const Dims d = dims_of(*a);
    SMX_REQUIRE(dims_ok(d), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(rows_ok(a->rows), SMX_E_SHAPE);
    const bool ln = a->ln != nullptr;
    const bool two = ln_second(a);
    SMX_REQUIRE(!ln || ((two || (!a->second && group != SMX_DDPG_GROUP_CRITIC2)) && dims_ok_ln(d, two) &&
                        offsets_ok(d, a->rows, true)), SMX_E_UNSUPPORTED);
    WUArgs G;
    memset(&G, 0, sizeof(G));
    const int rc = fill_update(G.U, a, group, u, d);
    if (rc) return rc;
    G.U.grads_out = const_cast<float*>(u->grads);
    G.rows = (int)a->rows;
    G.tbuf = g_tbuf;
    const smx_ddpg_rows_second* s2 = a->second;                      // (fill_update has checked it for the second critic)
    const smx_ddpg_rows_ln& l = ln ? *a->ln : NO_LN;
    const smx_ddpg_rows_ln_second& l2 = two ? *a->ln->second : NO_LN2;
    const int ldc = d.c1 + d.A;
    WIo io;
    switch (group) {
        case SMX_DDPG_GROUP_CRITIC2:
            io = {{ln ? l2.dz1c2 : s2->dxcat2, s2->dz2_2, s2->dz3_2}, {ln ? d.c1 : ldc, d.c2, 1},
                  {a->x, s2->xcat2, s2->h2c2}, {d.D, ldc, d.c2}, &s2->critic2, &s2->target_critic2,
                  {s2->dxcat2, l2.dn2_2}, {l2.c2_a1, l2.c2_a2}, {l2.c2m1, l2.c2m2}, {l2.c2r1, l2.c2r2}, {d.c1, d.c2}, {ldc, d.c2},
                  &l2.critic2, &l2.target_critic2};
            break;
        case SMX_DDPG_GROUP_CRITIC:
            io = {{ln ? l.dz1c : a->dxcat, a->dz2, a->dz3}, {ln ? d.c1 : ldc, d.c2, 1},
                  {a->x, a->xcat, a->h2c}, {d.D, ldc, d.c2}, &a->critic, &a->target_critic,
                  {a->dxcat, l.dn2}, {l.c_a1, l.c_a2}, {l.cm1, l.cm2}, {l.cr1, l.cr2}, {d.c1, d.c2}, {ldc, d.c2},
                  &l.critic, &l.target_critic};
            break;
        default:
            io = {{a->dz1a, a->dz2a, a->dz3a}, {d.H1, d.H2, d.A},
                  {a->x, a->h1a, a->h2a}, {d.D, d.H1, d.H2}, &a->actor, &a->target_actor,
                  {l.dn1a, l.dn2a}, {l.a1, l.a2}, {l.am1, l.am2}, {l.ar1, l.ar2}, {d.H1, d.H2}, {d.H1, d.H2},
                  &l.actor, &l.target_actor};
    }
    const float* b[3] = {io.net->b1, io.net->b2, io.net->b3};
    const float* tb[3] = {io.tnet->b1, io.tnet->b2, io.tnet->b3};
    int tiles = 0;
    for (int j = 0; j < 3; ++j) {
        SMX_REQUIRE(io.dz[j] && io.x[j] && b[j], SMX_E_NULL);
        WMat& W = G.w[j];
        const UMat& X = G.U.mat[j];
        W.dz = io.dz[j]; W.ldz = io.ldz[j]; W.x = io.x[j]; W.ldx = io.ldx[j];
        W.boff = b[j] - u->theta;
        SMX_REQUIRE(W.boff >= 0 && W.boff + X.M <= u->n, SMX_E_SHAPE);
        if (u->target) SMX_REQUIRE(tb[j] && tb[j] - u->target == W.boff, SMX_E_SHAPE);
        SMX_REQUIRE((int64_t)a->rows * imax(io.ldz[j], io.ldx[j]) * 4 < (1ll << 31), SMX_E_SHAPE);
        W.tiles_n = (X.K + 31) / 32;
        W.tile0 = tiles;
        tiles += ((X.M + 31) / 32) * W.tiles_n;
    }
    // every element of the group's buffer is a weight or a bias of the three layers: nothing is left without its step
    {
        long covered = 0;
        for (int j = 0; j < 3; ++j) covered += (long)G.U.mat[j].M * G.U.mat[j].K + G.U.mat[j].M;
        if (ln) covered += 2l * (io.F[0] + io.F[1]);                 // ... or a LayerNorm's gain or bias
        SMX_REQUIRE(covered == u->n, SMX_E_SHAPE);
    }
    G.tiles = tiles;
    if (ln) {
        const float* gam[2] = {io.p->g1, io.p->g2};
        const float* bet[2] = {io.p->b1, io.p->b2};
        const float* tgam[2] = {io.tp->g1, io.tp->g2};
        const float* tbet[2] = {io.tp->b1, io.tp->b2};
        int blocks = 0;
        for (int k = 0; k < 2; ++k) {
            const int F = io.F[k];
            SMX_REQUIRE(gam[k] && bet[k] && io.dn[k] && io.pre[k] && io.mean[k] && io.rstd[k], SMX_E_NULL);
            WLn& W = G.ln[k];
            W.dn = io.dn[k]; W.lddn = io.lddn[k]; W.pre = io.pre[k]; W.ldp = F; W.mean = io.mean[k]; W.rstd = io.rstd[k]; W.F = F;
            W.goff = gam[k] - u->theta; W.boff = bet[k] - u->theta;
            SMX_REQUIRE(W.goff >= 0 && W.goff + F <= u->n && W.boff >= 0 && W.boff + F <= u->n, SMX_E_SHAPE);
            if (u->target)
                SMX_REQUIRE(tgam[k] && tbet[k] && tgam[k] - u->target == W.goff && tbet[k] - u->target == W.boff, SMX_E_SHAPE);
            W.blk0 = blocks;
            blocks += (F + LNC - 1) / LNC;
        }
        G.ln_blocks = blocks;
    }
    if (u->stats) {
        SMX_REQUIRE(a->q && a->y && a->rewards && a->actions && a->q_actor, SMX_E_NULL);
        G.stats = u->stats; G.s_q = a->q; G.s_y = a->y; G.s_rewards = a->rewards; G.s_actions = a->actions;
        G.s_q_actor = a->q_actor; G.s_A = d.A;
        G.stats_host = u->stats_host;
        if (s2 && s2->stats2) {          // the second critic's block, (q2, y), by the same workgroup
            SMX_REQUIRE(s2->q2, SMX_E_NULL);
            G.stats2 = s2->stats2; G.s_q2 = s2->q2;
        }
    }
    hipLaunchKernelGGL(ddpg_rows_wgrad_update_kernel, dim3((unsigned)(tiles + G.ln_blocks + (u->stats ? 1 : 0))), dim3(64 * WNW), 0,
                       smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}
