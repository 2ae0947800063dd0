/*
 * surreal_amd.h -- C ABI of libsurreal_amd.so: the MI355X (gfx950) hot path of
 * SurrealAI/surreal's Agent -> Replay -> Learner data path.
 *
 * The reference is 100 % Python on PyTorch ATen ops: it has NO native layer and
 * NO FFI for this path.  The entry points below are
 * therefore exactly the set a maintainer's ctypes binding would call from the
 * reference's own plugin classes; each one cites the reference interface
 * (file:line, relative to the reference tree) whose arithmetic it replaces.
 * INTEGRATION.md shows the reference-side ctypes stubs.
 *
 * Conventions
 *   - extern "C", plain device pointers + sizes, no torch / C++ types.
 *   - every function returns 0 on success, a negative SMX_E_* argument error, or a
 *     positive hipError_t from the launch; nothing throws.
 *   - nothing allocates, nothing synchronises: the caller (PyTorch-ROCm on the
 *     host side) owns every buffer, including the workspaces whose sizes the
 *     *_ws_bytes() helpers return.  All launches go to `stream` (a hipStream_t
 *     passed as void*), so every entry point is legal inside hipGraph capture.
 *   - all tensors are dense row-major fp32 unless stated.
 *   - mutable training scalars (learning rates, beta, clip epsilon, Adam step
 *     counters, the KL early-exit flag) live in DEVICE memory (smx_ppo_ctrl) so
 *     that a captured graph can be replayed while they change.
 */
#ifndef SURREAL_AMD_H
#define SURREAL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* smx_stream_t; /* hipStream_t */

enum {
    SMX_OK = 0,
    SMX_E_NULL = -1,      /* required pointer is NULL */
    SMX_E_SHAPE = -2,     /* non-positive / inconsistent dimension */
    SMX_E_UNSUPPORTED = -3, /* shape outside what the kernel is built for */
    SMX_E_WORKSPACE = -4, /* workspace too small */
    SMX_E_ALIGN = -5      /* pointer not 16-byte aligned where required */
};

enum { SMX_ACT_NONE = 0, SMX_ACT_RELU = 1, SMX_ACT_TANH = 2 };
enum { SMX_PPO_CLIP = 0, SMX_PPO_ADAPT = 1 };

int smx_abi_version(void);   /* 2 (1: the DDPG rollout and the parameter noise had an entry point per actor variant) */
const char* smx_error_string(int code);

/* ---------------------------------------------------------------------------
 * Three-layer MLP: Linear(D,H1)-ReLU-Linear(H1,H2)-ReLU-Linear(H2,OUT)[-Tanh]
 * = PPO_ActorNetwork / PPO_CriticNetwork (surreal/model/model_builders/builders.py:86-175).
 * W* are [out_features, in_features] row-major (torch.nn.Linear layout).
 * ------------------------------------------------------------------------- */
typedef struct {
    const float* W1; const float* b1; /* [H1,D]  [H1]  */
    const float* W2; const float* b2; /* [H2,H1] [H2]  */
    const float* W3; const float* b3; /* [OUT,H2] [OUT] */
    int32_t D, H1, H2, OUT;
} smx_mlp3_t;

/* --- z-filter (surreal/model/z_filter.py:44-79) ---------------------------- */
/* mean = sum/count ; std = clamp(sqrt(sumsq/count - mean^2), min=eps)  (z_filter.py:74-76) */
int smx_zfilter_stats_f32(const float* running_sum, const float* running_sumsq,
                          const float* count, int32_t D, float eps,
                          float* mean_out, float* std_out, smx_stream_t stream);
/* out[r,:] = clamp((x[r*ldx + :] - mean)/std, -5, 5), r < rows  (z_filter.py:77).
 * ldx = row stride of x in floats (>= D; e.g. N*D to read step 0 of every sub-trajectory,
 * ppo.py:537); out is dense [rows, D]. */
int smx_zfilter_forward_f32(const float* x, int64_t ldx, int64_t rows, int32_t D,
                            const float* mean, const float* std, float* out,
                            smx_stream_t stream);
/* the two calls above in one launch, straight from the running sums: what an acting agent
 * needs for its one observation per step (PPOAgent.act -> forward_actor -> ZFilter.forward,
 * ppo_agent.py:106-154, z_filter.py:59-79).  Bit-identical to stats + forward. */
int smx_zfilter_forward_sums_f32(const float* x, int64_t ldx, int64_t rows, int32_t D,
                                 const float* running_sum, const float* running_sumsq,
                                 const float* count, float eps, float* out, smx_stream_t stream);
/* sum += sum_rows x ; sumsq += sum_rows x*x ; count += count_rows  (z_filter.py:55-57).
 * count_rows lets a data-parallel rank add its local column sums while the caller
 * all-reduces them (pass 0 and add the global count once). */
int smx_zfilter_update_f32(const float* x, int64_t ldx, int64_t rows, int32_t D,
                           float* running_sum, float* running_sumsq, float* count,
                           float count_rows, smx_stream_t stream);
/* The same for MANY rows (the z-update of a policy on a stem runs over B * E ~ 10^5 observation rows): the rows are cut
 * into chunks whose column sums go through ws (smx_zfilter_update_ws_floats(rows, D) floats; 0 = few rows) and are
 * added in chunk order by a second launch.  With ws == NULL or too small this IS smx_zfilter_update_f32. */
int64_t smx_zfilter_update_ws_floats(int64_t rows, int32_t D);
int smx_zfilter_update_ws_f32(const float* x, int64_t ldx, int64_t rows, int32_t D, float* running_sum,
                              float* running_sumsq, float* count, float count_rows, float* ws, int64_t ws_floats,
                              smx_stream_t stream);

/* Process-wide switch of smx_mlp3_forward_fused_f32's z-filter arithmetic.  0 (default): (x - m) * (1 / s), one rounding
 * more than surreal/model/z_filter.py:77 (<= 1 ulp of the filtered input); 1: the reference's division, on the
 * generic (slower) staging path.  tests/test_gpu_kernels.py::test_fused_exact_zfilter_switch pins both. */
int smx_mlp3_fused_exact_zfilter(int32_t on);

/* --- fused critic/actor forward over every step of every sub-trajectory ------
 * Replaces PPOModel.forward_critic / forward_actor on the concatenated
 * (obs, obs_next) tensor in PPOLearner._gae_and_return (surreal/learner/ppo.py:376-386,
 * surreal/model/ppo_net.py:253-315): z-filter prologue + three GEMMs on FP32 MFMA
 * with activations kept in registers.  Logical row r = g*(T0+T1)+t reads
 * x_main[g, t, :] for t < T0 and x_tail[g, t-T0, :] otherwise, so the reference's
 * torch.cat([obs, obs_next], dim=1) copy is never materialised.
 *   x_main [G, T0, D], x_tail [G, T1, D] (T1 may be 0, x_tail NULL)
 *   zmean/zstd [D] or NULL (no z-filter)
 *   packed: weights repacked by smx_mlp3_pack_f32 (K-chunked, zero padded)
 *   out [G*(T0+T1), OUT]; out_act SMX_ACT_NONE (critic) or SMX_ACT_TANH (actor mean)
 * Supported: H1 <= 320, H2 <= 224, OUT <= 32, any D >= 1. */
size_t smx_mlp3_packed_bytes(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_mlp3_pack_f32(const smx_mlp3_t* net, float* packed, size_t packed_bytes,
                      smx_stream_t stream);
/* the same launch also refreshing the z-filter statistics the pass that follows reads (exactly
 * smx_zfilter_stats_f32: mean_out / std_out [D] from the running sums) */
int smx_mlp3_pack_zstats_f32(const smx_mlp3_t* net, float* packed, size_t packed_bytes,
                             const float* running_sum, const float* running_sumsq, const float* count,
                             int32_t D, float eps, float* mean_out, float* std_out, smx_stream_t stream);
int smx_mlp3_forward_fused_f32(const float* packed, int32_t D, int32_t H1, int32_t H2,
                               int32_t OUT, const float* x_main, const float* x_tail,
                               int64_t G, int32_t T0, int32_t T1, const float* zmean,
                               const float* zstd, float* out, int32_t out_act,
                               smx_stream_t stream);
/* The same pass with layer 1 of the 16-row kernel on 3-way split-bf16 MFMA (split_bf16 != 0): W1 and the filtered x
 * are each split into three bf16 planes that sum to the fp32 value exactly, and six of the nine plane products are
 * accumulated in fp32 (everything down to 2^-23 of a product; DESIGN.md 3.1 states the measured error against
 * float64).  smx_mlp3_pack*_f32 write the planes of W1 behind the fp32 image when `packed` has
 * smx_mlp3_packed_bytes bytes; packed_bytes is that size.  Layers 2 and 3 are fp32 MFMA as before.  The fp32 kernel
 * of smx_mlp3_forward_fused_f32 runs instead when split_bf16 is 0, the planes are missing, exact-z-filter mode is on
 * or the shape is off the 16-row kernel.  A non-finite x or weight makes the affected outputs non-finite on both
 * paths; an Inf may come out as NaN here (Inf - Inf in the residual planes). */
int smx_mlp3_forward_fused_split_f32(const float* packed, size_t packed_bytes, int32_t split_bf16, int32_t D,
                                     int32_t H1, int32_t H2, int32_t OUT, const float* x_main,
                                     const float* x_tail, int64_t G, int32_t T0, int32_t T1, const float* zmean,
                                     const float* zstd, float* out, int32_t out_act, smx_stream_t stream);

/* --- one dense layer on FP32 MFMA (small-batch epochs) ------------------------
 * C[M,N] = act(A[M,K] . B[N,K]^T + bias[N]); every epoch-loop GEMM of
 * _clip_update/_adapt_update/_value_update (ppo.py:227-353) is an instance.
 * a_kcontig: A(m,k) = A[m*lda+k] (1) or A[k*lda+m] (0); same for B.
 * relu_mask (optional, [M,ldc]): C *= (relu_mask > 0)  -- ReLU backward. */
int smx_linear_f32(const float* A, int32_t lda, int32_t a_kcontig, const float* B,
                   int32_t ldb, int32_t b_kcontig, const float* bias, float* C,
                   int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t act,
                   const float* relu_mask, const int32_t* stop_flag, smx_stream_t stream);

/* Up to 9 INDEPENDENT dense problems in ONE launch -- the layers (or weight gradients) of one dependency level of an
 * update, e.g. DDPG's target-actor, critic and actor first layers (surreal/learner/ddpg.py:244-352 issues them as
 * separate ATen calls).  kind 0: C [M,N] = act(A . B^T + bias) (* (relu_mask > 0)), arguments as smx_linear_f32;
 * kind 1: C = dW [M,N] = A^T . B with A = dZ [K rows, >= M] (stride lda), B = X [K rows, >= N] (stride ldb),
 * dbias [M] = column sums of dZ (nullable), arguments as smx_linear_wgrad_f32. */
typedef struct smx_linear_job {
    int32_t kind, act;
    const float* A; const float* B; const float* bias; const float* relu_mask;
    float* C; float* dbias;
    int32_t lda, ldb, ldc, a_kcontig, b_kcontig, M, N, K;
    const int32_t* stop_flag;
} smx_linear_job_t;
int smx_linear_multi_f32(const smx_linear_job_t* jobs, int32_t njobs, smx_stream_t stream);

/* Weight gradient of one dense layer: dW[M,N] = dZ^T . X, db[M] = column sums of dZ (db may be
 * NULL); dZ [rows, .] with row stride ldz, X [rows, .] with row stride ldx (what
 * loss.backward() produces for nn.Linear, ddpg.py:308,331). */
int smx_linear_wgrad_f32(const float* dZ, int32_t ldz, const float* X, int32_t ldx, float* dW,
                         int32_t ldw, float* db, int32_t M, int32_t N, int32_t rows,
                         smx_stream_t stream);

/* The same with the rows cut into chunks (split-K) when rows >> 1000 -- the weight gradients of
 * the LSTM / CNN stems run over B*T or B*E*pixels rows.  ws: caller's workspace of at least
 * smx_linear_wgrad_ws_floats(M, N, rows) floats (0 = the plain entry point is used); partial
 * tiles are added in a fixed order (deterministic).  ws == NULL falls back to the plain call. */
int64_t smx_linear_wgrad_ws_floats(int32_t M, int32_t N, int32_t rows);
int smx_linear_wgrad_splitk_f32(const float* dZ, int32_t ldz, const float* X, int32_t ldx,
                                float* dW, int32_t ldw, float* db, int32_t M, int32_t N,
                                int32_t rows, float* ws, int64_t ws_floats, smx_stream_t stream);
/* TWO weight gradients from the same dZ [rows, M] (the LSTM's dW_ih = dgates^T . x and dW_hh = dgates^T . h_prev,
 * ppo_net.py:143-152 under loss.backward()): dW1 [M, N1] = dZ^T . X1, dW2 [M, N2] = dZ^T . X2 (dense, row stride N),
 * db1 / db2 [M] column sums (nullable).  One split-K launch for both when both run on the 32 x 32-tile kernel
 * (ws >= smx_linear_wgrad_ws_floats(M, N1, rows) + ..(M, N2, rows) floats), otherwise exactly two
 * smx_linear_wgrad_splitk_f32 calls; results are those of the two calls, bit for bit. */
int smx_linear_wgrad_splitk_pair_f32(const float* dZ, int32_t ldz, int32_t M, int32_t rows, const float* X1,
                                     int32_t ldx1, float* dW1, float* db1, int32_t N1, const float* X2,
                                     int32_t ldx2, float* dW2, float* db2, int32_t N2, float* ws,
                                     int64_t ws_floats, smx_stream_t stream);

/* One MLP forward or backward "job" for the multi-network entry points below: PPO's actor and
 * critic are independent networks updated in lock-step epochs (ppo.py:541-562), so their
 * layer-l GEMMs share one launch.  Forward uses net/x/rows/h1/h2/out/out_act; backward uses
 * net/x/rows/h1/h2/dz3 (in) and dz2/dz1/grads/sumsq_partials (out).  stop_flag (device int,
 * may be NULL): non-zero turns this job's part of every launch into a no-op. */
typedef struct {
    const smx_mlp3_t* net;
    const float* x;
    int64_t rows;
    float* h1;
    float* h2;
    float* out;
    int32_t out_act;
    int32_t out_ld;      /* row stride of `out` in floats; 0 = OUT (dense) */
    const float* dz3;
    float* dz2;
    float* dz1;
    float* grads;
    float* sumsq_partials;
    const int32_t* stop_flag;
    /* optional transposed copies, all [features, rows] with row stride ldT floats (>= rows; 0 means
     * rows -- pad it, e.g. rows + 16: a power-of-two stride puts all 32 rows of a fragment load
     * on the same cache set / memory channel): the forward writes
     * h1T / h2T, the backward writes dz2T / dz1T; when xT, dz3T and all four are given the
     * weight-gradient GEMMs read K-contiguous operands (16-byte loads) instead of strided ones */
    float* h1T;
    float* h2T;
    const float* xT;
    const float* dz3T;
    float* dz2T;
    float* dz1T;
    int64_t ldT;
} smx_mlp3_job_t;
/* forward: 1 <= njobs <= 4 (one launch per layer for all jobs; jobs may differ in rows and
 * shapes -- e.g. actor, critic, reference actor and the critic over the obs_next rows at the
 * start of a learn); backward: 1 <= njobs <= 3 (three launches: dz2, dz1, all weight gradients) */
int smx_mlp3_forward_multi_f32(const smx_mlp3_job_t* jobs, int32_t njobs, smx_stream_t stream);
int smx_mlp3_backward_multi_f32(const smx_mlp3_job_t* jobs, int32_t njobs, smx_stream_t stream);

/* MLP forward keeping the hidden activations (needed by the backward):
 * h1 [rows,H1], h2 [rows,H2], out [rows,OUT] = act(layer 3). */
int smx_mlp3_forward_f32(const smx_mlp3_t* net, const float* x, int64_t rows, float* h1,
                         float* h2, float* out, int32_t out_act,
                         const int32_t* stop_flag, smx_stream_t stream);
/* The same over MANY rows (the MLPs on top of an LSTM / CNN stem: rows = B * E ~ 10^5 per epoch; the reference calls
 * the same nn.Sequential, surreal/model/ppo_net.py:284-315): ONE launch of the fused 16-row kernel -- x read once,
 * activations from the accumulators to h1 / h2 once and on to the next layer in registers -- behind a repack of the
 * weights into `packed` (smx_mlp3_packed_bytes(D, H1, H2, OUT) bytes, 16-byte aligned; contents are scratch).
 * out [rows, OUT] with row stride out_ld floats (0 = OUT).  Returns SMX_E_UNSUPPORTED outside the kernel's fast path
 * (smx_mlp3_forward_rows_supported: D, H1, H2 multiples of 4, 64 < H1 <= 320, 64 < H2 <= 224, OUT <= 32; x, h1, h2
 * 16-byte aligned) -- the caller then uses smx_mlp3_forward_f32.  Results equal the layered path's within fp32
 * rounding (another summation order), not bit for bit. */
int32_t smx_mlp3_forward_rows_supported(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_mlp3_forward_rows_f32(const smx_mlp3_t* net, const float* x, int64_t rows, float* h1, float* h2,
                              float* out, int32_t out_act, int32_t out_ld, float* packed, size_t packed_bytes,
                              const int32_t* stop_flag, smx_stream_t stream);

/* MLP backward from dz3 = dLoss/d(pre-activation of layer 3) [rows,OUT]:
 *   grads  flat [H1*D + H1 + H2*H1 + H2 + OUT*H2 + OUT] in (W1,b1,W2,b2,W3,b3) order
 *   dz2 [rows,H2], dz1 [rows,H1] scratch; sumsq_partials [smx_mlp3_backward_partials()]
 *   receives per-tile sums of squares of the gradients (for clip_grad_norm_). */
int32_t smx_mlp3_backward_partials(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_mlp3_backward_f32(const smx_mlp3_t* net, const float* x, const float* h1,
                          const float* h2, const float* dz3, int64_t rows, float* dz2,
                          float* dz1, float* grads, float* sumsq_partials,
                          const int32_t* stop_flag, smx_stream_t stream);
/* The same for MANY rows (the MLP on top of an LSTM / CNN stem runs over B x T rows, loss.backward() of
 * surreal/learner/ppo.py:227-353 with surreal/model/ppo_net.py:143-152 in front): the rows of every weight gradient are cut
 * into chunks (one workgroup per (tile, chunk), partial tiles in ws), one segmented reduce forms the six gradients in a
 * fixed order.  ws: smx_mlp3_backward_ws_floats() floats (0: few rows, no split); with ws == NULL or too small this IS
 * smx_mlp3_backward_f32 without sum-of-squares partials. */
int64_t smx_mlp3_backward_ws_floats(int32_t D, int32_t H1, int32_t H2, int32_t OUT, int64_t rows);
int smx_mlp3_backward_splitk_f32(const smx_mlp3_t* net, const float* x, const float* h1, const float* h2,
                                 const float* dz3, int64_t rows, float* dz2, float* dz1, float* grads, float* ws,
                                 int64_t ws_floats, const int32_t* stop_flag, smx_stream_t stream);
/* ... with the three data-gradient products as ONE fused launch in front of the split-K weight gradients
 * (csrc/smx_mlp3_bwd16.hip: a wavefront owns 16 rows from dz3 to dx, dz2 / dz1 go from the accumulators to memory once
 * and on in registers; the weight gradients of the hidden layers run with the whole dW in one workgroup's registers,
 * csrc/smx_wgrad.hip).  dx [rows, D] (may be NULL): the gradient with respect to the MLP's input -- what the layered
 * path leaves to a separate smx_linear_f32(dz1, W1) call.  packedT: scratch of smx_mlp3_dgrad_rows_ws_floats() floats,
 * 16-byte aligned.  Returns SMX_E_UNSUPPORTED -- nothing launched -- outside the fused kernel's shapes
 * (smx_mlp3_dgrad_rows_supported: D <= 128, D / H1 / H2 multiples of 4, 64 < H1 <= 320, 64 < H2 <= 224, OUT <= 32),
 * for unaligned operands, or when rows are too few for a split-K workspace: the caller then uses the call above.
 * Same sums in another order: equal within fp32 rounding, not bit for bit. */
int32_t smx_mlp3_dgrad_rows_supported(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int64_t smx_mlp3_dgrad_rows_ws_floats(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_mlp3_backward_rows_f32(const smx_mlp3_t* net, const float* x, const float* h1, const float* h2,
                               const float* dz3, int64_t rows, float* dz2, float* dz1, float* dx, float* grads,
                               float* ws, int64_t ws_floats, float* packedT, int64_t packedT_floats,
                               const int32_t* stop_flag, smx_stream_t stream);

/* --- windowed GAE / n-step returns (surreal/learner/ppo.py:387-418) ----------
 * values [B,N+1] RAW critic outputs -- or, when values_tail != NULL, values [B,N] for the N
 * steps and values_tail [B] for obs_next (lets the caller evaluate the two row sets with
 * different kernels); the done-mask values[:,1:] *= 1-dones (ppo.py:387) is applied inside.  H = N -> non-RNN branch (E = 1);
 * H = rnn.horizon -> RNN branch, E = N-H+1 sliding windows.
 * gamma_pow/lam_pow [H] = torch.pow(gamma|lam, arange) as the reference builds
 * them (ppo.py:372-374); gamma_H = gamma**H.
 * adv [B,E] (un-normalised), ret [B,E]. */
int smx_windowed_gae_returns_f32(const float* values, const float* values_tail,
                                 const float* rewards,
                                 const float* dones, const float* gamma_pow,
                                 const float* lam_pow, float gamma, float gamma_H,
                                 int32_t B, int32_t N, int32_t H, float* adv, float* ret,
                                 smx_stream_t stream);
/* smx_windowed_gae_returns_f32 + smx_moments_f32 + smx_adv_normalize_f32 in ONE launch (single rank):
 * the last workgroup to finish forms the batch moments of adv (adv_moments[3]) and normalises adv in
 * place with max(std_unbiased, min_std).  ticket: one int32 in device memory, zero before the first
 * call (the kernel leaves it zero). */
int smx_windowed_gae_norm_f32(const float* values, const float* values_tail, const float* rewards,
                              const float* dones, const float* gamma_pow, const float* lam_pow,
                              float gamma, float gamma_H, int32_t B, int32_t N, int32_t H, float* adv,
                              float* ret, float* adv_moments, float min_std, int32_t* ticket,
                              smx_stream_t stream);
/* rewards * reward_scale and RewardFilter.forward + RewardFilter.update (surreal/learner/ppo.py:452-455,
 * surreal/model/reward_filter.py:33-57) in ONE launch, legal under graph capture:
 *   x = rewards[i] * scale;  out[i] = use_filter ? clamp((x - mean) / std, -5, 5) : x   with
 *   mean = state[1] / state[0], std = max(sqrt(state[2] / state[0] - mean^2), eps) taken BEFORE the update;
 *   update_state: state[0] += n, state[1] += sum(x), state[2] = sum(x*x)  (assigned, reward_filter.py:42).
 * state = {count, running_sum, running_sumsq} (3 floats in device memory); sums (nullable): {n, sum(x),
 * sum(x*x)} of this call (what several ranks exchange before they update the state themselves);
 * partials: smx_reward_filter_partials() doubles of scratch; ticket: one int32, zero before the first call
 * (left zero).  out may alias rewards. */
int smx_reward_filter_f32(const float* rewards, int64_t n, float scale, int32_t use_filter, float* state,
                          float eps, int32_t update_state, float* out, float* sums, double* partials,
                          int32_t* ticket, smx_stream_t stream);
int32_t smx_reward_filter_partials(void);
/* What PPOLearner._optimize does after its epoch loops (ppo.py:565-584) in ONE launch (single rank):
 *   smx_value_loss_finalize_f32 (v_partials [n_epochs, nblk, 8] -> v_stats rows; n_epochs may be 0),
 *   smx_moments_f32 over the return targets (ret_moments[3]), smx_zfilter_update_f32 on x [rows, D]
 *   (x == NULL: no z-filter), then -- by the last workgroup to finish, so it reads the updated sums --
 *   smx_ppo_final_stats_f32 (out4).  ticket as above. */
typedef struct smx_learn_epilogue {
    const float* x; int64_t ldx; int64_t rows; int32_t D; int32_t A;
    float* running_sum; float* running_sumsq; float* count; float count_rows; int32_t n_epochs;
    const float* ret; int64_t n_ret; float* ret_moments;
    const float* v_partials; int32_t nblk; int32_t stats_stride; float* v_stats;
    const float* log_var; float* out4; int32_t* ticket;
} smx_learn_epilogue_t;
int smx_ppo_learn_epilogue_f32(const smx_learn_epilogue_t* args, smx_stream_t stream);
/* moments[3] = {n, mean, M2 = sum (x-mean)^2} over n values (two-pass, one workgroup) */
int smx_moments_f32(const float* x, int64_t n, float* moments, smx_stream_t stream);
/* Chan-merge k per-rank moment triples [k,3] into out[3] (multi-GPU advantage norm) */
int smx_moments_merge_f32(const float* parts, int32_t k, float* out, smx_stream_t stream);
/* x = (x - mean) / max(std_unbiased, min_std)   (ppo.py:402-405, 413-416) */
int smx_adv_normalize_f32(float* x, int64_t n, const float* moments, float min_std,
                          smx_stream_t stream);

/* --- PPO device-resident control block ---------------------------------------
 * Mutable scalars read by the loss / optimiser kernels (see file header). */
typedef struct {
    float lr_actor, lr_critic;  /* current learning rates (ppo.py:576) */
    float beta, eta;            /* adapt mode: KL penalty, cutoff coeff (ppo.py:108-112) */
    float clip_eps;             /* clip mode (ppo.py:115) */
    float kl_target;            /* ppo.py:95 */
    float actor_max_norm, critic_max_norm; /* <=0: no clipping (ppo.py:154-157) */
    float actor_weight_decay, critic_weight_decay;
    int32_t adam_step_actor, adam_step_critic; /* torch.optim.Adam 'step' state */
    int32_t stop_flag;     /* set when KL(ref||curr) > 4*kl_target (ppo.py:556-557) */
    int32_t epochs_done;   /* policy epochs actually applied this learn() */
    int32_t reserved[2];   /* [0]: error word of a peer exchange (smx_xchg_*: pass its address as `err`); [1]: raised by
                              smx_epoch_fwdbwd_f32 when its in-launch wait timed out.  Either makes smx_clip_adam* skip
                              the step. */
} smx_ppo_ctrl_t;

/* per-epoch statistics slots (floats) written by the kernels; see ppo.py:219-224,278-284 */
enum {
    SMX_PS_SURR = 0,     /* _surr_loss */
    SMX_PS_LOSS = 1,     /* _clip_surr_loss | _kl_loss_adapt */
    SMX_PS_ENTROPY = 2,  /* _entropy */
    SMX_PS_KL = 3,       /* mean KL(ref||learn) at this forward */
    SMX_PS_GRADNORM = 4, /* grad_norm_actor */
    SMX_PS_LB = 5,       /* mean behave likelihood */
    SMX_PS_ISW = 6,      /* mean L_learn/(L_behave+1e-4) */
    SMX_PS_REFBEH = 7,   /* mean KL(ref||behave) */
    SMX_PS_STRIDE = 8
};
enum { SMX_VS_LOSS = 0, SMX_VS_EXPVAR = 1, SMX_VS_GRADNORM = 2, SMX_VS_STRIDE = 4 };

/* --- DiagGauss surrogate losses, forward + backward to dz3 --------------------
 * Replaces DiagGauss.loglikelihood/likelihood/kl/entropy (ppo_net.py:29-72) and
 * _clip_loss / _adapt_loss (ppo.py:194-285) including their autograd backward down to
 * the pre-tanh output of the actor's last layer and to log_var.
 *   mean [rows,A] = tanh output of the actor; log_var [A]; actions [rows, lda_act..]
 *   behave [rows,2A] = [mean|std] (row stride ld_beh), ref [rows,2A] (stride ld_ref)
 *   adv [rows] (row stride 1)
 *   row_partials [nblk, SMX_LOSS_PARTIALS(A)], nblk = smx_ppo_loss_blocks(rows)
 *   g_surr, g_kl [rows,A]: d(sum_r surr_r)/dz3 and d(sum_r KL_r)/dz3, combined by
 *   smx_ppo_loss_finalize_f32 once the batch means are known.
 * n_total = global number of rows over all ranks (the mean's denominator). */
int32_t smx_ppo_loss_blocks(int64_t rows);
int32_t smx_ppo_loss_partial_stride(int32_t A);
int smx_ppo_policy_loss_f32(int32_t mode, const float* mean, const float* log_var,
                            const float* actions, int32_t ld_act, const float* behave,
                            int32_t ld_beh, const float* ref, int32_t ld_ref,
                            const float* adv, int64_t rows, int32_t A,
                            const smx_ppo_ctrl_t* ctrl, float* g_surr, float* g_kl,
                            float* row_partials, smx_stream_t stream);
/* Reduce the partials (optionally already all-reduced across ranks: pass nblk = 1 and a
 * summed partial row), write stats[SMX_PS_*], the combined dz3 = (g_surr + c*g_kl)/n_total
 * and the log_var gradient.  When `check_stop` is non-zero it evaluates the KL early-exit
 * test of the PREVIOUS update (mean KL(ref||curr) > 4*kl_target, ppo.py:553-557) and raises
 * ctrl->stop_flag.  When `will_update` is non-zero and the flag stays clear it advances
 * ctrl->adam_step_actor and ctrl->epochs_done for the optimiser step that follows.
 * dlogvar_sumsq (optional) receives sum(dlogvar^2), one more clip_grad_norm_ partial.
 * dz3_t (optional) receives the transposed copy dz3_t[a * ld_t + r] (see smx_mlp3_job_t).
 * No-op when ctrl->stop_flag is already set on entry. */
/* Folds nblk partial rows (row stride = stride floats) to nout rows in front of smx_ppo_loss_finalize_f32: out[j] = the
 * sum of rows [j R, (j + 1) R), R = ceil(nblk / nout), in a fixed order.  For the policies on a stem, whose B * E ~ 10^5
 * rows leave thousands of partial rows that every workgroup of the finalize would walk.  No-op when ctrl (may be NULL)
 * has its stop flag set. */
int smx_ppo_partials_fold_f32(const float* row_partials, int32_t nblk, int32_t stride, float* out, int32_t nout,
                              const smx_ppo_ctrl_t* ctrl, smx_stream_t stream);
int smx_ppo_loss_finalize_f32(int32_t mode, const float* row_partials, int32_t nblk,
                              const float* g_surr, const float* g_kl, const float* log_var,
                              int64_t rows, int64_t n_total, int32_t A, smx_ppo_ctrl_t* ctrl,
                              int32_t check_stop, int32_t will_update, float* dz3,
                              float* dz3_t, int64_t ld_t, float* dlogvar, float* dlogvar_sumsq,
                              float* stats, smx_stream_t stream);

/* --- value loss (ppo.py:311-332): loss = mean((V-ret)^2), explained variance ---
 * dz3[r] = 2 (V_r - ret_r) / n_total ; partials [nblk, 8] = per-block
 * {n, mean_d, M2_d, mean_ret, M2_ret, sum d^2, 0, 0} with d = ret - V (mergeable moments).
 * Advances ctrl->adam_step_critic when will_update != 0. */
int32_t smx_value_loss_blocks(int64_t rows);
int smx_value_loss_f32(const float* values, const float* returns, int64_t rows,
                       int64_t n_total, float* dz3, float* partials, smx_ppo_ctrl_t* ctrl,
                       int32_t will_update, smx_stream_t stream);
/* The three entry points above in one call, for a single-GPU lock-step epoch (n_total == rows;
 * with several ranks the loss partials must be all-reduced between the loss and its finalize, so
 * the separate entry points are used): the policy loss and the value loss share ONE launch
 * (disjoint workgroup ranges), the policy finalize follows.  Results are bit-identical to the
 * three separate calls.  Field meanings as there; values == NULL skips the value loss. */
typedef struct smx_ppo_losses {
    int32_t mode, A;
    const float* mean;
    const float* log_var;
    const float* actions;
    const float* behave;
    const float* ref;
    const float* adv;
    int32_t ld_act, ld_beh, ld_ref, check_stop;
    int64_t rows;
    float* g_surr;
    float* g_kl;
    float* row_partials;
    float* dz3;
    float* dz3_t;
    int64_t ld_t;
    float* dlogvar;
    float* dlogvar_sumsq;
    float* stats;
    const float* values;
    const float* returns;
    float* v_dz3;
    float* v_partials;
    int32_t will_update, v_will_update;
} smx_ppo_losses_t;
int smx_ppo_epoch_losses_f32(const smx_ppo_losses_t* args, smx_ppo_ctrl_t* ctrl,
                             smx_stream_t stream);
/* Data-parallel lock-step epoch (several ranks): ONE all-reduce per epoch instead
 * of one for the loss sums and one for the gradients.  The gradient of either loss is linear in
 * dz3 = (g_surr + c_kl * g_kl) / n_total, and only c_kl needs the GLOBAL mean KL (ppo.py:272-276),
 * so the backward pass runs on the two right-hand sides separately and the combination happens
 * after the all-reduce:
 *   smx_ppo_epoch_losses_dp_f32   the launch of smx_ppo_epoch_losses_f32 WITHOUT its finalize:
 *                                 args->g_surr / g_kl receive the tiles already divided by
 *                                 n_total (+ transposed copies [A, ld_t] when g_surr_t != NULL),
 *                                 args->row_partials the block sums, the value loss uses n_total;
 *                                 args->dz3 / dz3_t / dlogvar / dlogvar_sumsq / stats are ignored
 *   (backward on both right-hand sides; all-reduce of [G_surr | G_critic | G_kl | row_partials])
 *   smx_ppo_epoch_combine_f32     grads_a[i] += c_kl * grads_kl[i] for i < n_mlp (adapt; clip:
 *                                 grads_kl may be NULL), grads_a[n_mlp + a] = log_var's gradient,
 *                                 stats / KL early exit / step counters exactly as
 *                                 smx_ppo_loss_finalize_f32, and the sum-of-squares partials of
 *                                 both groups for smx_clip_adam_step_pair_f32:
 *                                 sumsq_a [smx_sumsq_blocks(n_a)], sumsq_c [smx_sumsq_blocks(n_c)]
 *                                 (grads_c == NULL: actor only). */
int smx_ppo_epoch_losses_dp_f32(const smx_ppo_losses_t* args, int64_t n_total, float* g_surr_t,
                                float* g_kl_t, smx_ppo_ctrl_t* ctrl, smx_stream_t stream);
typedef struct smx_ppo_combine {
    int32_t mode, A;
    const float* row_partials; /* [nblk, 8 + 2A], summed over ranks */
    int32_t nblk;
    int32_t check_stop;
    int64_t n_total;
    const float* log_var;
    float* stats;
    float* grads_a;
    const float* grads_kl;
    int64_t n_mlp, n_a;
    float* sumsq_a;
    const float* grads_c;
    int64_t n_c;
    float* sumsq_c;
    int32_t will_update, reserved;
} smx_ppo_combine_t;
int smx_ppo_epoch_combine_f32(const smx_ppo_combine_t* args, smx_ppo_ctrl_t* ctrl,
                              smx_stream_t stream);
/* the weight-gradient launch of smx_mlp3_backward_multi_f32 alone (all three layers of up to 3 jobs
 * in ONE launch): dW_l = dz_l^T . input_l, db_l = column sums, per-tile sums of squares.  Needs the
 * transposed operands (xT, h1T, h2T, dz3T, dz2T, dz1T, ldT) the fused epoch kernels write. */
int smx_mlp3_wgrad_multi_f32(const smx_mlp3_job_t* jobs, int32_t njobs, smx_stream_t stream);

/* --- fused row-block epoch kernels -------------------------------------------------------------
 * One policy / value epoch of PPOLearner._optimize (surreal/learner/ppo.py:541-562; losses
 * :194-353; forward_actor / forward_critic surreal/model/ppo_net.py:253-315) on a few thousand
 * rows as FOUR dependent launches instead of nine: a workgroup owns 16 rows of one network and runs
 *   smx_epoch_forward_f32   layer 1 -> 2 -> 3 (FP32 MFMA 16x16x4, activations through LDS) and the
 *                           job's loss on those rows: SMX_EPOCH_LOSS_POLICY = DiagGauss likelihoods /
 *                           KL / surrogate -> loss->g_surr, g_kl [rows, A] and the block partial
 *                           sums loss->row_partials [smx_epoch_blocks(rows), 8 + 2A];
 *                           SMX_EPOCH_LOSS_VALUE = loss->v_dz3 [rows] = 2 (V - ret) / n_total and
 *                           loss->v_partials [smx_epoch_blocks(rows), 8] (mergeable moments, the
 *                           layout smx_value_loss_finalize_f32 reads).  h1T / h2T ([H, ldT]) receive
 *                           the hidden activations transposed; out ([rows, OUT], row stride out_ld)
 *                           the network output (optional).  A job with a raised stop_flag is skipped.
 *   smx_epoch_backward_f32  policy job: batch means from the partial rows -> KL coefficient
 *                           (ppo.py:272-276), loss->stats / dlogvar / dlogvar_sumsq, the KL early
 *                           exit and step counters exactly as smx_ppo_loss_finalize_f32, then
 *                           dz3 = (g_surr + c_kl g_kl) / n_total; value job: dz3 = job.dz3 [rows].
 *                           dz2 = (dz3 . W3) * relu'(h2), dz1 = (dz2 . W2) * relu'(h1) written
 *                           transposed (dz3T [OUT, ldT] policy only, dz2T, dz1T).  With
 *                           loss->will_update == 0 (the final, forward-only pass) only the
 *                           statistics / early-exit part runs (one job, one workgroup).
 * followed by smx_mlp3_wgrad_multi_f32 and smx_clip_adam_step_pair_f32.
 * Requirements (smx_epoch_supported): H1, H2 multiples of 4, OUT <= 32, x dense [rows, D]; W2, W3,
 * b1, b2 (and x when D % 4 == 0) 16-byte aligned.  loss->mean / dz3 / dz3_t / values are not used (the tiles stay on chip). */
/* backward only, data-parallel epochs (several ranks): SMX_EPOCH_RHS_SURR / _KL run the actor's data
 * gradients on ONE right-hand side each, dz3 = g_surr / n_total or g_kl / n_total, with no batch means
 * and no statistics (the loss gradient is linear in dz3; smx_ppo_epoch_combine_f32 forms G_surr + c_kl
 * G_kl after the all-reduce) */
enum { SMX_EPOCH_LOSS_NONE = 0, SMX_EPOCH_LOSS_POLICY = 1, SMX_EPOCH_LOSS_VALUE = 2, SMX_EPOCH_RHS_SURR = 3,
       SMX_EPOCH_RHS_KL = 4 };
typedef struct smx_epoch_job {
    const smx_mlp3_t* net;
    const float* x;
    int64_t rows;
    float* h1T;
    float* h2T;
    int64_t ldT;
    float* out;
    int32_t out_ld;   /* 0 = OUT */
    int32_t out_act;
    int32_t loss;     /* SMX_EPOCH_LOSS_* */
    int32_t reserved;
    const int32_t* stop_flag;
    const float* dz3; /* backward, value job: [rows] */
    float* dz3T;
    float* dz2T;
    float* dz1T;
    const float* packed; /* forward: the net's weights as smx_epoch_pack_f32 lays them out */
} smx_epoch_job_t;
/* The forward kernel reads the weights in MFMA fragment order: [tile of 16 features][32-wide K chunk]
 * [half][lane][4], zero padded to whole tiles and an even chunk count, so that every load instruction
 * reads one contiguous KB (from the row-major matrices a fragment load touches 16 cache lines and the
 * loop runs at half the MFMA rate).  smx_epoch_pack_f32 writes that copy for up to 4 networks in one
 * launch; the epoch loop keeps it current by repacking after every optimiser step. */
typedef struct smx_epoch_pack {
    const smx_mlp3_t* net;
    float* packed; /* smx_epoch_packed_floats(D, H1, H2, OUT) floats, 16-byte aligned */
} smx_epoch_pack_t;
int64_t smx_epoch_packed_floats(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_epoch_pack_f32(const smx_epoch_pack_t* items, int32_t n, smx_stream_t stream);
/* What PPOLearner._optimize prepares once per learn for its epoch loops (ppo.py:527-539), in ONE launch:
 *   xn  [rows, D] = ZFilter.forward(obs0) with the model's statistics (zmean / zstd from
 *        smx_zfilter_stats_f32; NULL: plain copy), xnT [D, ldT] its transposed copy (optional);
 *   xr  [rows, D] = the same through the REFERENCE policy's filter, straight from its running sums
 *        (ref_filter != 0; else plain copy)  -- ref_target_model.forward_actor's input (ppo.py:539);
 *   xnext [rows, D] = ZFilter.forward(obs_next rows) (optional: the critic's tail rows, ppo.py:380);
 *   ref_std [rows, A] (row stride ld_ref) = exp(ref_log_var): the std columns of ref_pol (builders.py:126-129);
 *   the packed weight copies of n_pack networks (smx_epoch_pack_f32);
 *   zero_words[0 .. n_zero) = 0 (the control block's stop flag / epoch counter / statistics rows).
 * obs0 / obs_next are row-strided views (ld in floats, e.g. N * D: step 0 of every sub-trajectory). */
typedef struct smx_epoch_prep {
    const float* obs0; int64_t ld_obs0; int64_t rows; int32_t D; int32_t A;
    const float* zmean; const float* zstd;
    float* xn; float* xnT; int64_t ldT;
    const float* ref_sum; const float* ref_sumsq; const float* ref_count; float ref_eps; int32_t ref_filter;
    float* xr;
    const float* obs_next; int64_t ld_next; float* xnext;
    const float* ref_log_var; float* ref_std; int64_t ld_ref;
    int32_t* zero_words; int32_t n_zero; int32_t n_pack;
    smx_epoch_pack_t pack[4];
} smx_epoch_prep_t;
int smx_epoch_prepare_f32(const smx_epoch_prep_t* args, smx_stream_t stream);
struct smx_ppo_losses;
int32_t smx_epoch_blocks(int64_t rows);
int32_t smx_epoch_supported(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_epoch_forward_f32(const smx_epoch_job_t* jobs, int32_t njobs, const struct smx_ppo_losses* loss,
                          smx_ppo_ctrl_t* ctrl, int64_t n_total, smx_stream_t stream);
int smx_epoch_backward_f32(const smx_epoch_job_t* jobs, int32_t njobs, const struct smx_ppo_losses* loss,
                           smx_ppo_ctrl_t* ctrl, int64_t n_total, smx_stream_t stream);
/* smx_epoch_forward_f32 + smx_epoch_backward_f32 of an UPDATING epoch (loss->will_update != 0; surreal/learner/
 * ppo.py:209-248 / 266-309 / 323-353 up to the data gradients) in ONE launch: a workgroup carries its 16 rows through
 * the three layers, the loss and back to dz2 / dz1 while the activations (the ReLU masks) and the loss's gradient
 * terms are still in LDS.  The batch means the adapt loss needs (c_kl = beta + 2 eta max(0, KL - 2 kl_target),
 * ppo.py:272-276) travel INSIDE the launch: every actor workgroup stores its block's KL sum together with a "there"
 * bit as ONE 8-byte device-scope word (kl_slots[block]), multiplies both right-hand sides (g_surr / n, g_kl / n)
 * through the output layer meanwhile, then reads the slots of all blocks (bounded wait: 0.25 s, then ctrl->reserved[1]
 * is raised and the optimiser launch skips its step), adds them in a fixed order and continues with
 * dz2 = (W3^T g_surr + c_kl W3^T g_kl) * relu'(h2) -- the combination is formed one layer later than
 * smx_epoch_backward_f32 forms it (rounding differs in the last bit, the contract is the same).  Clip mode: no
 * gradient depends on the batch, nobody waits.  The epoch's scalars (statistics, log_var's gradient, early-exit flag,
 * step counters) are formed once, by the last workgroup of the grid after its own rows, from the partial rows
 * (device-scope stores; *sync_word counts the actor workgroups whose row is complete).  loss->g_surr / g_kl are not
 * written (the tiles stay in LDS).
 * Jobs: SMX_EPOCH_LOSS_POLICY (at most one) and / or SMX_EPOCH_LOSS_VALUE, fields as for the two calls it
 * replaces.  sync_word: one int32 per launch; kl_slots: smx_epoch_blocks(rows of the policy job) 8-byte words per
 * launch; both zero on entry (the caller clears them once per learn).
 * smx_epoch_fwdbwd_supported: smx_epoch_supported and H2 <= 384 and the larger LDS carve-up fits.
 * Adapt mode needs every actor workgroup of the launch resident at once (one per CU): a launch with more workgroups than
 * the device has CUs runs as smx_epoch_forward_f32 + smx_epoch_backward_f32 (two launches, same results). */
int32_t smx_epoch_fwdbwd_supported(int32_t D, int32_t H1, int32_t H2, int32_t OUT);
int smx_epoch_fwdbwd_f32(const smx_epoch_job_t* jobs, int32_t njobs, const struct smx_ppo_losses* loss,
                         smx_ppo_ctrl_t* ctrl, int64_t n_total, int32_t* sync_word, uint64_t* kl_slots,
                         smx_stream_t stream);
/* Pair mode of the two calls above: every 16-row block is carried by TWO workgroups on two CUs of one XCD.  Half h takes
 * the feature tiles t with t % 2 == h of layer 1, layer 2 and dz1 -- each CU issues half of the MFMAs and streams half of
 * the packed weights -- and the halves hand their h1 and h2 tiles to each other through `xchg` (every element as one
 * 8-byte device-scope word, value | hand-over count << 32, polled by its reader: no fence, no flag round trip; a wait
 * is bounded at 0.25 s like the batch KL's, then ctrl->reserved[1] is raised).  Layer 3, the loss and W3^T dz3 are done by both halves; results that exist once per
 * block leave from half 0.  A tile's arithmetic does not depend on which workgroup carries it: every output has the
 * bits of the unpaired call.
 * xchg: smx_epoch_pair_xchg_bytes(widest H1, widest H2) bytes (for every launch the device can pair), 16-byte aligned,
 * ZERO when allocated and never written by anyone else; it may be reused by every later launch (on one stream) of any
 * shape that fits -- the counts only grow, nothing is ever cleared.
 * The doubled grid must be resident at once: when smx_epoch_pair_fits(row blocks of all jobs) is 0 (or xchg is too
 * small) the launch runs unpaired, as smx_epoch_forward_f32 / smx_epoch_fwdbwd_f32. */
int64_t smx_epoch_pair_xchg_bytes(int32_t H1, int32_t H2);
int32_t smx_epoch_pair_fits(int64_t blocks);
int smx_epoch_forward_pair_f32(const smx_epoch_job_t* jobs, int32_t njobs, const struct smx_ppo_losses* loss,
                               smx_ppo_ctrl_t* ctrl, int64_t n_total, void* xchg, int64_t xchg_bytes,
                               smx_stream_t stream);
int smx_epoch_fwdbwd_pair_f32(const smx_epoch_job_t* jobs, int32_t njobs, const struct smx_ppo_losses* loss,
                              smx_ppo_ctrl_t* ctrl, int64_t n_total, int32_t* sync_word, uint64_t* kl_slots,
                              void* xchg, int64_t xchg_bytes, smx_stream_t stream);
/* The learn's FINAL forward-only policy pass (one SMX_EPOCH_LOSS_POLICY job, loss->will_update == 0) with the launches
 * that used to follow it folded in; every word they wrote is written with the same bits.
 *   stats_ticket != NULL: the pass's statistics, as smx_epoch_backward_f32 forms them for will_update == 0
 *     (loss->stats / dlogvar / dlogvar_sumsq, the KL early-exit flag), by the last policy workgroup to finish -- found by
 *     a ticket (an atomic add and a branch, never a wait); the partial rows cross workgroups as device-scope stores and
 *     loads and are added in smx_epoch_backward_f32's order.  A job whose stop_flag is up writes nothing, as there.
 *   epilogue != NULL: what smx_ppo_learn_epilogue_f32 does, on extra workgroups behind the row blocks (they do not
 *     look at the stop flag); the last of them forms out4.  512 threads play the 1024 of that launch in two passes:
 *     every sum keeps its operands and its order.  The value finalize reads v_partials of EARLIER launches only.
 * Both tickets: one int32 each in device memory, zero before the first call, left zero.
 * xchg / xchg_bytes: pair mode as smx_epoch_forward_pair_f32 (NULL / 0: unpaired). */
struct smx_learn_epilogue;
int smx_epoch_forward_final_f32(const smx_epoch_job_t* jobs, int32_t njobs, const struct smx_ppo_losses* loss,
                                smx_ppo_ctrl_t* ctrl, int64_t n_total, void* xchg, int64_t xchg_bytes,
                                int32_t* stats_ticket, const struct smx_learn_epilogue* epilogue,
                                smx_stream_t stream);
/* A co-tenant for the launch above (diagnostics / tests; no reference counterpart): `blocks` workgroups, each holding
 * one compute unit to itself (more than half of its LDS) for `microseconds` (<= 2 s) without doing work.  The in-launch
 * wait of smx_epoch_fwdbwd_f32 is bounded at 0.25 s: a tenant that keeps its workgroups off the device for longer makes
 * that learn fail loudly (ctrl->reserved[1]); a learner that may share the device uses the two-launch form
 * (session_config.learner.exclusive_device = False). */
int smx_device_occupy(int32_t blocks, int64_t microseconds, smx_stream_t stream);

/* --- acting head (PPOAgent.act, ppo_agent.py:106-154; DiagGauss.sample/maxprob, ppo_net.py:74-91) ---
 * pd[r] = [mean[r, :], exp(log_var) * noise_scale[r]]   (builders.py:127; ppo_agent.py:139:
 *         action_pd[:, A:] *= exp(noise), noise_scale == NULL: 1)
 * actions[r] = clip(eps[r] * std + mean, -1, 1)         (ppo_net.py:80-82, ppo_agent.py:147),
 *              eps == NULL: clip(mean) -- the deterministic evaluation modes.
 * eps is the caller's standard-normal draw (one row per actor); every ld is a row stride in
 * floats, so pd / actions can be slots of a rollout buffer.  pd may be NULL. */
int smx_diaggauss_sample_f32(const float* mean, int64_t ld_mean, const float* log_var,
                             const float* noise_scale, const float* eps, int64_t ld_eps,
                             int64_t rows, int32_t A, float* actions, int64_t ld_act, float* pd,
                             int64_t ld_pd, smx_stream_t stream);
/* The means PPOLearner._optimize reports once per learn, formed on the device so that the whole
 * statistics block needs one read-back: out4 = {mean(log_var) (ppo.py:572), mean_d(running_sum/
 * count), mean_d(running_sumsq/count), mean_d(sqrt(running_sumsq/count - (running_sum/count)^2))}
 * (ppo.py:580-583, z_filter.py:81-107; running_sum == NULL: only out4[0]). */
int smx_ppo_final_stats_f32(const float* log_var, int32_t A, const float* running_sum,
                            const float* running_sumsq, const float* count, int32_t D, float* out4,
                            smx_stream_t stream);
/* stats[e, SMX_VS_*] for e < count from partials [count, nblk, 8] (one launch per learn) */
int smx_value_loss_finalize_f32(const float* partials, int32_t count, int32_t nblk,
                                float* stats, int32_t stats_stride, smx_stream_t stream);

/* --- clip_grad_norm_ + Adam (ppo.py:243-247,304-308,348-352; torch.optim.Adam) ----
 * theta/grads/exp_avg/exp_avg_sq flat [n]; sumsq_partials [npart]: sums of squares of
 * disjoint pieces of `grads` (per-tile values from smx_mlp3_backward_f32 followed by any
 * extra entries the caller appended, e.g. log_var's; or smx_sumsq_partials_f32 of the
 * all-reduced gradient).  which = 0 actor / 1 critic selects lr, max_norm, weight decay and
 * the (already advanced) step counter in ctrl.  Writes the pre-clip total norm to
 * *grad_norm_out.  No-op when ctrl->stop_flag is set and honour_stop != 0. */
int smx_clip_adam_step_f32(float* theta, const float* grads, float* exp_avg,
                           float* exp_avg_sq, int64_t n, const float* sumsq_partials,
                           int32_t npart, const smx_ppo_ctrl_t* ctrl, int32_t which,
                           int32_t honour_stop, float* grad_norm_out, smx_stream_t stream);
/* The same step for the actor's group AND the critic's group in one launch (a lock-step epoch
 * updates both: ppo.py:541-562 touches disjoint optimisers).  `which` is implied: actor = 0,
 * critic = 1. */
typedef struct smx_adam_group {
    float* theta;
    const float* grads;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    const float* sumsq_partials;
    int32_t npart;
    int32_t honour_stop;
    float* grad_norm_out;
    /* optional (both or neither): the group's MLP and its packed copy (smx_epoch_pack_f32 layout); the
     * step then writes every updated weight into the packed copy as well, so the next fused epoch
     * forward needs no separate packing launch */
    const smx_mlp3_t* pack_net;
    float* packed;
} smx_adam_group_t;
/* one group (which: 0 = actor's scalars of the control block, 1 = critic's), with the optional packed copy */
int smx_clip_adam_step_group_f32(const smx_adam_group_t* group, int32_t which, const smx_ppo_ctrl_t* ctrl,
                                 smx_stream_t stream);
int smx_clip_adam_step_pair_f32(const smx_adam_group_t* actor, const smx_adam_group_t* critic,
                                const smx_ppo_ctrl_t* ctrl, smx_stream_t stream);
/* partials[b] = sum of squares of block b's slice of x; returns via *nblk_out the count
 * used (<= max_blocks). */
int32_t smx_sumsq_blocks(int64_t n);
int smx_sumsq_partials_f32(const float* x, int64_t n, float* partials, smx_stream_t stream);

/* --- replay buffers (surreal/replay/fifo_replay.py:27-48, uniform_replay.py:36-47) ---
 * Storage is struct-of-arrays in HBM: one [capacity, width] fp32 table per field.
 * ring insert: table[(cursor + i) % capacity, :] = src[i, :] for i < n */
int smx_ring_insert_f32(float* table, int64_t capacity, int32_t width, int64_t cursor,
                        const float* src, int64_t n, smx_stream_t stream);
/* gather: dst[i, :] = table[idx[i], :]  (uniform sample with injected / generated idx,
 * FIFO pop with idx = (head + i) % capacity) */
int smx_gather_rows_f32(const float* table, int64_t capacity, int32_t width,
                        const int64_t* idx, int64_t n, float* dst, smx_stream_t stream);
/* with-replacement uniform indices in [0, len) from a Philox4x32-10 stream
 * (random.randint(0, len-1) per draw in the reference, uniform_replay.py:44-45) */
int smx_uniform_indices(int64_t* idx, int64_t n, int64_t len, uint64_t seed,
                        uint64_t offset, smx_stream_t stream);
/* The generator behind it by itself -- Philox4x32-10 (Salmon et al., SC'11) on arbitrary counters and keys:
 * ctr_key [n, 6] = {ctr0..3, key0, key1} -> out [n, 4].  The sampler's row i uses ctr = (lo32(offset + i),
 * hi32(offset + i), 0, 0), key = (lo32(seed), hi32(seed)) and idx = mulhi64((out0 << 32) | out1, len).  Exists so that
 * the device code can be checked against Random123's published known-answer vectors (tests/philox_ref.py). */
int smx_philox4x32_10(const uint32_t* ctr_key, int64_t n, uint32_t* out, smx_stream_t stream);
/* UniformReplay.sample (surreal/replay/uniform_replay.py:36-47) over a device-resident replay in ONE launch: the rows
 * idx[i] (or, idx == NULL, the rows smx_uniform_indices(len, seed, offset) would draw -- the same Philox counters) of up
 * to 8 field tables [capacity, row_bytes] -> dst [rows, row_bytes] each.  idx_out (nullable) receives the indices. */
typedef struct {
    const void* table;
    void* dst;
    int64_t row_bytes;
} smx_gather_job_t;
int smx_uniform_gather_multi(const smx_gather_job_t* jobs, int32_t njobs, int64_t capacity, int64_t rows,
                             const int64_t* idx, int64_t len, uint64_t seed, uint64_t offset, int64_t* idx_out,
                             smx_stream_t stream);

/* The same two copies for fields of any element width: a row is `row_bytes` opaque bytes (uint8 camera frames --
 * `pixel_input`, surreal/env/wrapper.py observation specs -- stay uint8 in HBM: a quarter of the table and copy
 * bytes of an fp32 widening).  Moves 16-byte lanes when pitch and addresses allow, else dwords, else bytes. */
int smx_ring_insert_bytes(void* table, int64_t capacity, int64_t row_bytes, int64_t cursor,
                          const void* src, int64_t n, smx_stream_t stream);
int smx_gather_rows_bytes(const void* table, int64_t capacity, int64_t row_bytes, const int64_t* idx,
                          int64_t n, void* dst, smx_stream_t stream);

/* --- sub-trajectory windowing (surreal/env/exp_sender_wrapper.py:209-264) -------
 * From per-actor rollouts laid out [actors, T, width] emit W moving windows of n_step rows:
 *   dst[(a*W + w), j, :] = src[a, start + w*stride + j, :]     0 <= j < n_step
 * The reference emits floor((T - n_step)/stride) + 1 windows per episode of T steps
 * (start = 0); obs_next of window w is the same call with start = n_step, n_step = 1 on a
 * rollout that holds T+1 observations. */
int smx_window_emit_f32(const float* src, int32_t actors, int32_t T, int32_t width,
                        int32_t start, int32_t n_step, int32_t stride, int32_t W, float* dst,
                        smx_stream_t stream);
/* byte-width variant (uint8 frames): rows of `row_bytes` bytes, same index arithmetic */
int smx_window_emit_bytes(const void* src, int32_t actors, int32_t T, int64_t row_bytes, int32_t start,
                          int32_t n_step, int32_t stride, int32_t W, void* dst, smx_stream_t stream);

/* --- "obs stacking" (FrameStackWrapper, surreal/env/wrapper.py:407-472) over a device-resident rollout -----------
 * frames [actors, R, frame_bytes] holds ONE raw camera frame per step (row 0: the frame after reset).  The stacked
 * observation of row s is the last n_stack frames on the channel axis, oldest first; a reset fills the history with
 * the first frame:   stacked(a, s)[i] = frames[a, max(s - (n_stack - 1) + i, first(a, s))],   0 <= i < n_stack,
 * first(a, s) = episode_first ? episode_first[a*R + s] : 0 (the row at which the episode that row s belongs to began).
 * Emitted as W moving windows of n_step rows (smx_window_emit_bytes' arithmetic) in the same gather:
 *   dst[(a*W + w), j, i, :] = stacked(a, start + w*stride + j)[i]      dst: [actors*W, n_step, n_stack, frame_bytes]
 * (W = 1, n_step = 1, start = t: what every actor's policy sees at step t.)  The raw frames are stored once; the
 * n_stack-fold copy of every frame that stacking on the host keeps per step is never made. */
int smx_frame_stack_u8(const void* frames, int32_t actors, int32_t R, int64_t frame_bytes, int32_t n_stack,
                       const int32_t* episode_first, int32_t start, int32_t n_step, int32_t stride, int32_t W,
                       void* dst, smx_stream_t stream);
/* the synthetic environment's camera (no reference counterpart: the reference renders MuJoCo): for every actor a,
 * dst[a*ld_dst + (c, y, x)] = (37 c + 5 y + 11 x + 3 t + (int)(100 |s0[a*ld_s0]|)) % 256, uint8 [C, H, W]. */
int smx_synth_frame_u8(const float* s0, int64_t ld_s0, int32_t n, int32_t C, int32_t H, int32_t W, int32_t t,
                       void* dst, int64_t ld_dst, smx_stream_t stream);

/* --- synthetic vectorised environment step ("batched vectorised env stepping") --------
 * There is no reference counterpart (the reference steps MuJoCo simulators one process per
 * agent, surreal/agent/base.py:244-271); this is the synthetic stand-in BASELINE.json names,
 * stepped for all actors of a GPU in one launch and recorded straight into the device rollout:
 *   obs_roll[a, slot, :] = state[a, :]; obs_roll[a, slot+1, :] = state'[a, :] (if slot+1 < T);
 *   act_roll[a, slot, :] = clip(actions[a, :], -1, 1)   (every roll has T rows per actor)
 *   state'[a, k] = clamp(0.9*state[a,k] + 0.5*act[a, k % A] + 0.01*((37*k) % 17 - 8), -10, 10)
 *   rew_roll[a, slot] = -0.1 * sum_j act[a,j]^2 + 0.05 * state'[a, 0]
 *   done_roll[a, slot] = (t + 1 >= episode_len); on done the state resets to
 *   init_state[a, :] (a fresh episode), mirroring Agent.main_loop's reset.
 * Rolls may be NULL (pure stepping). */

/* The episode monitor of the device actors (surreal/env/monitor.py:11-75 EpisodeMonitor, which wraps one host env):
 * what every launch that evaluates the synthetic reward keeps per actor a when ep_reward != NULL, from call to call:
 *   every step:  ep_reward[a] += (double)reward (the fp32 reward of the step, added in step order); ep_steps[a] += 1
 *   on done:     e = ep_count[a]; done_reward[a, e % capacity] = ep_reward[a]; done_steps[a, e % capacity] = ep_steps[a];
 *                ep_count[a] = e + 1; ep_reward[a] = 0; ep_steps[a] = 0
 * so ep_reward / ep_steps [n] are the open episode, ep_count [n] the episodes finished since the monitor was attached,
 * done_reward / done_steps [n, capacity] a ring of the last `capacity` finished episodes per actor.  One lane owns an
 * actor's words (the lane that forms its reward), no atomics: a sum depends on the order of its steps only.  The
 * persistent kernels hold the open pair in LDS over their steps (HBM at entry, at a closing step and at exit).
 * ep_reward == NULL: no monitor -- the launch does exactly what it does without one (all five pointers or none, and
 * capacity > 0, else SMX_E_NULL / SMX_E_SHAPE). */
struct smx_episode_monitor {               /* (by tag: no typedef) */
    double* ep_reward;
    int32_t* ep_steps;
    int64_t* ep_count;
    double* done_reward;
    int32_t* done_steps;
    int32_t capacity, reserved;
};

/* The exploration noise of the device actors as a counter-based stream: the standard normal of (seed, global actor id
 * g, draw step s, action component j) is a pure function of the four, formed inside the launch that consumes it
 * (csrc/smx_philox.inc.h has the expressions):
 *   x[0..3] = Philox4x32-10(counter = (g, low32(s), high32(s), j >> 2), key = (low32(seed), high32(seed)))
 *   the pair p = (j & 3) >> 1 of words: u0 = ((x[2p] >> 8) + 0.5) 2^-24, u1 = ((x[2p + 1] >> 8) + 0.5) 2^-24 (never 0 or 1)
 *   r = sqrtf(-2 logf(u0)), angle = 2 pi u1 (sincospif(2 u1)); normal = r cos(angle) for even j, r sin(angle) for odd j
 * so one Philox block gives components 4q .. 4q + 3 by two Box-Muller pairs; |normal| <= sqrt(-2 ln 2^-25) ~ 5.887.
 * THE RULE of every launch that takes `eps` and a stream `noise`:
 *   eps != NULL:                   eps is used exactly as without a stream;
 *   eps == NULL, noise.enabled:    the draw of local actor a, the call's k-th step (0 in a one-step launch) and
 *                                  component j is normal(seed, actor_base + a, step + k, j);
 *   eps == NULL, !noise.enabled:   the launch is deterministic (the zero struct: what it did before there were streams);
 *   smx_ddpg_rollout.noise_type == SMX_DDPG_NOISE_NONE reads neither.
 * An actor's draws depend on its global id and the draw step only: not on n, on the steps of a call, on how a run is cut
 * into calls or on how the actors are split over launches (actor_base: the global id of the launch's actor 0).  With
 * enabled set, actor_base < 0 or actor_base + n > 2^32: SMX_E_SHAPE.  The four argument blocks that carry a stream hold it
 * by value right in front of `mon`, which stays their last member. */
struct smx_noise_stream {                  /* (by tag: no typedef) */
    uint64_t seed;
    int64_t actor_base;                    /* global id of local actor 0 */
    int64_t step;                          /* draw step of the call's first step */
    int32_t enabled, reserved;
};
/* out [steps, n, A] <- the draws a launch on `noise` over n actors forms for its `steps` steps (the same inline function;
 * noise->enabled is not read).  For the paths that sample outside these launches, and for tests. */
int smx_noise_fill_f32(const struct smx_noise_stream* noise, int32_t steps, int32_t n, int32_t A, float* out,
                       smx_stream_t stream);

/* mon: NULL, or the episode monitor above */
int smx_synth_env_step_f32(float* state, const float* init_state, const float* actions,
                           int32_t n, int32_t D, int32_t A, int32_t t, int32_t episode_len,
                           int32_t slot, int32_t T, float* obs_roll, float* act_roll,
                           float* rew_roll, float* done_roll, const struct smx_episode_monitor* mon,
                           smx_stream_t stream);

/* One launch between two policy forwards of a device-resident rollout: the acting head
 * (smx_diaggauss_sample_f32 on `mean`), the environment step above with the sampled action, and the
 * z-filter of the NEXT observation (smx_zfilter_forward_sums_f32) into xn_out -- what the next
 * policy forward reads.  pd_roll [n, T, 2A] receives the action_infos distribution; eps == NULL:
 * deterministic, or the draws of `noise` (the rule at struct smx_noise_stream); zsum == NULL: xn_out = the raw next observation; rolls may be NULL. */
typedef struct smx_synth_act_step {
    float* state;
    const float* init_state;
    const float* mean;
    const float* log_var;
    const float* noise_scale;
    const float* eps;
    int64_t ld_mean, ld_eps;
    int32_t n, D, A, t, episode_len, slot, T, reserved;
    float* obs_roll;
    float* act_roll;
    float* rew_roll;
    float* done_roll;
    float* pd_roll;
    const float* zsum;
    const float* zsumsq;
    const float* zcount;
    float zeps, reserved_f;
    float* xn_out;
    struct smx_noise_stream noise;         /* eps NULL and noise.enabled: the draws are formed in the launch */
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
} smx_synth_act_step_t;
int smx_synth_act_env_step_f32(const smx_synth_act_step_t* args, smx_stream_t stream);
/* The same launch with the policy's output layer folded in (PPOAgent.act's last Linear + Tanh, surreal/model/
 * model_builders/builders.py:126-135): mean = act(h2 . W3^T + b3) is formed per actor inside (A <= 32; args->mean is
 * ignored), so an acting step of a device-resident rollout is three dependent launches instead of four. */
int smx_synth_act_env_step_head_f32(const smx_synth_act_step_t* args, const float* W3, const float* b3,
                                    const float* h2, int64_t ld_h2, int32_t H2, int32_t out_act,
                                    smx_stream_t stream);


/* --- DDPG update pieces (surreal/learner/ddpg.py:244-352, 403-428) --------------------
 * Dense layers reuse smx_linear_f32 / smx_mlp3_*; the critic's "concat action into layer 2"
 * (builders.py:58-84) is expressed with row strides: layer 1 writes into the first c1 columns
 * of a [rows, c1+A] buffer whose last A columns hold the action.
 *   y = rewards + gamma^n * Q'(s', mu'(s')) * (1 - done)   (ddpg.py:279)
 *   dz3 = 2 (Q - y) / rows = d MSELoss / dQ                (ddpg.py:307-308) */
int smx_ddpg_critic_loss_f32(const float* q, const float* q_next_target, const float* rewards,
                             const float* dones, float gamma_n, int64_t rows, float* y,
                             float* dz3, smx_stream_t stream);
/* out = da * (1 - a^2): backward of the actor's final Tanh (builders.py:50) */
int smx_tanh_backward_f32(const float* da, const float* a, int64_t n, float* out,
                          smx_stream_t stream);
int smx_fill_f32(float* x, int64_t n, float value, smx_stream_t stream);
/* LayerNorm over the last dimension, forward and backward (DDPG use_layernorm = True: L.LayerNorm(1) behind every hidden
 * ReLU of ActorNetworkX / CriticNetworkX, model_builders/builders.py:42-48, 65-75; taken as torch.nn.LayerNorm(F):
 * biased variance, eps inside the root, elementwise affine -- torchx's source is not in the reference tree).
 *   forward : y[r, :] = (x[r, :] - mean_r) * rstd_r * gamma + beta; mean / rstd [rows] saved for the backward (may be NULL)
 *   backward: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; relu_mask != 0: dx *= (x > 0) (x is the output
 *             of the ReLU in front of the LayerNorm: dx is then the gradient at that ReLU's input);
 *             dgamma[j] = sum_r dy xhat, dbeta[j] = sum_r dy (overwritten; summed in a fixed order through ws,
 *             smx_layernorm_backward_ws_floats(rows, F) floats).  F <= 1024. */
int smx_layernorm_forward_f32(const float* x, int64_t ldx, int64_t rows, int32_t F, const float* gamma, const float* beta,
                              float eps, float* y, int64_t ldy, float* mean, float* rstd, smx_stream_t stream);
int64_t smx_layernorm_backward_ws_floats(int64_t rows, int32_t F);
int smx_layernorm_backward_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                               const float* rstd, const float* gamma, int64_t rows, int32_t F, int32_t relu_mask, float* dx,
                               int64_t lddx, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, smx_stream_t stream);
/* torch.optim.Adam step with optional clip_grad_value_ (Module.clip_grad_value, ddpg.py:309,332);
 * step = 1-based Adam step count; clip_value <= 0 disables clipping. */
int smx_adam_step_f32(float* theta, const float* grads, float* exp_avg, float* exp_avg_sq,
                      int64_t n, double lr, int32_t step, double weight_decay,
                      double clip_value, smx_stream_t stream);
/* The pieces that let ONE captured hipGraph be replayed for every DDPG iteration: the Adam step
 * count and the learning rates live in device memory.
 *   smx_ddpg_critic_loss_step_f32  = smx_ddpg_critic_loss_f32 + (*step_counter += 1): the
 *                                    iteration's step count, read by both Adam launches after it
 *   smx_adam_step_dev_f32          = smx_adam_step_f32 with lr / step read from the device
 *   smx_hard_update_every_f32      target <- source when *step % interval == 0 (the hard target
 *                                    update of ddpg.py:403-409, decided on the device) */
int smx_ddpg_critic_loss_step_f32(const float* q, const float* q_next_target, const float* rewards,
                                  const float* dones, float gamma_n, int64_t rows, float* y,
                                  float* dz3, int32_t* step_counter, smx_stream_t stream);
int smx_adam_step_dev_f32(float* theta, const float* grads, float* exp_avg, float* exp_avg_sq,
                          int64_t n, const float* lr, const int32_t* step, double weight_decay,
                          double clip_value, smx_stream_t stream);
int smx_hard_update_every_f32(float* target, const float* source, int64_t n, const int32_t* step,
                              int32_t interval, smx_stream_t stream);
/* target = target*(1-tau) + source*tau ; tau >= 1 is hard_update (ddpg.py:410-428) */
int smx_soft_update_f32(float* target, const float* source, float tau, int64_t n,
                        smx_stream_t stream);
/* stats[7] = {actor_loss = -mean q_actor, critic_loss = mean (q-y)^2, action_norm = mean
 * ||a||_2, mean rewards, Q_target = mean y, Q_policy = mean q   (ddpg.py:335-342),
 * max |a| (NaN if any action is NaN) for the |actions| <= 1 check of ddpg.py:262-263} */
int smx_ddpg_stats_f32(const float* q, const float* y, const float* rewards,
                       const float* actions, int32_t ld_act, int32_t A, const float* q_actor,
                       int64_t rows, float* stats, smx_stream_t stream);

/* --- one DDPG iteration on ROW BLOCKS (round 5; surreal/learner/ddpg.py:244-352, low-dimensional observations, one critic or TD3's two) ---
 * The layer-by-layer schedule above is ~19 dependent launches of 512-row problems.  Batch rows are independent up to the
 * weight gradients, so a workgroup carries FOUR rows through whole chains (round 6: the v_mfma_f32_4x4x1 loop of the
 * rollout kernel, the chain as a table of layer steps in the kernel arguments; the learner uses it up to 1024 rows per rank):
 *   smx_ddpg_rows_critic_f32  mu'(s') -> Q'(s', mu'(s')) (target networks); Q(s, a); y = r + gamma^n Q' (1 - done) and
 *                             dz3 = 2 (Q - y) / rows (ddpg.py:279, 307-308); *step += 1; the critic's data gradients
 *                             dz2 [rows, c2] and dz1 (first c1 columns of dxcat); mu(s) for the actor phase (h1a, h2a, act)
 *   smx_ddpg_rows_actor_f32   Q(s, mu(s)) through the critic as it is NOW (after its step, which keeps the
 *                             packed copy current) -> q_actor; d(-mean Q)/d(action) through tanh
 *                             -> dz3a; the actor's data gradients dz2a, dz1a (ddpg.py:326-331)
 * The weight gradients (sums over all rows) and the optimiser step are smx_ddpg_rows_wgrad_update_f32 (one rank) or the
 * launches declared above around smx_ddpg_rows_update_f32 (several), on the same row-major buffers.  Weights are read from a copy in MFMA fragment order (`packed`,
 * smx_ddpg_rows_packed_floats floats, 16-byte aligned) which smx_ddpg_rows_pack_f32 refreshes from the row-major
 * parameters: every network (SMX_DDPG_PACK_ALL) or the critic's blocks only.  xcat / dxcat have row stride c1 + A.
 * H1, H2, c1, c2 multiples of 4, A <= 32: smx_ddpg_rows_supported; otherwise SMX_E_UNSUPPORTED.
 *
 * TD3 (ddpg.py:119-147, 266-283, 312-319: use_double_critic, use_action_regularization) on the same rows: args->second
 * names the second critic, its target, a packed buffer of their own (smx_ddpg_rows_second_packed_floats floats: critic 2's
 * W1, W2, W3 and the first c1 rows of W2^T, target critic 2's W1, W2, W3; refreshed by SMX_DDPG_PACK_SECOND) and its
 * row-major buffers.  NULL: one critic, everything below as before.
 *   smx_ddpg_rows_critic_td3_f32  mu'(s'); Q1'(s', mu') and Q2'(s', clamp(mu' + noise, -1, 1)) (noise [rows, A] or NULL:
 *                             the second target alone sees it, fp32 add then clamp); y = min(y1, y2), each formed as
 *                             above (-> y; q_next = Q1', q_next2 = min(Q1', Q2')); *step += 1 once; per critic k:
 *                             Qk(s, a), dz3_k = 2 (Qk - y) / rows and its data gradients; mu(s) for the actor phase
 *   smx_ddpg_rows_actor_f32   unchanged: the actor goes through the first critic only (ddpg.py:325-328)
 *   SMX_DDPG_GROUP_CRITIC2    the second critic's step in smx_ddpg_rows_update_f32 / _wgrad_update_f32 (dxcat2 / dz2_2 /
 *                             dz3_2 against x / xcat2 / h2c2), its target and both copies inside packed2
 * With second->stats2 the statistics workgroup also forms a second block as smx_ddpg_stats_f32 would for (q2, y) (the
 * reference reports the second critic's loss and Q_policy2); update->stats_host is then [2][16]: slot (*step & 1), the
 * first block in words 0 .. 6, the second in words 8 .. 14.
 * smx_ddpg_rows_second_supported: the shapes' LDS budget with y kept between the two losses, and every row-major buffer
 * of `rows` rows within the 31-bit byte offsets the launches address them by.
 *
 * use_layernorm (model_builders/builders.py:42-48, 65-75: Linear -> ReLU -> LayerNorm on both hidden layers of actor and
 * critic; ddpg.py:244-352) on the same rows, one critic: args->ln names the four networks' gains and biases (read
 * row-major, no packed copy), eps and the extra row-major buffers.  NULL: no LayerNorm, everything as before.  With it
 *   smx_ddpg_rows_critic_f32 / _actor_f32  the same chains with a LayerNorm rule behind every hidden layer (the bits
 *                             of smx_layernorm_forward_f32 given the same row) and its backward rule (those of
 *                             smx_layernorm_backward_f32 with relu_mask) behind the backward products.  xcat[:, :c1], h2c,
 *                             h1a, h2a receive the LayerNorm OUTPUTS -- what the weight gradients multiply --, the
 *                             activations in front go to c_a1, c_a2, a1, a2 with each row's mean and rstd; dz2, dz2a, dz1a
 *                             are the gradients at the ReLUs' inputs as before, the critic's dz1 goes to dz1c [rows, c1] and
 *                             dxcat[:, :c1] keeps d/d(LayerNorm 1's output); dn2, dn2a, dn1a the other three.  The actor
 *                             chain goes back through the updated critic's second LayerNorm only.
 *   smx_ddpg_rows_wgrad_update_f32  also forms dgamma = sum_rows dn xhat and dbeta = sum_rows dn of the group's two
 *                             LayerNorms (further workgroups of the launch, a fixed summation order, no atomics) and steps
 *                             them: update->n covers the dense layers and, behind them, the four LayerNorm vectors.
 * smx_ddpg_rows_update_f32 returns SMX_E_UNSUPPORTED with ln set, and so does every entry given `second` together with
 * an `ln` whose own `second` is NULL; smx_ddpg_rows_pack_f32 packs the dense weights as before.
 * smx_ddpg_rows_ln_supported: what smx_ddpg_rows_supported_at says, narrowed by the LDS budget with the
 * pre-LayerNorm and dn tiles kept, and every row-major buffer within 31-bit byte offsets.
 *
 * use_layernorm together with TD3: args->second AND args->ln->second (the second critic's and its target's gains and
 * biases, its pre-LayerNorm activations c2_a1 / c2_a2 with mean and rstd, dn2_2, and dz1c2 -- dxcat2[:, :c1] keeps
 * d/d(LayerNorm 1's output), xcat2[:, :c1] and h2c2 receive the LayerNorm outputs).  Then
 *   smx_ddpg_rows_critic_td3_f32  runs TD3's chain with the LayerNorm rules behind every hidden layer and behind each
 *                             critic's loss and W2^T product (smx_ddpg_rows_critic_f32 still refuses ln with second)
 *   smx_ddpg_rows_actor_f32   the LayerNorm actor chain, unchanged: through the first critic only
 *   smx_ddpg_rows_wgrad_update_f32  SMX_DDPG_GROUP_CRITIC2 as SMX_DDPG_GROUP_CRITIC: the second critic's three weight
 *                             gradients, dgamma / dbeta of its two LayerNorms, Adam, its target, the copies in packed2
 * smx_ddpg_rows_ln_second_supported: smx_ddpg_rows_ln_supported narrowed by the LDS budget with y kept between the two
 * losses (and what smx_ddpg_rows_second_supported says). */
typedef struct smx_ddpg_net {          /* nn.Linear layouts: W [out, in] row-major */
    const float *W1, *b1, *W2, *b2, *W3, *b3;
} smx_ddpg_net_t;
struct smx_ddpg_rows_second {
    smx_ddpg_net_t critic2, target_critic2;
    float* packed2;
    const float* noise;                                        /* [rows, A] or NULL */
    float *xcat2, *h2c2, *q2, *q_next2, *dz3_2, *dz2_2, *dxcat2;   /* critic phase, out (xcat2 / dxcat2: row stride c1 + A) */
    float* stats2;                                             /* [7] or NULL */
};
struct smx_ddpg_ln_net {               /* the two LayerNorms of a network: gain and bias behind layer 1 [H1 | c1], layer 2 [H2 | c2] */
    const float *g1, *b1, *g2, *b2;
};
struct smx_ddpg_rows_ln_second {       /* use_layernorm with TD3's second critic: its LayerNorms and its own row-major buffers */
    struct smx_ddpg_ln_net critic2, target_critic2;
    float *c2_a1, *c2m1, *c2r1, *c2_a2, *c2m2, *c2r2;          /* critic phase, out: as c_a1 ... cr2 for the second critic */
    float *dn2_2, *dz1c2;                                      /* critic phase, out: [rows, c2], [rows, c1] */
};
struct smx_ddpg_rows_ln {
    struct smx_ddpg_ln_net actor, critic, target_actor, target_critic;
    float eps;
    float *c_a1, *cm1, *cr1, *c_a2, *cm2, *cr2;                /* critic phase, out: [rows, c1], [rows] x 2, [rows, c2], [rows] x 2 */
    float *dn2, *dz1c;                                         /* critic phase, out: [rows, c2], [rows, c1] */
    float *a1, *am1, *ar1, *a2, *am2, *ar2;                    /* critic phase out, actor phase in: [rows, H1], .., [rows, H2], .. */
    float *dn2a, *dn1a;                                        /* actor phase, out: [rows, H2], [rows, H1] */
    const struct smx_ddpg_rows_ln_second* second;              /* with args->second: the second critic's part; NULL: one critic */
};
typedef struct smx_ddpg_rows {
    int64_t rows;
    int32_t D, A, H1, H2, c1, c2;      /* actor D -> H1 -> H2 -> A (tanh); critic D -> c1, [c1 | A] -> c2 -> 1 */
    smx_ddpg_net_t actor, critic, target_actor, target_critic;
    float* packed;
    const float *x, *x_next, *actions, *rewards, *dones;       /* [rows, D] x 2, [rows, A], [rows] x 2 */
    float gamma_n;
    float *xcat, *h2c, *q, *q_next, *y, *dz3, *dz2, *dxcat;    /* critic phase, out */
    float *h1a, *h2a, *act;                                    /* critic phase out, actor phase in */
    float *q_actor, *dz3a, *dz2a, *dz1a;                       /* actor phase, out */
    int32_t* step;                                             /* device Adam step counter (may be NULL) */
    const struct smx_ddpg_rows_second* second;                 /* TD3's second critic; NULL: one critic */
    const struct smx_ddpg_rows_ln* ln;                         /* use_layernorm; NULL: none */
} smx_ddpg_rows_t;
enum { SMX_DDPG_PACK_ALL = 0, SMX_DDPG_PACK_CRITIC = 1, SMX_DDPG_PACK_SECOND = 2 };   /* ALL / CRITIC: args->packed only */
int32_t smx_ddpg_rows_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2);   /* on 4-row blocks */
/* ... for a batch of `rows` (the same answer for every row count since the 16-row kernels of round 5 are gone) */
int32_t smx_ddpg_rows_supported_at(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2, int64_t rows);
int64_t smx_ddpg_rows_packed_floats(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2);
int smx_ddpg_rows_pack_f32(const smx_ddpg_rows_t* args, int32_t which, smx_stream_t stream);
int smx_ddpg_rows_critic_f32(const smx_ddpg_rows_t* args, smx_stream_t stream);
int smx_ddpg_rows_actor_f32(const smx_ddpg_rows_t* args, smx_stream_t stream);
int32_t smx_ddpg_rows_second_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2, int64_t rows);
int64_t smx_ddpg_rows_second_packed_floats(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2);
int smx_ddpg_rows_critic_td3_f32(const smx_ddpg_rows_t* args, smx_stream_t stream);
int32_t smx_ddpg_rows_ln_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2, int64_t rows);
int32_t smx_ddpg_rows_ln_second_supported(int32_t D, int32_t A, int32_t H1, int32_t H2, int32_t c1, int32_t c2, int64_t rows);
/* Delayed policy updates (TD3's third ingredient; the reference's iteration, ddpg.py:244-352, is the case d = 1): the
 * actor and every target move once per d critic updates.  An iteration that updates the critics alone runs
 *   smx_ddpg_rows_critic_only_f32 / smx_ddpg_rows_critic_only_td3_f32  the chains of smx_ddpg_rows_critic_f32 /
 *                             _critic_td3_f32 WITHOUT the actor's forward pass, on the same kernels (the chain is a step
 *                             table): target networks, y, *step += 1, each critic's loss and data gradients -- with args->ln
 *                             the LayerNorm forms.  h1a, h2a, act (ln: a1 ... ar2) are neither required nor written.
 * followed by the critic groups' smx_ddpg_rows_wgrad_update_f32 with target == NULL, the last of them carrying the
 * statistics (q_actor as the last actor chain left it).  An iteration that updates the actor too runs today's launches, the
 * actor's update with a step word of its own, and between the actor chain and that update
 *   smx_ddpg_rows_delay_tail_f32  one workgroup: with stats, the statistics exactly as smx_ddpg_rows_wgrad_update_f32's
 *                             extra workgroup forms them (args' q, y, rewards, actions, q_actor; second->stats2; stats_host
 *                             slot *args->step & 1 -- the ITERATION's word, not the actor's); then *actor_step += 1.
 *                             stats == NULL (args may be NULL then): the increment alone. */
int smx_ddpg_rows_critic_only_f32(const smx_ddpg_rows_t* args, smx_stream_t stream);
int smx_ddpg_rows_critic_only_td3_f32(const smx_ddpg_rows_t* args, smx_stream_t stream);
int smx_ddpg_rows_delay_tail_f32(const smx_ddpg_rows_t* args, int32_t* actor_step, float* stats, float* stats_host,
                                 smx_stream_t stream);

/* One optimiser group's step of the row schedule in ONE launch (round 6): Adam exactly as smx_adam_step_dev_f32
 * (torch.optim.Adam after clip_grad_value_: ddpg.py:310-311, 332-333), then the group's target network -- soft
 * (interval == 0: target = target (1 - tau) + theta tau) or hard every `interval` iterations of *step (ddpg.py:389-428),
 * target == NULL: none -- and the fragment-order copies of both inside args->packed, element by element: no
 * smx_ddpg_rows_pack_f32 is needed between iterations as long as nothing else writes the parameters.  theta / target are
 * the group's parameter buffers ([n], holding the W1, W2, W3 that args names for the group at the same offsets). */
typedef struct smx_ddpg_update {
    float* theta;
    const float* grads;
    float *exp_avg, *exp_avg_sq;
    float* target;
    int64_t n;
    const float* lr;                   /* device */
    const int32_t* step;               /* device: Adam's step count of this iteration (also decides a hard update) */
    float weight_decay, clip_value, tau;
    int32_t interval;
    float* stats;                      /* smx_ddpg_rows_wgrad_update_f32 only, may be NULL: [7] as smx_ddpg_stats_f32 writes them,
                                          from args' q, y, rewards, actions, q_actor -- one more workgroup of the launch */
    float* stats_host;                 /* with stats, may be NULL: device-accessible HOST memory [2][8]; the same seven words also
                                          go to slot (*step & 1) -- the caller reads them after the launch without a copy */
} smx_ddpg_update_t;
enum { SMX_DDPG_GROUP_ACTOR = 0, SMX_DDPG_GROUP_CRITIC = 1, SMX_DDPG_GROUP_CRITIC2 = 2 };
int smx_ddpg_rows_update_f32(const smx_ddpg_rows_t* args, int32_t group, const smx_ddpg_update_t* update,
                             smx_stream_t stream);
/* The same step with the group's weight gradients formed in the SAME launch (one rank: nothing to exchange between them):
 * dW = dz^T x and db = the column sums of dz over args->rows rows, from the buffers the chain launches wrote (critic:
 * dxcat / dz2 / dz3 against x / xcat / h2c; actor: dz1a / dz2a / dz3a against x / h1a / h2a), written to update->grads
 * (laid out like theta) and stepped while still in the accumulators.  update->n must be exactly the three layers'
 * weights and biases. */
int smx_ddpg_rows_wgrad_update_f32(const smx_ddpg_rows_t* args, int32_t group, const smx_ddpg_update_t* update,
                                   smx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM stem (surreal/model/ppo_net.py:143-152: nn.LSTM(in, rnn_hidden, 1, batch_first=True) in
 * front of the actor / critic MLPs; forward at :277-279, :307-309, single step at :338-349).
 * torch.nn.LSTM layouts: W_ih [4H, D], W_hh [4H, H], b_ih [4H], b_hh [4H], gate order i, f, g, o.
 * H must be a multiple of 4 and <= 384; B*T*4H < 2^31.
 * Alignment: W_hh must be 16-byte aligned (the kernels read its rows four floats at a time; with H % 4 == 0 every row
 * then is) -- inside a flat [W_ih | W_hh | b_ih | b_hh] vector that is a 16-byte aligned W_ih, since 4 H D is a multiple
 * of 4 floats.  smx_lstm_forward_f32 refuses anything else (SMX_E_UNSUPPORTED).  W_ih, b_ih, b_hh, x, h0, c0 and every
 * output need only float alignment.
 * ------------------------------------------------------------------------------------------- */
typedef struct smx_lstm {
    const float* W_ih;
    const float* W_hh;
    const float* b_ih;
    const float* b_hh;
    int32_t D, H;
} smx_lstm_t;

/* number of parameters, laid out [W_ih | W_hh | b_ih | b_hh] (also the layout of `grads` below) */
int64_t smx_lstm_param_count(int32_t D, int32_t H);

/* out[b, t, :] = h_t for x [B, T, D] starting from (h0, c0) [B, H] (NULL = zeros).  Saved for
 * the backward pass: gates [B, T, 4H] (activated i, f, g, o), cs [B, T, H] (c_t), hprev
 * [B, T, H] (h_{t-1}, may be NULL for inference).  hN / cN [B, H] (optional) receive the final
 * state (forward_actor_expose_cells).  A non-zero *stop_flag skips the whole call. */
int smx_lstm_forward_f32(const smx_lstm_t* net, const float* x, int64_t B, int32_t T,
                         const float* h0, const float* c0, float* gates, float* out, float* cs,
                         float* hprev, float* hN, float* cN, const int32_t* stop_flag,
                         smx_stream_t stream);

/* Back-propagation through time given dout [B, T, H] = dLoss/dh_t from the layers above
 * (h0, c0 are constants: ppo.py:511-515 detaches them).  dgates [B, T, 4H] is workspace (it may
 * alias `gates`).  grads receives dW_ih, dW_hh, db_ih, db_hh (overwritten, not accumulated).
 * ws / ws_floats: optional split-K workspace for the two weight-gradient GEMMs over B*T rows
 * (smx_lstm_backward_ws_floats; NULL = unsplit).  A non-zero *stop_flag skips the whole call, the weight-gradient
 * launches included: dgates, grads and ws are left as they are (like smx_lstm_forward_f32 and every other call that
 * takes the flag). */
int64_t smx_lstm_backward_ws_floats(int32_t D, int32_t H, int64_t B, int32_t T);
int smx_lstm_backward_f32(const smx_lstm_t* net, const float* x, int64_t B, int32_t T,
                          const float* c0, const float* gates, const float* cs,
                          const float* hprev, const float* dout, float* dgates, float* grads,
                          const int32_t* stop_flag, float* ws, int64_t ws_floats,
                          smx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CNN stem data movement (surreal/model/model_builders/builders.py:8-33 CNNStemNetwork;
 * ppo_net.py:268-273, 368-375 `_scale_image`).  The convolutions themselves are smx_linear_f32 /
 * smx_linear_wgrad_f32 over patch rows.
 * ------------------------------------------------------------------------------------------- */
/* cols[(f*Ho + oy)*Wo + ox, c*kh*kw + i*kw + j] = src(f, c, oy*stride + i, ox*stride + j)
 * [/ scale_div when scale_div != 0: x / 255.0 of _scale_image].  src: uint8 or fp32 frames
 * [F, C, Hin, Win] (channel_last = 0), or an fp32 activation [F, Hin*Win, C] (channel_last = 1).
 * No padding (torch default); Ho = (Hin - kh)/stride + 1.  The k order is torch's
 * Conv2d.weight.view(out, -1) order. */
int smx_im2col_f32(const void* src, int32_t src_is_u8, int32_t channel_last, int64_t F, int32_t C,
                   int32_t Hin, int32_t Win, int32_t kh, int32_t kw, int32_t stride,
                   float scale_div, float* cols, smx_stream_t stream);
/* First convolution over uint8 frames as an implicit GEMM (no patch matrix): y[(f, oy, ox), o] = relu(b[o] +
 * sum_{c,i,j} W[o][c][i][j] * float(frames[f][c][oy*stride + i][ox*stride + j]) / 255) -- Conv2d + ReLU of
 * surreal/model/model_builders/builders.py:8-33 on `x / 255` (ppo_net.py:268-275), the same numbers as
 * smx_im2col_f32 (scale_div 255) + smx_linear_f32 (ReLU).  y is channel-last [F*Ho*Wo, cout].
 * SMX_E_UNSUPPORTED unless cout <= 16, k % 4 == 0, Win % 4 == 0, stride % 4 == 0, C*k*k in {64, 128, 192, 256}.
 * stop_flag (device, may be NULL): non-zero turns the launch into a no-op (the KL early exit). */
int smx_conv_u8_forward_f32(const void* frames, int64_t F, int32_t C, int32_t Hin, int32_t Win, int32_t k,
                            int32_t stride, const float* W, const float* bias, int32_t cout, float* y,
                            const int32_t* stop_flag, smx_stream_t stream);
/* The same layer's weight gradient, again from the uint8 frames (no patch matrix): dW[o][(c, i, j)] = sum over
 * (f, oy, ox) of dy[(f, oy, ox), o] * float(frames[f][c][oy*stride + i][ox*stride + j]) / 255, db[o] = the column
 * sums of dy -- what autograd gives Conv2d.weight / .bias (ppo.py:243-247 backward through builders.py:8-33); equal
 * to smx_im2col_f32 + smx_linear_wgrad_splitk_f32 up to summation order.  dy is [F*Ho*Wo, cout] row-major; ws holds
 * smx_conv_u8_wgrad_ws_floats(cout, C*k*k) floats (per-workgroup partials, added in a fixed order by a second launch).
 * Same shape limits as smx_conv_u8_forward_f32. */
int64_t smx_conv_u8_wgrad_ws_floats(int32_t cout, int32_t K);
int smx_conv_u8_wgrad_f32(const void* frames, int64_t F, int32_t C, int32_t Hin, int32_t Win, int32_t k,
                          int32_t stride, const float* dy, int32_t cout, float* dW, float* db, float* ws,
                          int64_t ws_floats, const int32_t* stop_flag, smx_stream_t stream);
/* A convolution over an fp32 CHANNEL-LAST source of 16 channels ([F, Hin*Win, 16]: the first convolution's output) as
 * implicit GEMMs, forward (+ bias + ReLU) and weight gradient -- the second Conv2d of builders.py:8-33 and what autograd
 * gives its weight / bias; W and dW in torch's [cout][16][k][k] order; y / dy are [F*Ho*Wo, cout].  Equal to
 * smx_im2col_f32 (channel_last = 1) + smx_linear_f32 / smx_linear_wgrad_splitk_f32 up to summation order.
 * SMX_E_UNSUPPORTED unless C == 16, cout <= 32, k in {2, 3, 4}.  ws: smx_conv_cl_wgrad_ws_floats(cout, k) floats. */
int smx_conv_cl_forward_f32(const float* src, int64_t F, int32_t C, int32_t Hin, int32_t Win, int32_t k,
                            int32_t stride, const float* W, const float* bias, int32_t cout, float* y,
                            const int32_t* stop_flag, smx_stream_t stream);
int64_t smx_conv_cl_wgrad_ws_floats(int32_t cout, int32_t k);
int smx_conv_cl_wgrad_f32(const float* src, int64_t F, int32_t C, int32_t Hin, int32_t Win, int32_t k,
                          int32_t stride, const float* dy, int32_t cout, float* dW, float* db, float* ws,
                          int64_t ws_floats, const int32_t* stop_flag, smx_stream_t stream);
/* ... and its data gradient, dx [F, Hin*Win, 16] (channel-last) = relu'(relu_of) * conv_transpose(dy, W), without the
 * intermediate dcols matrix: what smx_linear_f32 (dy . W) + smx_col2im_f32 give, up to summation order.
 * SMX_E_UNSUPPORTED unless C == 16, cout <= 32 and k == 2 * stride. */
int smx_conv_cl_dgrad_f32(const float* dy, int64_t F, int32_t C, int32_t Hin, int32_t Win, int32_t k,
                          int32_t stride, const float* W, int32_t cout, const float* relu_of, float* dx,
                          const int32_t* stop_flag, smx_stream_t stream);
/* data gradient of the convolution above: dx [F, Hin*Win, C] (channel-last) gathers dcols
 * [F*Ho*Wo, C*kh*kw]; relu_of (optional, same shape as dx): dx *= (relu_of > 0). */
int smx_col2im_f32(const float* dcols, int64_t F, int32_t C, int32_t Hin, int32_t Win, int32_t kh,
                   int32_t kw, int32_t stride, const float* relu_of, float* dx,
                   smx_stream_t stream);
/* Flatten order of the Linear after the convolutions: to_channel_last != 0:
 * out[o, p*C + c] = in[o, c*P + p], else the inverse (used for the weight and for its gradient). */
int smx_flatten_order_f32(const float* in, int32_t O, int32_t C, int32_t P,
                          int32_t to_channel_last, float* out, smx_stream_t stream);

/* A whole device-resident rollout in ONE launch: `steps` iterations of [z-filter -> policy MLP -> DiagGauss sample ->
 * clip -> synthetic env step -> record] for all n actors (the per-step loop of surreal/agent/base.py:244-271 with
 * PPOAgent.act, surreal/agent/ppo_agent.py:106-154, and the recording of env/exp_sender_wrapper.py:153-264).  A
 * workgroup owns actors_per_workgroup = 4, 8 or 16 actors for the whole rollout (0: 4, 8 from 1025 actors on, 16 beyond
 * 2048 on 256 CUs -- the smallest block whose grid fits the CUs once; anything else: SMX_E_SHAPE); the policy layers
 * run on FP32 MFMA (v_mfma_f32_4x4x1; 16x16x4 for 16-actor blocks) from `packed`
 * (smx_epoch_pack_f32 of `net`): the means equal smx_epoch_forward_f32's to fp32 rounding of the layer sums (another
 * summation order), 4- and 8-actor blocks bit for bit each other's; sampling, dynamics, recording and the z-filter use the
 * expressions of smx_synth_act_env_step_f32.
 * eps [steps, n, A] standard normals (NULL: deterministic, or the draws of `noise`); zsum/zsumsq/zcount: the z-filter's running sums (NULL:
 * raw observations); rolls [n, rows_per_actor, .] (any may be NULL); state [n, D] is read at the start and left at
 * the state after the last step; t: the episode clock at the first step.
 * obs_last [n, D] (nullable): where the observation AFTER row rows_per_actor - 1 goes.  With rows_per_actor = steps + 1
 * (a rollout table) that observation is the table's last row and obs_last is not used; with rows_per_actor = steps the
 * tables have exactly the replay's layout -- obs [n, n_step, D] + obs_next [n, 1, D] = obs_last -- and the rollout is
 * recorded STRAIGHT INTO the FIFO's slots when stride == n_step (env/exp_sender_wrapper.py:209-228: a window then is
 * the rollout; no window cut, no insert copy). */
typedef struct smx_synth_rollout {
    const smx_mlp3_t* net;
    const float* packed;
    int32_t out_act, n;
    const float* log_var;
    const float* noise_scale;
    const float* eps;
    const float* zsum;
    const float* zsumsq;
    const float* zcount;
    float zeps;
    int32_t t, episode_len, steps, rows_per_actor, slot;
    float* state;
    const float* init_state;
    float* obs_roll;
    float* act_roll;
    float* rew_roll;
    float* done_roll;
    float* pd_roll;
    float* obs_last;
    int32_t actors_per_workgroup;          /* 4 | 8 | 16, 0: the smallest whose grid fits the CUs once */
    struct smx_noise_stream noise;         /* eps NULL and noise.enabled: the draws are formed in the launch */
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
} smx_synth_rollout_t;
int32_t smx_synth_rollout_supported(int32_t D, int32_t H1, int32_t H2, int32_t A);
int smx_synth_rollout_f32(const smx_synth_rollout_t* args, smx_stream_t stream);

/* The same rollout for a PPO policy with a one-layer LSTM stem on low-dimensional observations (the reference's default
 * policy: surreal/main/ppo_configs.py if_rnn_policy, rnn_layer 1), in ONE launch: per step and actor (all actors share
 * the episode clock)
 *   x = zfilter(s)                                     (or raw, as above)
 *   g = W_ih x + b_ih + W_hh h + b_hh                   gate order i, f, g, o (ppo_net.py:143-152, 338-349)
 *   c' = sigmoid(f) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c')
 *   mu = act(MLP(h')), the DiagGauss sample and clip, the synthetic environment step and its recording as above
 * -- PPOAgent.act with the LSTM (surreal/agent/ppo_agent.py:106-154, ppo_net.py:317-354) for every actor and step.
 * The kernel replaces a per-step act_batch (z-filter, smx_lstm_forward_f32 at T = 1, the actor, the sampling head,
 * the step launch).  roll.net is the actor with roll.net->D == lstm->H; lstm_packed: smx_lstm_rollout_pack_f32 of lstm.
 * hidden: the logical units (lstm->H is padded to a multiple of 4 with zero weights; the padded units stay zero and are
 * never written): every state buffer below is [n, hidden].  h0 / c0 (nullable, both or neither: zeros) the state
 * before the first step; hN / cN the state after the last; h_before / c_before (nullable) the state before the last
 * step (what PPOAgent.batch_cells_before holds).  cell_roll [n, rows_per_actor, 2, hidden] (nullable): the state every
 * actor held BEFORE each step, h then c, at row slot + step -- ppo_agent.py:133-135 onetime_infos.  Gates use
 * smx_lstm_forward_f32's sigmoid and tanh; the gate sums run on the 4-row loop over K = [x | h] (another summation
 * order than smx_lstm_forward_f32: equal to fp32 rounding).  4, 8 and 16 actors per workgroup give the same bits. */
struct smx_synth_lstm_rollout {               /* (by tag: no typedef) */
    smx_synth_rollout_t roll;
    const smx_lstm_t* lstm;
    const float* lstm_packed;
    int32_t hidden, reserved;
    const float* h0;
    const float* c0;
    float* hN;
    float* cN;
    float* h_before;
    float* c_before;
    float* cell_roll;
};
/* shapes smx_synth_lstm_rollout_f32 takes: those of smx_synth_rollout_supported with the actor's input H, H a multiple
 * of 4 up to 128 */
int32_t smx_synth_lstm_rollout_supported(int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A);
/* floats of the gate pass's packed weights ([4H, D + H] in fragment order + the summed biases); 0 for bad shapes */
int64_t smx_lstm_rollout_packed_floats(int32_t D, int32_t H);
/* packed (16-byte aligned, smx_lstm_rollout_packed_floats) <- net; refresh it whenever the weights change */
int smx_lstm_rollout_pack_f32(const smx_lstm_t* net, float* packed, smx_stream_t stream);
int smx_synth_lstm_rollout_f32(const struct smx_synth_lstm_rollout* args, smx_stream_t stream);

/* The PPO rollouts above (base.lstm NULL: smx_synth_rollout_f32's plain-MLP policy from base.roll; else
 * smx_synth_lstm_rollout_f32's one-layer LSTM stem) with every step exactly as there, recorded as the moving windows of
 * ExpSenderWrapperMultiStepMovingWindowWithInfo (surreal/env/exp_sender_wrapper.py:153-264, restated in
 * surreal_amd/env/exp_sender_wrapper.py) straight into the FIFO replay's ring instead of rollout tables.  Per actor a
 * and episode step tau (all actors share the clock tau = base.roll.t at the first step, anywhere in an episode;
 * N = n_step, adv = advance = min(stride, n_step), window_advance):
 *   slot tau % N of the carry rings <- the state before the step (the raw observation), the action, the reward and
 *     the pd [mu | sd] (exp_sender_wrapper.py:200-208 fills a queue of n_step); an LSTM policy's state (h, c) before
 *     the step to slot (tau / adv) % S, S = ceil(N / adv), when tau % adv == 0 (onetime_infos, ppo_agent.py:133-135)
 *   window j = tau + 1 - N closes at step tau when j >= 0 and j % adv == 0 (exp_sender_wrapper.py:209-228: the queue
 *     is full, then `stride` entries are popped); at the k-th closing step of the call actor a's window goes to FIFO
 *     row (cursor + k n + a) % capacity: obs [N, D], actions [N, A], rewards [N], dones [N], pds [N, 2A] in episode
 *     order, obs_next [D] the observation after step tau (the terminal one before the reset, SyntheticEnv._step),
 *     cells [2, hidden] (h then c; the replay's [2, 1, hidden]) the state before step j
 *   windows never cross an episode: the clock restarts at 0 after the terminal step, so a partial window is dropped
 *     (the wrapper's _reset, exp_sender_wrapper.py:192-197); the carry rings hold the open windows from one call to
 *     the next (the caller clears them when it resets the environments), one call may span several episode ends
 *   the LSTM state goes from h0 / c0 (nullable: zeros) to hN / cN across windows and episodes: the reference resets it
 *     only in PPOAgent.__init__ (ppo_agent.py:168-181; Agent.main_loop, agent/base.py:244-271, never does);
 *     h_before / c_before as in smx_synth_lstm_rollout_f32
 * carry_obs [n, N, D], carry_act [n, N, A], carry_rew [n, N], carry_pd [n, N, 2A], carry_cells [n, S, 2, hidden]
 * (LSTM only); obs [capacity, N, D], obs_next [capacity, D], actions [capacity, N, A], rewards / dones [capacity, N],
 * pds [capacity, N, 2A], cells [capacity, 2, hidden] (LSTM only).  The caller makes n * (closing steps) <= capacity
 * (checked: SMX_E_SHAPE).  base.roll's rollout tables, slot and rows_per_actor and base.cell_roll are not used.
 * 4, 8 and 16 actors per workgroup (0: as there) all run the 4-row loop and give the same bits; the means equal those
 * of smx_synth_rollout_f32 / smx_synth_lstm_rollout_f32 at 4 actors per workgroup bit for bit. */
struct smx_synth_ppo_window_rollout {      /* (by tag: no typedef) */
    struct smx_synth_lstm_rollout base;     /* base.lstm NULL: a plain-MLP policy (the stem's fields unused) */
    int32_t n_step, advance;
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* carry_pd;
    float* carry_cells;
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    float* pds;
    float* cells;
    int64_t cursor, capacity;
};
/* shapes smx_synth_ppo_window_rollout_f32 takes: H == 0 a plain-MLP policy (those of smx_synth_rollout_supported, with
 * 16-actor blocks on the 4-row loop), else those of smx_synth_lstm_rollout_supported */
int32_t smx_synth_ppo_window_rollout_supported(int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A);
int smx_synth_ppo_window_rollout_f32(const struct smx_synth_ppo_window_rollout* args, smx_stream_t stream);

/* DDPG's acting loop on the device, recorded as n-step transitions straight into the uniform replay's ring: per step and
 * actor a (all actors share the episode clock tau = args->t at the first step)
 *   mu = tanh(MLP(s))                                      DDPGModel.actor (surreal/model/ddpg_net.py:13-95)
 *   act = clip(mu, -1, 1), then                            DDPGAgent.act (surreal/agent/ddpg_agent.py:155-184)
 *     gaussian: act = (float)((double)act + (0.0 + sigma_a * eps))                  (action_noise.py:14-23)
 *     OU:       x = (x + (theta * (0 - x)) * dt) + (sigma_a * root_dt) * eps;        (action_noise.py:26-39; x = 0
 *               act = (float)((double)act + x)                 when tau == 0: pre_episode, ddpg_agent.py:205-208)
 *   act = clip(act, -1, 1); the synthetic environment step of smx_synth_env_step_f32
 *   tau >= n_step - 1: transition j = tau - n_step + 1 closes (ExpSenderWrapperSSARNStepBootstrap,
 *     surreal/env/exp_sender_wrapper.py:72-112): obs = s_j, actions = a_j, obs_next = s_{tau+1} (the terminal
 *     observation before a reset), dones = d_tau, rewards = (float)(((r_j + g[e] r_{j+1}) + g[e] r_{j+2}) + ...) in
 *     fp64 with the wrapper's discount exponents, g = gpow [n_step] (gamma ** e, fp64).  The k-th closing step of a call
 *     writes actor a to row (cursor + k n + a) % capacity of obs / obs_next [capacity, D], actions [capacity, A],
 *     rewards / dones [capacity]; the caller makes n * (closing steps) <= capacity (checked: SMX_E_SHAPE).
 * carry_obs [n, n_step, D], carry_act [n, n_step, A], carry_rew [n, n_step]: the open transitions (slot tau % n_step),
 * ou [n, A] (fp64): the OU processes -- both carry over between calls.  eps [steps, n, A] standard normals, sigmas [n]
 * (fp64); neither is read with noise_type SMX_DDPG_NOISE_NONE (the deterministic agent modes).  eps NULL with another
 * noise_type: the draws of `noise`, which must then be enabled (SMX_E_NULL). */
#define SMX_DDPG_NOISE_NONE 0
#define SMX_DDPG_NOISE_GAUSSIAN 1
#define SMX_DDPG_NOISE_OU 2
struct smx_ddpg_rollout {
    const smx_mlp3_t* net;                 /* the actor (smx_synth_ddpg_rollout_f32 only) */
    const float* packed;                   /* smx_epoch_pack_f32 of net (smx_synth_ddpg_rollout_f32 only) */
    int32_t n, D, A, steps;
    int32_t t, episode_len, n_step, noise_type;
    int32_t actors_per_workgroup;          /* 4 | 8 | 16, 0: the smallest whose grid fits the CUs once */
    int32_t reserved;
    const float* eps;
    const double* sigmas;
    double theta, dt, root_dt;
    const double* gpow;
    double* ou;
    float* state;                          /* [n, D] in / out */
    const float* init_state;
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    int64_t cursor, capacity;
    struct smx_noise_stream noise;         /* eps NULL and noise.enabled: the draws are formed in the launch */
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
typedef struct smx_ddpg_rollout smx_ddpg_rollout_t;

/* What the actor of smx_synth_ddpg_rollout_f32 may be beyond the plain three layers; the two pointers switch
 * independently, and a block with both NULL is the plain actor.
 * ln: a LayerNorm behind each hidden ReLU (DDPGModel, use_layernorm):
 *   h1 = LN1(relu(W1 x + b1)), h2 = LN2(relu(W2 h1 + b2)), mu = tanh(W3 h2 + b3)
 * LN as smx_layernorm_forward_f32 (torch.nn.LayerNorm(F): biased variance, eps inside the square root, elementwise
 * affine), in its summation order: given the same ReLU row, the normalised row has that function's bits, at every block
 * size.  ln: ln1.W [H1] | ln1.b [H1] | ln2.W [H2] | ln2.b [H2], contiguous (the tail of DDPGModel's actor parameters), on
 * 4 bytes (SMX_E_ALIGN); ln_eps > 0 (SMX_E_SHAPE).
 * packed_pop: a population of perturbed actors (struct smx_param_noise below): args->n = agents * actors_per_agent
 * actors, actors_per_agent a multiple of 4; the workgroup that owns actors [a0, a0 + block) runs the actor's layers
 * (with ln: its LayerNorms too) from the copy of agent a0 / actors_per_agent in packed_pop [agents, packed_stride]
 * (smx_param_noise_refresh_f32's layout for the same ln; packed_stride >= smx_param_noise_copy_floats(.., ln != NULL), a
 * multiple of 4; 16-byte aligned), so the block size must divide actors_per_agent: args->actors_per_workgroup = 0
 * takes the size the plain launch would if it divides, else the next smaller of 16 / 8 / 4 that does; a forced size
 * that does not divide: SMX_E_SHAPE.  Everything else is the plain launch, bit for bit: an agent's actors see what a
 * launch over them alone would with args->packed = its copy.
 * measure_step: -1, or the step of the call (< args->steps) at which the workgroup that holds an agent's FIRST actor also
 * evaluates the clean actor (args->net, args->packed, ln) on that actor's observation and stores
 *   dist[p] = sqrt(sum_j ((double)(mu_j - clean_j))^2)      (fp64 sum, j ascending; mu, clean: the tanh outputs in fp32,
 *                                                            before clip and noise: ddpg_agent.py:173-175, one action pair)
 * Other steps and other workgroups do nothing for it; dist is written only by a call that measures.  Without packed_pop
 * the fields from packed_stride on are not read. */
struct smx_ddpg_actor_variant {            /* (by tag: no typedef) */
    const float* ln;                       /* NULL: no LayerNorm */
    float ln_eps;
    int32_t reserved;
    const float* packed_pop;               /* NULL: one actor for all */
    int64_t packed_stride;
    int32_t actors_per_agent, agents;
    int32_t measure_step, reserved2;
    double* dist;                          /* [agents] fp64 (measure_step >= 0) */
};
/* shapes smx_synth_ddpg_rollout_f32 takes: A <= 32, H1 and H2 multiples of 4 up to 640, D <= 512; ln != 0: those of
 * them whose 16-actor layout still holds the 2 (H1 + H2) LayerNorm floats */
int32_t smx_synth_ddpg_rollout_supported(int32_t D, int32_t H1, int32_t H2, int32_t A, int32_t ln);
/* all `steps` steps in ONE launch, in the persistent kernel shape of smx_synth_rollout_f32: a workgroup owns
 * actors_per_workgroup = 4, 8 or 16 actors for the whole rollout (0: chosen as there; anything else: SMX_E_SHAPE), the
 * actor's layers run on v_mfma_f32_4x4x1 from `packed` at every block size (smx_rows4_mma.inc.h: mu equals
 * smx_epoch_forward_f32's to fp32 rounding of the layer sums; every block size gives the same bits).  variant NULL: the
 * plain actor.  Every argument check is made before anything is launched. */
int smx_synth_ddpg_rollout_f32(const smx_ddpg_rollout_t* args, const struct smx_ddpg_actor_variant* variant,
                               smx_stream_t stream);
/* the block size the launch takes for a population of n actors (0: refused, SMX_E_SHAPE there); forced =
 * args->actors_per_workgroup */
int32_t smx_synth_ddpg_population_block(int32_t n, int32_t actors_per_agent, int32_t forced);
/* ONE step (args->steps is ignored; eps [n, A]; the step's closing transitions go to the rows from args->cursor) given
 * the actor's output mu [n, A] (row stride ld_mu) from any forward pass */
int smx_synth_ddpg_step_f32(const smx_ddpg_rollout_t* args, const float* mu, int64_t ld_mu, smx_stream_t stream);

/* An episode clock PER ACTOR for the two one-launch, low-dimensional rollouts above (the shared clock of
 * smx_synth_ppo_window_rollout_f32 / smx_synth_ddpg_rollout_f32 makes all actors end their episodes on the same step; the
 * reference's actors are n independent processes, surreal/agent/base.py:244-271).  Actor a has an episode length
 * L[a] >= 1 and a clock t[a] in [0, L[a]); one step: tau = t[a], done = (tau + 1 >= L[a]), t[a] = done ? 0 : tau + 1.
 * Everything that depends on the shared tau there depends on the actor's own here: the carry-ring slots tau % N, the
 * LSTM window-start slot, the closing rule (j = tau + 1 - N >= 0 and j % adv == 0; adv = 1 for DDPG), the reset to
 * init_state, the OU process's x = 0 at tau == 0, dones, the monitor.  What stays on the call's step index s and the actor
 * id: the exploration noise (eps[s, a, :] or the stream), noise_scale / sigmas, the population and its measure_step, the
 * LSTM state (never reset at episode ends).
 * Row order: the closing pairs (s, a) of a call are numbered s ascending, then a ascending -- the order in which n host
 * wrappers stepped in actor order insert; pair number `off` goes to row (cursor + off) % capacity.  With all clocks
 * equal that is the shared clock's (cursor + k n + a).  The numbering is a pure function of the clocks: with
 * f(x) = x >= N ? (x - N) / adv + 1 : 0, m = min(s, L - t0), r = s - m the closings of an actor in its first s steps are
 *   cnt(s) = f(t0 + m) - f(t0) + (r / L) f(L) + f(r % L)
 * and off[s, a] = sum_a' cnt_a'(s) + #{a' < a closing at s}: no atomics, nothing read back; the host forms `rows` (the
 * number of pairs) and the clocks after the call by the same rule.
 *
 * smx_actor_clock_rows_i32: row_off [steps, n] int32 <- off[s, a], -1 where (s, a) closes nothing.  ONE launch (workgroup
 * s: a sum over the actors, then a ballot / popcount scan in actor order).  t / episode_len [n] int32 on the device;
 * t_host / episode_len_host: the host arrays they were copied from, or NULL: checked before the launch (t outside
 * [0, L), L < 1: SMX_E_SHAPE).  advance outside [1, n_step], n * steps >= 2^31: SMX_E_SHAPE.  An actor whose device
 * clock is outside [0, L) closes nothing. */
struct smx_actor_clock_rows {              /* (by tag: no typedef) */
    int32_t n, steps;
    int32_t n_step, advance;
    const int32_t* t;
    const int32_t* episode_len;
    const int32_t* t_host;                 /* NULL: not checked on the host */
    const int32_t* episode_len_host;
    int32_t* row_off;                      /* [steps, n] */
};
int smx_actor_clock_rows_i32(const struct smx_actor_clock_rows* args, smx_stream_t stream);

/* The clocks of a call and its table (smx_actor_clock_rows_i32 with the call's steps, n_step and advance -- 1 for DDPG);
 * rows: the table's closing pairs.  The kernels write a record only where the actor's own clock closes one AND
 * 0 <= row_off < rows: a table that does not belong to the clocks loses records, it never writes out of bounds. */
struct smx_actor_clocks {                  /* (by tag: no typedef) */
    const int32_t* t;                      /* [n] at the call's first step */
    const int32_t* episode_len;            /* [n] */
    const int32_t* row_off;                /* [steps, n] */
    int64_t rows;
};
/* smx_synth_ppo_window_rollout_f32 / smx_synth_ddpg_rollout_f32 with per-actor clocks: the same argument blocks
 * (base.roll.t / episode_len, resp. t / episode_len, are ignored), the same supported shapes, the same checks with
 * 0 <= clocks->rows <= capacity (SMX_E_SHAPE) in place of n x closing steps <= capacity; clocks and its three pointers
 * non-NULL (SMX_E_NULL).  The clocks are read once and stored nowhere: the host knows them.  4, 8 and 16 actors per
 * workgroup give the same bits; an actor's records equal those of the shared-clock launch with episode_len = L[a]. */
int smx_synth_ppo_window_rollout_clocks_f32(const struct smx_synth_ppo_window_rollout* args,
                                            const struct smx_actor_clocks* clocks, smx_stream_t stream);
int smx_synth_ddpg_rollout_clocks_f32(const smx_ddpg_rollout_t* args, const struct smx_ddpg_actor_variant* variant,
                                      const struct smx_actor_clocks* clocks, smx_stream_t stream);

/* The dynamics of the synthetic environment, by task.  SMX_TASK_DRIFT: smx_synth_env_step_f32's (every element decays on
 * its own; a workload).  SMX_TASK_REACH (surreal_amd/env/tasks.py holds the one definition): A point masses are steered to
 * A goals, D = 3 A, the state row is [p (A) | v (A) | g (A)]; fp32, no contraction, each product rounded before the sum:
 *   a = clip(action, -1, 1);  v'[j] = clamp((0.9f v[j]) + (0.2f a[j]), -1, 1);  p'[j] = clamp(p[j] + (0.1f v'[j]), -10, 10);
 *   g'[j] = g[j];  d[j] = p'[j] - g[j];  reward = (float)(-(sum_j d[j]^2 + 0.01 sum_j a[j]^2)), both sums in fp64, j
 *   ascending, one term at a time;  done and the reset as in smx_synth_env_step_f32.
 * SMX_TASK_ARM (the same file): a planar arm of A links of length w = 2^-ceil(log2 A), D = 2 A + 2, the state row is
 * [theta (A) | omega (A) | g (2)] -- each link's absolute orientation, its angular velocity, the fingertip's goal; the rule:
 *   a = clip(action, -1, 1);  omega'[j] = clamp((0.9f omega[j]) + (0.4f a[j]), -1, 1);
 *   theta'[j] = clamp(theta[j] + (0.2f omega'[j]), -3.1415927f, 3.1415927f)  (joint limits, no wrap);  g' = g;
 *   s[j], c[j] = theta'[j] P_S(theta'[j]^2), P_C(theta'[j]^2): the Taylor polynomials of sine and cosine with the fp32
 *   coefficients (float)((-1)^k / (2k+1)!), k <= 8, and (float)((-1)^k / (2k)!), k <= 9, by Horner, each operation rounded
 *   (the polynomials are the definition: no library function);
 *   dx = (sum_j c[j]) w - g[0];  dy = (sum_j s[j]) w - g[1];  reward = (float)(-((dx dx + dy dy) + 0.01 sum_j a[j]^2)),
 *   the three sums and what follows them in fp64, j ascending, one term at a time.
 * smx_synth_task_supported: 1 where the task entry points below take (task, D, A) -- DRIFT: D, A > 0; REACH: D == 3 A
 * and A <= 21; ARM: D == 2 A + 2 and A <= 30 (a row's elements sit in one wavefront) -- else 0 (an unknown task too).
 * The three entry points take the arguments of smx_synth_env_step_f32, smx_synth_ppo_window_rollout_f32 and
 * smx_synth_ddpg_rollout_f32 (the plain actor: no variant) and a task.  With SMX_TASK_DRIFT each forwards to that entry
 * point.  What smx_synth_task_supported refuses returns SMX_E_UNSUPPORTED before any launch; every other check is the
 * forwarded entry point's.  4, 8 and 16 actors per workgroup give the same bits. */
#define SMX_TASK_DRIFT 0
#define SMX_TASK_REACH 1
#define SMX_TASK_ARM 2
int32_t smx_synth_task_supported(int32_t task, int32_t D, int32_t A);
int smx_synth_task_env_step_f32(float* state, const float* init_state, const float* actions,
                                int32_t n, int32_t D, int32_t A, int32_t t, int32_t episode_len,
                                int32_t slot, int32_t T, float* obs_roll, float* act_roll,
                                float* rew_roll, float* done_roll, const struct smx_episode_monitor* mon,
                                int32_t task, smx_stream_t stream);
int smx_synth_ppo_window_rollout_task_f32(const struct smx_synth_ppo_window_rollout* args, int32_t task,
                                          smx_stream_t stream);
int smx_synth_ddpg_rollout_task_f32(const smx_ddpg_rollout_t* args, int32_t task, smx_stream_t stream);

/* The episodes of SMX_TASK_REACH as a counter-based stream: element k < 3 A of the row [p | v | g] that (seed, global actor
 * id g, episode index e) begins with is a pure function of the four, formed inside the launch that steps over the episode's
 * end (csrc/smx_philox.inc.h has the expressions; surreal_amd/env/tasks.py the one definition):
 *   x[0..3] = Philox4x32-10(counter = (g, low32(e), high32(e), 0x52530000 | (k >> 2)), key = (low32(seed), high32(seed)))
 *   u = (float)(x[k & 3] >> 8) * 2^-23 - 1       (a 24-bit integer, scaled, minus one: exact in fp32; u in [-1, 1))
 *   a position (k < A) or a goal (k >= 2 A) is u; a velocity is +0.
 * SMX_TASK_ARM draws its row [theta | omega | g], k < 2 A + 2, from the same blocks: an orientation (k < A) is u, an
 * angular velocity +0, a goal coordinate (k >= 2 A) 0.25f * u.
 * The fourth counter word keeps these blocks apart from the exploration stream's (j >> 2 < 16) and the parameter noise's
 * (0x504E0001).  `episode` is the index of the NEXT episode to begin: the i-th episode end of a call (i from 0; the
 * actors share one clock, so they share the index) draws episode + i for every actor, and the caller adds the call's
 * episode ends afterwards -- nothing is written back.  An actor's reset states depend on its global id and the episode
 * index only: not on n, on the steps of a call, on how a run is cut into calls or on how the actors are split over launches.
 * smx_reset_fill_f32: out [n, D] <- the rows of episode resets->episode (enabled is not read); task must be one with a
 * reset distribution (SMX_TASK_REACH with D == 3 A', A' <= 21, or SMX_TASK_ARM with D == 2 A' + 2, A' <= 30: else
 * SMX_E_UNSUPPORTED).
 * The three *_resets_f32 entry points take what the *_task_f32 ones take and a stream.  resets NULL or !resets->enabled:
 * exactly the task entry point (init_state is read at an episode end).  Enabled: init_state is not read (it may be any
 * non-NULL pointer).  Before any launch: an enabled stream on SMX_TASK_DRIFT is SMX_E_UNSUPPORTED; actor_base < 0,
 * actor_base + n > 2^32 or episode < 0 is SMX_E_SHAPE; every other check is the task entry point's.
 *
 * Per-step DISTURBANCES from the same stream make the tasks stochastic.  The word `reserved` holds the bits of an fp32 scale
 * s, 0 <= s <= 1 (memcpy a float into it; it keeps its name, offset and size, and the zero bit pattern -- what every caller
 * has passed so far -- means none); it is read only when `enabled`.  With s != 0, step t (0 <= t < episode_len) of the
 * episode under way e (0 <= e < 2^32) of global actor g draws, for joint / mass j < A,
 *   x[0..3] = Philox4x32-10(counter = (g, low32(e), t, 0x44530000 | (j >> 2)), key = (low32(seed), high32(seed)))
 *   w[j]    = (float)(x[j & 3] >> 8) * 2^-23 - 1                  (the reset rows' exact conversion; w in [-1, 1))
 *   REACH:  v'[j]     = clamp(((0.9f v[j]) + (0.2f a[j])) + (s * w[j]), -1, 1)
 *   ARM:    omega'[j] = clamp(((0.9f omega[j]) + (0.4f a[j])) + (s * w[j]), -1, 1)
 * in fp32 without contraction, the product rounded before the sum; everything downstream of v' / omega' is unchanged.  With
 * s == 0 the term is NOT added: such a stream leaves the bytes it left, signed zeros included.  The tag 0x4453.... keeps
 * these blocks apart from the reset rows' (0x5253....), the exploration stream's and the parameter noise's.  The draw is a
 * pure function of (seed, g, e, t, j): not of how a run is cut into calls, of the block size or of how the actors are split
 * over launches.  Every entry point that takes a stream honours it, in the lane that forms v'[j] / omega'[j] (ten Philox
 * rounds a step, no memory read): smx_synth_task_env_step_resets_f32 (its `t` is the step in the episode; e = episode - 1),
 * smx_synth_ppo_window_rollout_resets_f32 (MLP and LSTM), smx_synth_ddpg_rollout_resets_f32,
 * smx_synth_ddpg_rollout_variant_task_f32 (all four actors) -- a recording launch is in episode e = episode - 1 + (its
 * episode ends so far) -- and smx_synth_ppo_eval_f32, smx_synth_ddpg_eval_f32 and both *_eval_sets_f32, whose row (a, i) is
 * in episode first_episode + i: a disturbed evaluation returns what the monitor records for that (seed, actor, episode, s).
 * Before any launch, with s != 0 on an enabled stream: a NaN, negative or > 1 scale, or an episode under way with an index
 * < 0 or >= 2^32 (a recording call: episode - 1 .. episode - 1 + (t + steps - 1) / episode_len; an evaluation:
 * first_episode .. first_episode + episodes - 1; the per-step call also t outside [0, episode_len)): SMX_E_SHAPE;
 * SMX_TASK_DRIFT: SMX_E_UNSUPPORTED, as for every enabled stream. */
struct smx_reset_stream {                  /* (by tag: no typedef) */
    uint64_t seed;
    int64_t actor_base;                    /* global id of local actor 0 */
    int64_t episode;                       /* index of the next episode to begin */
    int32_t enabled, reserved;             /* reserved: the bits of the fp32 disturbance scale (0: none) */
};
int smx_reset_fill_f32(const struct smx_reset_stream* resets, int32_t task, int32_t n, int32_t D, float* out,
                       smx_stream_t stream);
int smx_synth_task_env_step_resets_f32(float* state, const float* init_state, const float* actions,
                                       int32_t n, int32_t D, int32_t A, int32_t t, int32_t episode_len,
                                       int32_t slot, int32_t T, float* obs_roll, float* act_roll,
                                       float* rew_roll, float* done_roll, const struct smx_episode_monitor* mon,
                                       int32_t task, const struct smx_reset_stream* resets, smx_stream_t stream);
int smx_synth_ppo_window_rollout_resets_f32(const struct smx_synth_ppo_window_rollout* args, int32_t task,
                                            const struct smx_reset_stream* resets, smx_stream_t stream);
int smx_synth_ddpg_rollout_resets_f32(const smx_ddpg_rollout_t* args, int32_t task,
                                      const struct smx_reset_stream* resets, smx_stream_t stream);

/* smx_synth_ddpg_rollout_f32's four actors (variant: as there; NULL or all-zero: the plain actor) on a task, with an
 * optional reset stream: the cross product of the actor variants with the tasks, on the shared clock.
 *   SMX_TASK_DRIFT, resets NULL or !resets->enabled: forwards to smx_synth_ddpg_rollout_f32(args, variant, stream).
 *   SMX_TASK_DRIFT with an enabled stream, an unknown task: SMX_E_UNSUPPORTED.
 *   SMX_TASK_REACH, SMX_TASK_ARM: every variant smx_synth_ddpg_rollout_f32 takes, the step's environment half replaced by the task's
 *   and the episodes' first rows by the stream's, as in smx_synth_ddpg_rollout_resets_f32 -- whose bytes the plain actor
 *   leaves.  Nothing else of a step changes: a population's measuring step, the LayerNorm's LDS copy, the episode monitor
 *   and the noise stream are smx_synth_ddpg_rollout_f32's.
 * The refusals are the union of those entry points', with their codes, all before any launch.  Per-actor clocks
 * (smx_synth_ddpg_rollout_clocks_f32) run on SMX_TASK_DRIFT only.  4, 8 and 16 actors per workgroup give the same bits. */
int smx_synth_ddpg_rollout_variant_task_f32(const smx_ddpg_rollout_t* args, const struct smx_ddpg_actor_variant* variant,
                                            int32_t task, const struct smx_reset_stream* resets, smx_stream_t stream);

/* Evaluation on the device: whole episodes of the policy in ONE launch, nothing recorded -- the evaluation workers of
 * the reference (agent_mode eval_deterministic / eval_stochastic: surreal/agent/base.py:277-345 get_env, prepare_env_eval
 * and main_eval around the per-step loop of base.py:244-271, behind surreal/env/monitor.py:164-218 EvalTensorplexMonitor)
 * and the offline surreal/main/rollout.py:1-87, which step one host environment per process.
 * Episode e of actor g is a pure function of (parameters, streams, g, e), so the (actor, episode) pairs are independent
 * ROWS: row r = a * episodes + i is episode resets.episode + i (first_episode + i) of local actor a.  The launch runs
 * n * episodes rows on workgroups of actors_per_workgroup = 4, 8 or 16 rows (0: chosen as in smx_synth_rollout_f32, from
 * the rows) and walks every row through exactly episode_len steps:
 *   start:  resets.enabled (SMX_TASK_REACH, SMX_TASK_ARM): the row the reset stream draws for (seed, actor_base + a,
 *           resets.episode + i), formed in the launch; else init_state[a] ([n, D]; with an enabled stream not read, any
 *           non-NULL pointer).  No state buffer is read or written; an LSTM policy starts every episode from zero h, c
 *           (PPOAgent.reset, surreal/agent/ppo_agent.py:169-178).
 *   step:   the policy step of smx_synth_ppo_window_rollout_f32 (PPO: z-filter, [one LSTM layer,] policy MLP, act(z + b3),
 *           clip; surreal/agent/ppo_agent.py:106-154) resp. smx_synth_ddpg_rollout_f32 with SMX_DDPG_NOISE_NONE (tanh, clip;
 *           surreal/agent/ddpg_agent.py:155-184), then the task's dynamics -- a row's actions and rewards have the bits of
 *           those launches, at every block size.
 *   PPO with noise.enabled (eval_stochastic): action = clip(mean + exp(log_var) * normal(noise.seed, noise.actor_base + a,
 *           noise.step + i * episode_len + t, j)) at step t of the row -- what a serial run of the actor's episodes on that
 *           stream (noise.step: first_step) draws; there is no eps tensor and no noise_scale.
 *   return: returns[a, i] ([n, episodes] fp64) = (((0.0 + r_0) + r_1) + ...) the fp32 step rewards added in fp64 in step
 *           order by the one lane that forms them (struct smx_episode_monitor's sum), stored once after the last step.
 * lstm NULL: a plain-MLP policy (lstm_packed, hidden unused); else net->D == lstm->H as in smx_synth_lstm_rollout_f32.
 * Before any launch: an enabled reset stream on SMX_TASK_DRIFT, or what smx_synth_eval_supported refuses:
 * SMX_E_UNSUPPORTED; actor_base < 0 or actor_base + n > 2^32 of an enabled stream, resets.episode < 0, n < 1, episodes < 1,
 * episode_len < 1, n * episodes >= 2^31, episodes * episode_len >= 2^31, actors_per_workgroup not 0 | 4 | 8 | 16:
 * SMX_E_SHAPE; a NULL required pointer (the z-filter's three: all or none): SMX_E_NULL. */
struct smx_synth_ppo_eval {                /* (by tag: no typedef) */
    const smx_mlp3_t* net;
    const float* packed;                   /* smx_epoch_pack_f32 of net */
    int32_t out_act, n;
    const float* log_var;
    const float* zsum;
    const float* zsumsq;
    const float* zcount;
    float zeps;
    int32_t episodes, episode_len, task;
    int32_t actors_per_workgroup, hidden;
    const smx_lstm_t* lstm;
    const float* lstm_packed;              /* smx_lstm_rollout_pack_f32 of lstm */
    const float* init_state;
    struct smx_reset_stream resets;        /* resets.episode: first_episode */
    struct smx_noise_stream noise;         /* noise.step: first_step */
    double* returns;                       /* [n, episodes] */
};
struct smx_synth_ddpg_eval {               /* (by tag: no typedef) */
    const smx_mlp3_t* net;                 /* the actor */
    const float* packed;
    int32_t n, episodes, episode_len, task;
    int32_t actors_per_workgroup, reserved;
    const float* init_state;
    struct smx_reset_stream resets;
    double* returns;
};
/* shapes the two take (host-side): ddpg != 0 the plain DDPG actor (H must be 0), else a PPO policy with H LSTM units (0: a
 * plain MLP); those of smx_synth_ddpg_rollout_supported(.., 0) resp. smx_synth_ppo_window_rollout_supported that
 * smx_synth_task_supported(task, D, A) takes too */
int32_t smx_synth_eval_supported(int32_t ddpg, int32_t task, int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A);
int smx_synth_ppo_eval_f32(const struct smx_synth_ppo_eval* args, smx_stream_t stream);
int smx_synth_ddpg_eval_f32(const struct smx_synth_ddpg_eval* args, smx_stream_t stream);

/* Several parameter sets of one policy architecture -- a learning curve's snapshots, an actor and its target, the
 * perturbed actors of a parameter-noise population -- evaluated in ONE launch on the same episodes.
 *
 * A SNAPSHOT is one policy's parameters as one contiguous blob of smx_eval_snapshot_floats floats (a multiple of 64; every
 * block on 16 bytes, the padding between and behind the blocks zero), D the observation's width (the LSTM's input width
 * where H > 0 units stand in front of the actor):
 *   DDPG (ddpg != 0, H == 0, zfilter == 0):  [smx_epoch_pack_f32's layout of the actor | b1 | b2 | b3] -- by definition
 *       smx_param_noise_copy_floats(D, H1, H2, A, 0) floats in that order: a plain-actor population is an array of snapshots;
 *   PPO:  the same four, then log_var [A]; with zfilter != 0 zsum [D] | zsumsq [D] | zcount [1]; with H > 0
 *       smx_lstm_rollout_pack_f32's layout of the LSTM (its gate biases included).
 * 0: a shape smx_synth_eval_supported refuses on every task, a DDPG actor with a z-filter, zfilter not 0 | 1. */
int64_t smx_eval_snapshot_floats(int32_t ddpg, int32_t D, int32_t H, int32_t H1, int32_t H2, int32_t A, int32_t zfilter);
struct smx_eval_snapshot_src {             /* (by tag: no typedef) what names a policy in the evaluation argument blocks */
    const smx_mlp3_t* net;                 /* the actor (with lstm: net->D == lstm->H) */
    const float* log_var;                  /* PPO [A]; not read with ddpg != 0 */
    const float* zsum;                     /* the z-filter's three, or none */
    const float* zsumsq;
    const float* zcount;
    const smx_lstm_t* lstm;                /* NULL: no LSTM stem */
    int32_t ddpg, reserved;
};
/* blob (16-byte aligned) <- the snapshot of the live parameters behind src: no host synchronisation, at most three
 * launches (smx_epoch_pack_f32 and smx_lstm_rollout_pack_f32 into the blob, one copy kernel for the small arrays and the
 * padding).  Writes exactly smx_eval_snapshot_floats floats.  A NULL pointer (the z-filter's three: all or none):
 * SMX_E_NULL; net->D != lstm->H: SMX_E_SHAPE; a policy whose snapshot has 0 floats: SMX_E_UNSUPPORTED; blob: SMX_E_ALIGN. */
int smx_eval_snapshot_store_f32(const struct smx_eval_snapshot_src* src, float* blob, smx_stream_t stream);

/* The launches.  args: the shapes (net, lstm, hidden, out_act, zeps), n, episodes, episode_len, task,
 * actors_per_workgroup, init_state and the streams, as above -- its parameter pointers (packed, log_var, zsum, zsumsq,
 * zcount, lstm_packed, the arrays behind net and lstm) are NOT read: set s reads its parameters from blobs + s * stride.
 * args->returns is [sets, n, episodes] fp64.  ONE launch of sets x ceil(n episodes / block) workgroups: every workgroup
 * belongs to one set, every set has its own tail block; actors_per_workgroup 0 chooses the block from the sets * n *
 * episodes rows as smx_synth_rollout_f32 does from its rows.  returns[s] has the bits smx_synth_*_eval_f32 leaves for a
 * policy holding set s's parameters, at every block size: row (a, i) of every set starts, draws and sums alike.
 * Before any launch: a NULL sets or blobs: SMX_E_NULL; sets < 1, sets > 65535, sets * n * episodes >= 2^31, stride <
 * smx_eval_snapshot_floats(.., zfilter) or no multiple of 4, zfilter not 0 | 1 (DDPG: not 0): SMX_E_SHAPE; blobs not on
 * 16 bytes: SMX_E_ALIGN; and what smx_synth_*_eval_f32 refuses, with its codes (the pointers that are not read apart). */
struct smx_eval_sets {                     /* (by tag: no typedef) */
    const float* blobs;                    /* [sets, stride] */
    int64_t stride;                        /* floats from one snapshot to the next */
    int32_t sets;
    int32_t zfilter;                       /* != 0: the snapshots hold a z-filter's sums, and the policy filters */
};
int smx_synth_ppo_eval_sets_f32(const struct smx_synth_ppo_eval* args, const struct smx_eval_sets* sets,
                                smx_stream_t stream);
int smx_synth_ddpg_eval_sets_f32(const struct smx_synth_ddpg_eval* args, const struct smx_eval_sets* sets,
                                 smx_stream_t stream);

/* Parameter-space noise of the device actors (surreal/agent/param_noise.py): a population of perturbed actors, one per
 * AGENT -- a group of consecutive actors that share one perturbation, as the actors of one reference agent process do
 * (an agent here spans at least the 4 actors of one MFMA row block, where the reference's spans one environment).  The
 * perturbation is a pure function: for global agent id g = agent_base + p, generation q and element i of the actor's flat
 * parameters W1 [H1, D] | b1 | W2 [H2, H1] | b2 | W3 [OUT, H2] | b3 (row-major each: the order DDPGModel keeps them in)
 *   z = component i & 3 of Philox4x32-10(counter = (g, q, i >> 2, 0x504E0001), key = (low32(seed), high32(seed))),
 *       through the word -> normal conversion of struct smx_noise_stream (the same inline function; the fixed fourth
 *       counter word keeps these blocks apart from the exploration stream's, whose fourth word is j >> 2 < 16)
 *   perturbed_i = w_i + (float)sigma[p] * z            in fp32, the product first; the build does not contract
 * `net` is read, never written.  g and q must lie in [0, 2^32) (SMX_E_SHAPE).
 * A LayerNorm actor (ln: the clean ln1.W | ln1.b | ln2.W | ln2.b): the flat parameters go on with those four (element
 * indices i behind b3's: the first six arrays keep theirs, so they are perturbed as without a LayerNorm), the same rule. */
struct smx_param_noise {                   /* (by tag: no typedef) */
    const smx_mlp3_t* net;                 /* the clean actor */
    uint64_t seed;
    int64_t agent_base;                    /* global id of agent 0 */
    int64_t generation;
    int32_t agents;                        /* P */
    int32_t adaptive;                      /* refresh: != 0 adapts sigma first (when acts > 0) */
    int64_t acts;                          /* refresh: act() calls since the last one */
    double alpha, target;                  /* refresh, adaptive */
    double* sigma;                         /* [P] fp64, in / out */
    const double* dist;                    /* [P] fp64: the action distances (refresh, adaptive and acts > 0) */
    float* packed_pop;                     /* refresh: [P, packed_stride] out, 16-byte aligned */
    int64_t packed_stride;                 /* floats, >= smx_param_noise_copy_floats(.., ln != NULL), a multiple of 4 */
    const float* ln;                       /* NULL: a plain actor */
};
/* floats of one agent's copy: [smx_epoch_pack_f32's layout of the actor | b1 | b2 | b3], with ln != 0 [| ln1.W | ln1.b |
 * ln2.W | ln2.b], rounded up to 64 */
int64_t smx_param_noise_copy_floats(int32_t D, int32_t H1, int32_t H2, int32_t OUT, int32_t ln);
/* out [H1 D + H1 + H2 H1 + H2 + OUT H2 + OUT (+ 2 (H1 + H2) with ln)] <- agent p's perturbed flat parameters (packed_pop,
 * dist, acts: not read) */
int smx_param_noise_fill_f32(const struct smx_param_noise* pn, int32_t p, float* out, smx_stream_t stream);
/* AdaptiveNormalParameterNoise.apply / NormalParameterNoise.apply for all P agents, no host synchronisation, at most two
 * launches: with adaptive != 0 and acts > 0 first, in a launch of its own,
 *   sigma[p] <- dist[p] / acts > target ? sigma[p] / alpha : sigma[p] * alpha      (fp64; param_noise.py:65-70)
 * then the copy of every agent's perturbed actor into packed_pop + p * packed_stride: the five blocks of
 * smx_epoch_pack_f32 bit for bit as it lays out a net holding the perturbed parameters (its padding exactly zero: noise
 * goes to logical elements only), the perturbed biases b1 | b2 | b3 behind them, with ln the perturbed four behind the
 * biases, zeros up to copy_floats. */
int smx_param_noise_refresh_f32(const struct smx_param_noise* pn, smx_stream_t stream);

/* The same step for actors with a camera (the reference's pixel DDPG configurations, ddpg_configs.py:176-228:
 * FrameStackWrapper in front of a CNN perception): smx_synth_ddpg_step_f32 on args->base (mu [n, A] = the actor's
 * output on the perception of obs_pixel), and the frames in the same launch.  F = C*H*W bytes per frame, S =
 * frame_stacks, tau = base.t, L = base.episode_len, Hd = hist_len >= n_step + S, p = hist_pos.
 *   history:  hist[a, (p - tau + u) mod Hd] holds the raw frame of step u of the current episode, tau - Hd < u <= tau;
 *   frame(u, s0)[c, y, x] = (37 c + 5 y + 11 x + 3 u + (int)(100 |s0|)) % 256        (smx_synth_frame_u8's rule)
 *   stacked(u)[i] = frame of step max(u - S + 1 + i, 0), 0 <= i < S                     (stack_sources)
 *   new = frame(tau + 1, s'_0): s' the next state before any reset (the terminal one when tau + 1 >= L)
 * This launch writes
 *   tau + 1 < L:   hist[a, (p + 1) mod Hd] = new;      obs_pixel[a] = stacked(tau + 1)
 *   tau + 1 >= L:  hist[a, (p + 1) mod Hd] = frame(0, init_state[a, 0]);  obs_pixel[a] = that frame S times
 *   tau >= n_step - 1, row = (base.cursor + a) % capacity, j = tau - n_step + 1:
 *                  pixel[row] = stacked(j);  pixel_next[row] = stacked(tau + 1) (its last frame: new)
 * so the caller's next call passes t = tau + 1 (0 after L) and p = (p + 1) mod Hd.  pixel / pixel_next are uint8
 * [capacity, S*F], obs_pixel uint8 [n, S*F] (what the actors act on at the next step), hist uint8 [n, Hd, F]; the
 * frames read (steps tau - n_step - S + 2 .. tau) never share a slot with the one written. */
struct smx_ddpg_pixel_step {           /* (by tag: no typedef) */
    smx_ddpg_rollout_t base;           /* steps, net, packed, actors_per_workgroup: ignored */
    int32_t C, H, W, frame_stacks;
    int32_t hist_len, hist_pos;
    uint8_t* hist;
    uint8_t* pixel;
    uint8_t* pixel_next;
    uint8_t* obs_pixel;
};
int smx_synth_ddpg_pixel_step(const struct smx_ddpg_pixel_step* args, const float* mu, int64_t ld_mu,
                              smx_stream_t stream);

/* The frame-pool layout of the camera replay: every raw frame is stored ONCE.  The reference's pixel DDPG configuration
 * ships frame_stack_concatenate_on_env: False (surreal/main/ddpg_configs.py:119-122: the agent sends the stack as a list
 * of frames "so that identical frames aren't duplicated in memory", the learner joins them, surreal/learner/ddpg.py:
 * 430-440); the stacked tables above hold each frame up to 2 S times.  Per replay:
 *   pool        uint8 [n, P, F]: actor a's frame with counter i (int64, monotone per actor) in slot i mod P;
 *   an environment step writes ONE frame, the observation after the step, at counter f + 1; a terminal step two: the
 *   terminal frame at f + 1 and the new episode's first frame at f + 2.  The frame of episode step u has counter
 *   first + u, `first` the counter of the episode's reset frame;
 *   a ring row carries, in place of pixel / pixel_next, frame_next (the counter of pixel_next's newest frame),
 *   frame_first (its episode's `first`) and frame_actor (int32: whose pool) -- [capacity] each;
 *   stack(top)[i] = frame max(top - S + 1 + i, frame_first), 0 <= i < S   (FrameStackWrapper, surreal/env/wrapper.py:
 *   407-453: a reset fills the history with the first frame; smx_frame_stack_u8's rule), pixel_next = stack(frame_next),
 *   pixel = stack(frame_next - n_step);
 *   a row is live while its oldest frame max(frame_first, frame_next - n_step - S + 1) >= f_now - P + 1; the host keeps
 *   the number of live rows (the newest ones of the ring) and samples among them only.
 *
 * smx_synth_ddpg_pixel_pool_step: smx_synth_ddpg_pixel_step in this layout (the shared episode clock; base as there, the
 * same step, monitor and noise stream).  frame = f, the counter of the current step's frame, episode_first = first; the
 * launch renders frame f + 1 once into the pool (on a terminal step also the new episode's first frame, counter f + 2),
 * writes obs_pixel [n, S*F] -- the stacked observation of the next step, its older frames out of the pool -- and at a
 * closing step (tau >= n_step - 1) frame_next = f + 1, frame_first = first, frame_actor = a of row (base.cursor + a) %
 * capacity.  The caller's next call passes f + 1 (terminal: f + 2, episode_first = f + 2).  pool_len < n_step + S + 1,
 * episode_first < 0 or > frame: SMX_E_SHAPE; the counter columns off their element size: SMX_E_ALIGN. */
struct smx_ddpg_pixel_pool_step {      /* (by tag: no typedef) */
    smx_ddpg_rollout_t base;           /* steps, net, packed, actors_per_workgroup: ignored */
    int32_t C, H, W, frame_stacks;
    int64_t pool_len;                  /* P */
    int64_t frame, episode_first;
    uint8_t* pool;
    uint8_t* obs_pixel;
    int64_t* frame_next;
    int64_t* frame_first;
    int32_t* frame_actor;
};
int smx_synth_ddpg_pixel_pool_step(const struct smx_ddpg_pixel_pool_step* args, const float* mu, int64_t ld_mu,
                                   smx_stream_t stream);

/* A whole uniform sample of a frame-pool replay in ONE launch (UniformReplay.sample, surreal/replay/uniform_replay.py:
 * 36-47, with the learner's frame join, surreal/learner/ddpg.py:430-440): smx_uniform_gather_multi over `jobs` (1..8
 * field tables) and, for the same rows, pixel / pixel_next [rows, S*F] built from the pool by the stack rule above,
 * straight into the caller's buffers.  Row i is idx[i], or (idx NULL) (base + u) % capacity with u = the i-th draw of
 * smx_uniform_indices(len, seed, offset): base = (cursor - live) mod capacity and len = live make that a draw among the
 * live rows.  idx_out as in smx_uniform_gather_multi.  Frames move in 16-byte units where F and the buffers allow, else in
 * 4- or single-byte ones.  pool_len < n_step + S + 1, base outside [0, capacity): SMX_E_SHAPE. */
struct smx_gather_pool {               /* (by tag: no typedef) */
    const uint8_t* pool;               /* [actors, pool_len, frame_bytes] */
    int64_t pool_len, frame_bytes;
    int32_t actors, frame_stacks, n_step, reserved;
    const int64_t* frame_next;         /* [capacity] */
    const int64_t* frame_first;
    const int32_t* frame_actor;
    uint8_t* pixel;                    /* [rows, S*F] out */
    uint8_t* pixel_next;
    int64_t base;
};
int smx_uniform_gather_pool(const smx_gather_job_t* jobs, int32_t njobs, const struct smx_gather_pool* pool,
                            int64_t capacity, int64_t rows, const int64_t* idx, int64_t len, uint64_t seed,
                            uint64_t offset, int64_t* idx_out, smx_stream_t stream);

/* ONE step of PPO's moving windows for actors with a camera (the reference's pixel PPO configuration: FrameStackWrapper,
 * surreal/env/wrapper.py:407-472, in front of the CNN stem; PPOAgent.act, surreal/agent/ppo_agent.py:106-154; the
 * windows of ExpSenderWrapperMultiStepMovingWindowWithInfo, surreal/env/exp_sender_wrapper.py:153-264), given the
 * policy mean mu [n, A] (row stride ld_mu) of the layers before it -- the per-step record launch of the windowed
 * rollout whose perception, LSTM step and actor run between two of them.  Per actor a, tau = t, N = n_step,
 * adv = advance, S = frame_stacks, F = C*H*W, Hd = hist_len >= N + S, p = hist_pos:
 *   head:   sd = exp(log_var) * noise_scale[a] (noise_scale NULL: 1), action = clip(eps * sd + mu, -1, 1) (eps NULL:
 *           clip(mu)), pd = [mu | sd]                                        (smx_diaggauss_sample_f32's expressions)
 *   step:   smx_synth_env_step_f32's dynamics, state in / out (init_state after the terminal step)
 *   rings:  slot tau % N of carry_obs / carry_act / carry_rew / carry_pd <- the state before the step, the action, the
 *           reward, the pd; when tau % adv == 0 and h_before / c_before [n, hidden] are given, slot
 *           (tau / adv) % ceil(N / adv) of carry_cells <- them (smx_synth_ppo_window_rollout's layout and slot rule)
 *   frames: the history and stacking rule of smx_synth_ddpg_pixel_step: new = frame(tau + 1, s'_0);
 *           tau + 1 < L:  hist[a, (p + 1) mod Hd] = new, obs_pixel[a] = stacked(tau + 1); else the new episode's first
 *           frame frame(0, init_state[a, 0]) there and S times in obs_pixel[a]
 *   window j = tau + 1 - N closes when j >= 0 and j % adv == 0, into row (cursor + a) % capacity (the caller advances
 *           cursor by n per closing step): obs [N, D], actions [N, A], rewards [N], pds [N, 2A] out of the rings in
 *           episode order, dones [N] 0 but the last (1 when tau + 1 >= L), obs_next [D] the observation after the step
 *           (the terminal one), cells [2, hidden] from the ring slot of j (cells NULL: not written),
 *           pixel [N, S*F] = stacked(j + u) for window step u, pixel_next [S*F] = stacked(tau + 1)
 * so the caller's next call passes t = tau + 1 (0 after L) and p = (p + 1) mod Hd.  The frames read (steps
 * tau - N - S + 2 .. tau) never share a slot with the one written.  A <= SMX_PPO_PIXEL_STEP_MAX_A
 * (SMX_E_UNSUPPORTED), n <= capacity, n <= 65535.  copy_workgroups: the workgroups per actor that move frames (0: sized
 * by the bytes this step moves -- a closing step has (N + 1) S - 1 destination frames more than any other). */
#define SMX_PPO_PIXEL_STEP_MAX_A 64
struct smx_synth_ppo_pixel_window_step {   /* (by tag: no typedef) */
    int32_t n, D, A, hidden;               /* hidden: the LSTM's units (0: a policy without one) */
    int32_t t, episode_len, n_step, advance;
    const float* log_var;                  /* [A] */
    const float* noise_scale;              /* [n] or NULL */
    const float* eps;                      /* [n, A] standard normals, or NULL (deterministic, or the draws of `noise`) */
    float* state;                          /* [n, D] in / out */
    const float* init_state;
    const float* h_before;                 /* [n, hidden] the LSTM state the step started from, or NULL */
    const float* c_before;
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* carry_pd;
    float* carry_cells;                    /* NULL without an LSTM */
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    float* pds;
    float* cells;                          /* NULL without an LSTM */
    int64_t cursor, capacity;
    int32_t C, H, W, frame_stacks;
    int32_t hist_len, hist_pos;
    int32_t copy_workgroups, reserved;
    uint8_t* hist;                         /* [n, Hd, F] */
    uint8_t* pixel;                        /* [capacity, N, S*F] */
    uint8_t* pixel_next;                   /* [capacity, S*F] */
    uint8_t* obs_pixel;                    /* [n, S*F] */
    struct smx_noise_stream noise;         /* eps NULL and noise.enabled: the draws are formed in the launch */
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
int smx_synth_ppo_pixel_window_step(const struct smx_synth_ppo_pixel_window_step* args, const float* mu, int64_t ld_mu,
                                    smx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Recording the steps of n HOST-stepped environments (GymAdapter, DMControlAdapter, RobosuiteWrapper: simulators that
 * end their episodes whenever they like) into the replays' device rings: what n of the reference's experience wrappers
 * do per step on the host -- Python queues, deep copies, one insert per experience (surreal/env/exp_sender_wrapper.py:
 * 72-112 and 153-264, restated as index arithmetic in surreal_amd/env/exp_sender_wrapper.py) -- as ONE launch per step
 * for all actors.  Every actor has an episode clock OF ITS OWN, kept by the host (it sees the dones):
 *   t [n] int32       the actor's step within its episode (>= 0)
 *   rank [n] int32    -1: the actor closes nothing this step; else its position among this step's closing actors in
 *                     ascending actor order: it writes row (cursor + rank) % capacity, so the rows of a step are dense and
 *                     in the order n host wrappers stepped in actor order would have inserted them; rows = their number
 *   t_host / rank_host  the host arrays t / rank were copied from, or NULL: checked before the launch (t < 0, rank outside
 *                     [-1, n), closing actors != rows: SMX_E_SHAPE).  The kernels skip an actor with t < 0 and treat a
 *                     rank outside [0, rows), or one the clock does not allow, as -1: nothing is written out of bounds.
 *   cur_obs [n, D]    in: what each actor acted on; out: its next acting observation -- step_obs_reset[a] where
 *                     step_dones[a] != 0 (step_obs_reset NULL: step_obs_next[a]), else step_obs_next[a]
 *   step_*            this step's results on the device: actions [n, A], obs_next [n, D] (the terminal observation on
 *                     done), rewards [n], dones [n] (0 / 1), obs_reset [n, D] (only the rows of done actors are read)
 * These launches move bytes and do no arithmetic (but the n-step reward): no shape limit beyond positive sizes, 16-byte
 * accesses for every field whose row width is a multiple of 4 floats and whose buffers are 16-byte aligned, 4-byte ones
 * otherwise.  No atomics.  mon: the episode monitor (ep_reward NULL: none), fed episode_account(a, reward, done) by the
 * lane that owns the actor's reward.
 *
 * smx_record_ppo_window_step_f32: one step of ExpSenderWrapperMultiStepMovingWindowWithInfo per actor, tau = t[a],
 * N = n_step, adv = advance, S = ceil(N / adv); rings and tables in smx_synth_ppo_window_rollout's layout:
 *   slot tau % N of carry_obs / carry_act / carry_rew / carry_pd <- cur_obs, step_actions, step_rewards, step_pds [n, 2A];
 *   with h_before / c_before [n, hidden] and tau % adv == 0, slot (tau / adv) % S of carry_cells <- them
 *   window j = tau + 1 - N closes iff j >= 0 and j % adv == 0 (that is what rank >= 0 must mean), into its row: obs
 *     [N, D], actions [N, A], rewards [N], pds [N, 2A] in episode order, dones [N] zeros but the last = step_dones[a]
 *     (windows never cross an episode), obs_next [D] = step_obs_next[a], cells [2, hidden] the state before step j
 *     (cells NULL: not written).  The window's last step comes from the step's inputs, its N - 1 older ones from the
 *     rings, so no workgroup reads what another one writes in the same launch.
 * copy_workgroups: the workgroups per actor that move a closing window's older steps (0: sized by the bytes the step
 * moves, window bytes x rows); <= 1024.
 *
 * smx_record_ddpg_nstep_step_f32: one step of ExpSenderWrapperSSARNStepBootstrap per actor, N = n_step:
 *   slot tau % N of carry_obs / carry_act / carry_rew <- cur_obs, step_actions, step_rewards
 *   tau >= N - 1 (what rank >= 0 must mean): transition j = tau - N + 1, in slot (tau + 1) % N, goes to its row: obs = s_j,
 *     actions = a_j, obs_next = step_obs_next[a], dones = step_dones[a], rewards = the fp64 sum of
 *     smx_synth_ddpg_rollout_f32 (gpow [N] = gamma ** e, fp64; the wrapper's fill-up exponents) rounded once
 *   the last N - 1 transitions of an episode are never written (the host restarts the clock).
 * n > capacity: SMX_E_SHAPE (every actor may close in one step). */
struct smx_record_ppo_window_step {        /* (by tag: no typedef) */
    int32_t n, D, A, hidden;               /* hidden: the LSTM's units (0: a policy without one) */
    int32_t n_step, advance, rows, copy_workgroups;
    const int32_t* t;
    const int32_t* rank;
    const int32_t* t_host;                 /* NULL: not checked on the host */
    const int32_t* rank_host;
    float* cur_obs;
    const float* step_actions;
    const float* step_pds;
    const float* h_before;                 /* [n, hidden] the LSTM state the step started from, or NULL */
    const float* c_before;
    const float* step_obs_next;
    const float* step_rewards;
    const float* step_dones;
    const float* step_obs_reset;           /* NULL: no actor is done */
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* carry_pd;
    float* carry_cells;                    /* NULL without an LSTM */
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    float* pds;
    float* cells;                          /* NULL without an LSTM */
    int64_t cursor, capacity;
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
int smx_record_ppo_window_step_f32(const struct smx_record_ppo_window_step* args, smx_stream_t stream);

struct smx_record_ddpg_nstep_step {        /* (by tag: no typedef) */
    int32_t n, D, A, n_step;
    int32_t rows, reserved;
    const int32_t* t;
    const int32_t* rank;
    const int32_t* t_host;                 /* NULL: not checked on the host */
    const int32_t* rank_host;
    float* cur_obs;
    const float* step_actions;
    const float* step_obs_next;
    const float* step_rewards;
    const float* step_dones;
    const float* step_obs_reset;           /* NULL: no actor is done */
    const double* gpow;
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    int64_t cursor, capacity;
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
int smx_record_ddpg_nstep_step_f32(const struct smx_record_ddpg_nstep_step* args, smx_stream_t stream);

/* The same two steps for host-stepped actors WITH A CAMERA (the reference's pixel configurations: FrameStackWrapper,
 * surreal/env/wrapper.py:407-472, between the simulator and the experience wrappers of surreal/env/
 * exp_sender_wrapper.py:72-112 and 153-264; ppo_configs.py / ddpg_configs.py:176-228 with pixel_input, frame_stacks 3):
 * everything smx_record_ppo_window_step_f32 / smx_record_ddpg_nstep_step_f32 do -- rings, windows, n-step reward, cells,
 * monitor, the t / rank / rows guards and the t_host / rank_host check -- and, in the same launch, the frames.  The
 * simulators emit ONE raw uint8 frame per step; the stacking is done here.  F = C*H*W bytes per frame, S = frame_stacks,
 * N = n_step, tau = t[a], Hd = hist_len >= N + S, p = hist_pos: ONE counter for all actors, which the caller advances by
 * 1 (mod Hd) per launch, because every actor receives exactly one frame per step:
 *   step_frame_next [n, F]   the frame after the step (the terminal frame where step_dones[a] != 0)
 *   step_frame_reset [n, F]  the first frame of the next episode: only the rows of done actors are read; NULL: no actor
 *                            is done (a done actor then goes on from step_frame_next, as cur_obs does from
 *                            step_obs_next without a step_obs_reset)
 *   history:  hist[a, (p - tau + u) mod Hd] holds the raw frame of step u of actor a's current episode, u <= tau
 *   stacked(u)[i] = frame of step max(u - S + 1 + i, 0), 0 <= i < S                        (stack_sources)
 *   hist[a, (p + 1) mod Hd] = step_frame_reset[a] where done, else step_frame_next[a]: the terminal frame never enters
 *             the history
 *   obs_pixel[a] = step_frame_reset[a] S times where done, else stacked(tau + 1) (its last frame: step_frame_next[a])
 *   PPO, closing window j = tau + 1 - N into its row: pixel[row, u] = stacked(j + u), u < N; pixel_next[row] =
 *             stacked(tau + 1), its last frame step_frame_next[a]: the terminal frame on done
 *   DDPG, emitting step into its row: pixel[row] = stacked(tau - N + 1); pixel_next[row] = stacked(tau + 1)
 * pixel is uint8 [capacity, N, S*F] (DDPG: [capacity, S*F]), pixel_next [capacity, S*F], obs_pixel [n, S*F] (what the
 * actors act on next), hist [n, Hd, F].  The frames a launch reads from the history are those of episode steps
 * max(tau - N - S + 2, 0) .. tau; the slot it writes is that of step tau + 1 - Hd <= tau - N - S + 1, and the step's own
 * frames come from the inputs: no workgroup reads what another one writes in the same launch.
 * Grid: per actor one workgroup does the low-dimensional step and stores step_frame_next wherever it goes;
 * copy_workgroups further workgroups per actor split the other destination frames (0: sized by the bytes the step moves
 * -- a closing PPO step has (N + 1) S - 1 destination frames more than any other; <= 1024).  16-byte accesses when
 * F % 16 == 0 and all six frame buffers sit on 16 bytes, single bytes otherwise.  No atomics.
 * Limits beyond those of the low-dimensional entry points (D >= 1 among them: an observation without a low-dimensional
 * part is not taken): C, H, W, frame_stacks >= 1, hist_len >= n_step + frame_stacks, 0 <= hist_pos < hist_len
 * (SMX_E_SHAPE); hist, pixel, pixel_next, obs_pixel, step_frame_next non-NULL (SMX_E_NULL); n <= capacity (SMX_E_SHAPE).
 * The actors lie on the grid's x axis: no limit on n of its own. */
struct smx_record_ppo_pixel_window_step {  /* (by tag: no typedef) */
    int32_t n, D, A, hidden;               /* hidden: the LSTM's units (0: a policy without one) */
    int32_t n_step, advance, rows, copy_workgroups;
    const int32_t* t;
    const int32_t* rank;
    const int32_t* t_host;                 /* NULL: not checked on the host */
    const int32_t* rank_host;
    float* cur_obs;
    const float* step_actions;
    const float* step_pds;
    const float* h_before;                 /* [n, hidden] the LSTM state the step started from, or NULL */
    const float* c_before;
    const float* step_obs_next;
    const float* step_rewards;
    const float* step_dones;
    const float* step_obs_reset;           /* NULL: no actor is done */
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* carry_pd;
    float* carry_cells;                    /* NULL without an LSTM */
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    float* pds;
    float* cells;                          /* NULL without an LSTM */
    int64_t cursor, capacity;
    int32_t C, H, W, frame_stacks;
    int32_t hist_len, hist_pos;
    const uint8_t* step_frame_next;        /* [n, F] */
    const uint8_t* step_frame_reset;       /* [n, F], or NULL: no actor is done */
    uint8_t* hist;                         /* [n, Hd, F] */
    uint8_t* pixel;                        /* [capacity, N, S*F] */
    uint8_t* pixel_next;                   /* [capacity, S*F] */
    uint8_t* obs_pixel;                    /* [n, S*F] */
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
int smx_record_ppo_pixel_window_step(const struct smx_record_ppo_pixel_window_step* args, smx_stream_t stream);

struct smx_record_ddpg_pixel_nstep_step {  /* (by tag: no typedef) */
    int32_t n, D, A, n_step;
    int32_t rows, copy_workgroups;
    const int32_t* t;
    const int32_t* rank;
    const int32_t* t_host;                 /* NULL: not checked on the host */
    const int32_t* rank_host;
    float* cur_obs;
    const float* step_actions;
    const float* step_obs_next;
    const float* step_rewards;
    const float* step_dones;
    const float* step_obs_reset;           /* NULL: no actor is done */
    const double* gpow;
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    int64_t cursor, capacity;
    int32_t C, H, W, frame_stacks;
    int32_t hist_len, hist_pos;
    const uint8_t* step_frame_next;        /* [n, F] */
    const uint8_t* step_frame_reset;       /* [n, F], or NULL: no actor is done */
    uint8_t* hist;                         /* [n, Hd, F] */
    uint8_t* pixel;                        /* [capacity, S*F] */
    uint8_t* pixel_next;                   /* [capacity, S*F] */
    uint8_t* obs_pixel;                    /* [n, S*F] */
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
int smx_record_ddpg_pixel_nstep_step(const struct smx_record_ddpg_pixel_nstep_step* args, smx_stream_t stream);

/* smx_record_ddpg_pixel_nstep_step in the frame-pool layout (above smx_synth_ddpg_pixel_pool_step; the reference's
 * frame_stack_concatenate_on_env: False, surreal/main/ddpg_configs.py:119-122, with the n-step wrapper of
 * surreal/env/exp_sender_wrapper.py:72-112): the low-dimensional step, rings, n-step reward, monitor and the t / rank /
 * rows guards exactly as smx_record_ddpg_nstep_step_f32, the rows where it puts them; the frames once, in the pool.  A
 * terminal step brings two frames, so every actor has counters of its own: counters_in int64 [2, n] = f | first before the
 * step (f: the counter of the actor's current frame, first: of its episode's reset frame), counters_out [2, n] after it
 * (another buffer: the caller swaps the two per launch).  With restart = step_dones[a] != 0 and step_frame_reset given:
 *   pool[a, (f + 1) mod P] = step_frame_next[a];  restart: pool[a, (f + 2) mod P] = step_frame_reset[a]
 *   obs_pixel[a] = stack(f + 1) over `first`;     restart: step_frame_reset[a] S times
 *   counters_out = (f + 1, first);                restart: (f + 2, f + 2)
 *   a closing actor's row: frame_next = f + 1, frame_first = first, frame_actor = a.
 * pool_len < n_step + S + 1, counters_in == counters_out: SMX_E_SHAPE; the counter arrays off their element size:
 * SMX_E_ALIGN. */
struct smx_record_ddpg_pixel_pool_nstep_step {  /* (by tag: no typedef) */
    int32_t n, D, A, n_step;
    int32_t rows, copy_workgroups;
    const int32_t* t;
    const int32_t* rank;
    const int32_t* t_host;                 /* NULL: not checked on the host */
    const int32_t* rank_host;
    float* cur_obs;
    const float* step_actions;
    const float* step_obs_next;
    const float* step_rewards;
    const float* step_dones;
    const float* step_obs_reset;           /* NULL: no actor is done */
    const double* gpow;
    float* carry_obs;
    float* carry_act;
    float* carry_rew;
    float* obs;
    float* obs_next;
    float* actions;
    float* rewards;
    float* dones;
    int64_t cursor, capacity;
    int32_t C, H, W, frame_stacks;
    int64_t pool_len;                      /* P */
    const uint8_t* step_frame_next;        /* [n, F] */
    const uint8_t* step_frame_reset;       /* [n, F], or NULL: no actor is done */
    uint8_t* pool;                         /* [n, P, F] */
    uint8_t* obs_pixel;                    /* [n, S*F] */
    const int64_t* counters_in;            /* [2, n] */
    int64_t* counters_out;                 /* [2, n] */
    int64_t* frame_next;                   /* [capacity] */
    int64_t* frame_first;
    int32_t* frame_actor;
    struct smx_episode_monitor mon;        /* mon.ep_reward NULL: none (stays the last member) */
};
int smx_record_ddpg_pixel_pool_nstep_step(const struct smx_record_ddpg_pixel_pool_nstep_step* args, smx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Data-parallel exchange between the learner ranks of one node over IPC-mapped peer buffers (xGMI loads): the
 * collectives N sharded learners need to equal the single reference learner -- the per-epoch
 * [gradients | loss partial rows] sum of surreal/learner/ppo.py:541-562 run on shards, the advantage moments
 * (ppo.py:413-416), the end-of-learn statistics -- as ONE kernel each inside the learner's hipGraph instead of an
 * eager RCCL call between graph segments (csrc/smx_xchg.hip has the protocol).  The reference has no counterpart (one
 * learner process); the host-side fallback is torch.distributed (RCCL).
 *
 * Set-up, once per learner workspace: every rank  smx_xchg_alloc()s a buffer of smx_xchg_bytes(capacity, world),
 * smx_xchg_export()s its 64-byte handle, the handles travel through the process group, every rank smx_xchg_open()s
 * its peers' handles and fills smx_xchg_t.peer[] (peer[rank] = its own buffer), then a barrier.  These are the only
 * entry points of the library that allocate or synchronise.
 * Exchanges: issued by every rank in the same order on ONE stream per exchange context; the sequence number lives in
 * the buffer, so a captured graph replays.  err (nullable): a device int32 into which a timed-out wait ORs
 * 0x100 | phase << 4 | peer (the caller reads it back with its statistics); after an error no wait blocks any more.
 * Results are bit-identical on all ranks (rank c alone reduces chunk c, summing the ranks in rank order). */
#define SMX_XCHG_MAX_RANKS 8
#define SMX_XCHG_HANDLE_BYTES 64
typedef struct {
    int32_t world, rank;
    int64_t capacity;                      /* floats one exchange may carry */
    void* peer[SMX_XCHG_MAX_RANKS];        /* every rank's buffer as mapped in THIS process */
} smx_xchg_t;
int64_t smx_xchg_bytes(int64_t capacity_floats, int32_t world);
/* kind (nullable) <- 0 uncached, 1 fine-grained, 2 plain device memory (what the runtime granted); timeout_s: bound of
 * every in-kernel wait (<= 0: 2 s).  Zero-fills and synchronises `stream`. */
int smx_xchg_alloc(int64_t bytes, double timeout_s, void** ptr, int32_t* kind, smx_stream_t stream);
int smx_xchg_free(void* ptr);
int smx_xchg_export(void* ptr, void* handle64);
int smx_xchg_open(const void* handle64, void** ptr);
int smx_xchg_close(void* ptr);
/* out[0, n) = sum over ranks of in[0, n); in == out allowed; 16-byte aligned; n <= capacity */
int smx_xchg_allreduce_f32(const smx_xchg_t* x, const float* in, float* out, int64_t n, int32_t* err,
                           smx_stream_t stream);
/* out [world, n_per_rank] <- every rank's in[0, n_per_rank); world * n_per_rank <= capacity */
int smx_xchg_allgather_f32(const smx_xchg_t* x, const float* in, int64_t n_per_rank, float* out, int32_t* err,
                           smx_stream_t stream);
/* seq_err_dev[2] (device) <- {exchanges completed, error word} of this rank's buffer */
int smx_xchg_status(const smx_xchg_t* x, uint32_t* seq_err_dev, smx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SURREAL_AMD_H */
