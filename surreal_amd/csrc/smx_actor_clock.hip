// Episode clocks per actor for the one-launch rollouts (struct smx_actor_clock_rows, include/surreal_amd.h): the ring
// row offsets of a call's closing records as a pure function of the clocks.  Actor a starts the call at clock t[a] of
// an episode of episode_len[a] steps; at the call's step s its clock is tau = (t[a] + s) % episode_len[a], and it closes
// a record there iff j = tau + 1 - N >= 0 and j % adv == 0.  The closing pairs (s, a) are numbered s ascending, then a
// ascending -- the order n host wrappers stepped in actor order insert in:
//   row_off[s, a] = sum over a' of cnt_a'(s) + #{a' < a closing at s}    (-1 where (s, a) closes nothing)
// with cnt_a(s) the closings of actor a in its first s steps, a closed form (closings_before).  One launch, workgroup s
// forms row s of the table: it sums cnt over the actors, then scans the step's closing flags in actor order -- a ballot
// and a popcount per wavefront, the wavefronts' totals through LDS.  Integers only, no atomics.
#include "smx_common.h"

namespace {

constexpr int CLK_THREADS = 256;
constexpr int CLK_WAVES = CLK_THREADS / 64;

struct ClockRows {
    int n, N, adv;
    const int32_t *t, *L;
    int32_t* row_off;
};

// records with x = tau + 1 <= `x` closed since the episode's start: x = N, N + adv, ...
__device__ __forceinline__ long long closed_by(long long x, int N, int adv) { return x >= N ? (x - N) / adv + 1 : 0; }

// the closings of an actor in its first s steps from clock t0 of episodes of L steps: the rest of the open episode, the
// whole episodes behind it, the begun one
__device__ __forceinline__ long long closings_before(long long t0, long long L, long long s, int N, int adv) {
    const long long m = s < L - t0 ? s : L - t0, r = s - m;
    return closed_by(t0 + m, N, adv) - closed_by(t0, N, adv) + (r / L) * closed_by(L, N, adv) + closed_by(r % L, N, adv);
}

__global__ __launch_bounds__(CLK_THREADS) void actor_clock_rows_kernel(ClockRows G) {
    __shared__ long long s_sum[CLK_WAVES];
    __shared__ int s_cnt[CLK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long s = blockIdx.x;
    // ---- the records all actors closed before step s --------------------------------------------------------------
    long long before = 0;
    for (int a = tid; a < G.n; a += CLK_THREADS) {
        const long long L = G.L[a], t0 = G.t[a];
        if (L >= 1 && t0 >= 0 && t0 < L) before += closings_before(t0, L, s, G.N, G.adv);
    }
    for (int o = 32; o > 0; o >>= 1) before += __shfl_down(before, o);
    if (lane == 0) s_sum[wv] = before;
    __syncthreads();
    long long base = 0;
    for (int w = 0; w < CLK_WAVES; ++w) base += s_sum[w];
    // ---- the step's closing actors in actor order, CLK_THREADS of them at a time ------------------------------------
    for (int a0 = 0; a0 < G.n; a0 += CLK_THREADS) {
        const int a = a0 + tid;
        bool closes = false;
        if (a < G.n) {
            const long long L = G.L[a], t0 = G.t[a];
            if (L >= 1 && t0 >= 0 && t0 < L) {
                const long long j = (t0 + s) % L + 1 - G.N;
                closes = j >= 0 && j % G.adv == 0;
            }
        }
        const unsigned long long votes = __ballot(closes);
        const int ahead = __popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wv] = __popcll(votes);
        __syncthreads();
        long long off = base + ahead;
        int total = 0;
        for (int w = 0; w < CLK_WAVES; ++w) {
            if (w < wv) off += s_cnt[w];
            total += s_cnt[w];
        }
        // (n * steps < 2^31: every offset fits the table's int32)
        if (a < G.n) G.row_off[s * G.n + a] = closes ? (int32_t)off : -1;
        base += total;
        __syncthreads();
    }
}

}  // namespace

extern "C" int smx_actor_clock_rows_i32(const struct smx_actor_clock_rows* a, smx_stream_t stream) {
    SMX_REQUIRE(a && a->t && a->episode_len && a->row_off, SMX_E_NULL);
    SMX_REQUIRE(a->n > 0 && a->steps > 0 && a->n_step > 0 && a->advance >= 1 && a->advance <= a->n_step, SMX_E_SHAPE);
    SMX_REQUIRE((long long)a->n * a->steps < (1ll << 31), SMX_E_SHAPE);
    for (int i = 0; i < a->n; ++i) {
        SMX_REQUIRE(!a->episode_len_host || a->episode_len_host[i] >= 1, SMX_E_SHAPE);
        SMX_REQUIRE(!a->t_host || a->t_host[i] >= 0, SMX_E_SHAPE);
        SMX_REQUIRE(!(a->t_host && a->episode_len_host) || a->t_host[i] < a->episode_len_host[i], SMX_E_SHAPE);
    }
    ClockRows G;
    G.n = a->n; G.N = a->n_step; G.adv = a->advance;
    G.t = a->t; G.L = a->episode_len; G.row_off = a->row_off;
    hipLaunchKernelGGL(actor_clock_rows_kernel, dim3(a->steps), dim3(CLK_THREADS), 0, smx_s(stream), G);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}
